// midaspom_amd/csrc/spom_future_plan.h -- host planning of the future
// engine's patch-parallel kernel k_future_wide<NP> (spom_future.hip): the
// options of mdp_future_create_opts, the two-sided distance image, the
// lane-owned bit layout of the occupancy and the un-interleaving of the
// states the kernel writes.  No HIP runtime call (spom_future_plan.cpp links
// into future_plan_check.cpp as it links into libmidaspom.so).
#ifndef SPOM_FUTURE_PLAN_H
#define SPOM_FUTURE_PLAN_H
#include <cstdint>
#include <vector>

#include "mdp_internal.h"

constexpr uint32_t kFutLaneMaxN = 64;     // k_future<NM>: one replicate per lane
constexpr uint32_t kFutWideMaxN = 1024;   // k_future_wide<8>: 8 patch pairs per lane
constexpr uint32_t kFutMaxMissing = 30;   // npstates = 2^nmiss fits an int
constexpr uint64_t kFutStatesMaxWords = 1ull << 20;  // mdp_future_states: nrep * W (8 MiB of words)

enum FutWideMode { kFutWideOff = 0, kFutWideAuto = 1, kFutWideOn = 2 };

// "NAME=VALUE" pairs in the grammar of mdp_engine_create_opts (separators
// ';', ',' or white space); NULL or "" leaves the default, kFutWideOff.
// MDP_FUT_WIDE = 0 | auto | 1; any other name or value is MDP_EINVAL.
int fut_parse_opts(const char *s, FutWideMode *mode);

// the kernel a survey row of n patches runs under `mode`: *np = 0 for the
// lane kernels, else the NP of k_future_wide<NP> (patch pairs per lane:
// 1, 2, 4, 8 for n <= 128, 256, 512, 1024).  MDP_EUNSUPPORTED beyond the
// mode's limit.
int fut_select_kernel(uint32_t n, FutWideMode mode, uint32_t *np);

// Lane lambda of a wave owns the patch pairs m = lambda + 64*j, j < NP, that
// is patches 2m and 2m+1; its occupancy word holds patch 2m + p in bit 2j + p.
struct FutWidePlan {
    uint32_t n = 0, np = 0, nmiss = 0;
    // doubles per copy of the distance image (even): n + 128*NP, so that the
    // pair of every lane, padded pairs included, is inside it for every l < n
    uint32_t len = 0;
    // image[0 .. len): G, image[len .. 2*len): G shifted by one double, where
    // G[i] = exp(-a*|i - (n-1)|*d)*K_D for i <= 2n-2, G[n-1] = 0.0, 0.0 beyond:
    // M[l][k]*K_D = G[k - l + n-1].  Lane pair m of survivor l reads the
    // 16-byte slot m + slot0(l) (fut_wide_slot0) of the image as double2.
    std::vector<double> image;
    std::vector<double> src;      // [128*NP] M[n][k]*K_S, 0.0 for k >= n
    std::vector<uint32_t> occ0;   // [64] occupied bits of the last survey, per lane
    std::vector<uint32_t> miss;   // [nmiss] (lane << 8) | bit of each missing patch, in patch order
};

// first 16-byte slot of survivor l's row: slots m + slot0 hold
// (M[l][2m]*K_D, M[l][2m+1]*K_D) for every pair m
inline uint32_t fut_wide_slot0(uint32_t n, uint32_t len, uint32_t l)
{
    const uint32_t base = n - 1 - l;  // index in G of patch 0's entry
    return (base & 1u) ? (len + base - 1) >> 1 : base >> 1;
}

// the last survey row (values -1 / 0 / 1, <= 30 missing) and the dispersal
// parameters into the plan; n and np as fut_select_kernel gave them
int fut_wide_plan(const int32_t *last_row, uint32_t n, uint32_t np, double m, double d, double KD, double KS,
                  double dS, FutWidePlan *plan);

// lanes[r*64 + lambda] (the kernel's output) -> words[r*W + k/64] bit k%64,
// W = ceil(n/64)
void fut_wide_unpack(const uint32_t *lanes, uint64_t nrep, uint32_t n, uint32_t np, uint64_t *words);

#endif
