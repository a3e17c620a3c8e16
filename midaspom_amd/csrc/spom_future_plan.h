// midaspom_amd/csrc/spom_future_plan.h -- host planning of the future engine
// (spom_future.hip), both kernel families: the options of
// mdp_future_create_opts and the kernel they select, the cumulative posterior
// the sampler searches, the lane kernels' k_future<NM> occupancy mask and
// dispersal table, and for the patch-parallel k_future_wide<NP> the two-sided
// distance image, the lane-owned bit layout of the occupancy and the
// un-interleaving of the states the kernel writes.  No HIP runtime call
// (spom_future_plan.cpp links into future_plan_check.cpp as it links into
// libmidaspom.so).
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
// MDP_FUT_WIDE = 0 | auto | 1; MDP_FUT_SUM_YEARS = 0..12288 (decimal; the cap
// on the summary path's years per window, 0 = the planner's own choice); any
// other name or value is MDP_EINVAL.
int fut_parse_opts(const char *s, FutWideMode *mode, uint32_t *sum_years = nullptr);

// the kernel a survey row of n patches runs under `mode`: *np = 0 for the
// lane kernels, else the NP of k_future_wide<NP> (patch pairs per lane:
// 1, 2, 4, 8 for n <= 128, 256, 512, 1024).  MDP_EUNSUPPORTED beyond the
// mode's limit.
int fut_select_kernel(uint32_t n, FutWideMode mode, uint32_t *np);

// padded patch count NM of the lane kernel k_future<NM> of n <= 64 patches
constexpr uint32_t fut_lane_nm(uint32_t n) { return n <= 8 ? 8 : n <= 16 ? 16 : n <= 32 ? 32 : 64; }

// What k_future<NM> is given of the last survey row and the dispersal
// parameters (future.c:266-277, :292-323).
struct FutLanePlan {
    uint32_t n = 0, nm = 0, nmiss = 0;
    uint64_t occ0 = 0;            // bit k = patch k occupied in the last survey
    std::vector<uint64_t> miss;   // [nmiss] the bit of each missing patch, in patch order
    std::vector<double> MK;       // [nm][nm] M[l][k]*K_D, 0.0 on the diagonal and in the padding
    std::vector<double> src;      // [nm] M[n][k]*K_S, 0.0 for k >= n
};

// the last survey row (values -1 / 0 / 1, <= 30 missing) of n <= 64 patches
// and the dispersal parameters into the plan
int fut_lane_plan(const int32_t *last_row, uint32_t n, double m, double d, double KD, double KS, double dS,
                  FutLanePlan *plan);

// The trapezoid-weighted cumulative posterior in the reference's scan order
// (:362-369), for both families.
struct FutPostPlan {
    std::vector<double> pcum;  // [necstep^2]
    uint32_t lvalid = 0;       // cells the sampler searches: up to the first NaN; 0 when the mass is not positive
    double pscale = 0.0;       // (double)((necstep-1)*(necstep-1)) (:361)
};

// MDP_EUNSUPPORTED for a cumulative sum that decreases before the first NaN
// (a negative cell); post may be null when necstep is 0
int fut_post_plan(const double *post, uint32_t necstep, FutPostPlan *plan);

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
// (M[l][2m]*K_D, M[l][2m+1]*K_D) for every pair m (constexpr: host and device)
constexpr uint32_t fut_wide_slot0(uint32_t n, uint32_t len, uint32_t l)
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

// ---------------------------------------------------------------------------
// The summary path (mdp_future_summary): hist[t][m] and occ[t][k] accumulate
// in LDS over windows of years, one launch per window; between windows every
// replicate rests in a record in device memory (its posterior cell and its
// occupancy: 8 bytes of mask, or the 64 lane words of k_future_wide).
// ---------------------------------------------------------------------------
constexpr uint32_t kFutSumMaxT = 12288;          // as simulate
constexpr uint64_t kFutSumMaxCells = 1ull << 21; // tfut * (2n+1): 16 MiB of 64-bit counters
constexpr uint32_t kFutSumTableBytes = 16384;    // LDS of one window's table
constexpr uint64_t kFutSumOneWindowReps = 1ull << 31;  // replicates per launch: no 32-bit LDS cell can wrap
constexpr uint64_t kFutSumLaneReps = 1ull << 20;  // replicates per launch when records are kept:
constexpr uint64_t kFutSumWideReps = 1ull << 16;  //   12 MiB (lane), 16.25 MiB (wide) of records

struct FutSumPlan {
    uint32_t cells = 0;    // 32-bit LDS cells per year: n+1 of hist, then n (lane kernels) or
                           //   128*NP in lane order (k_future_wide) of occ
    uint32_t years = 0;    // years per window
    uint32_t windows = 0;  // ceil(tfut / years)
    uint32_t lds = 0;      // dynamic LDS of a launch: fixed tables + years*cells*4
    uint32_t maxwg = 0;    // grid cap: the workgroups 256 CUs hold at the kernel's VGPR count (every
                           //   workgroup flushes its window once per launch)
    uint64_t reps = 0;     // replicates per launch
};

// np = 0: the lane kernels (16 KB survivor table when n <= 8), else
// k_future_wide<np> with `wlen` doubles per copy of the image; cap = the
// MDP_FUT_SUM_YEARS option.  MDP_EUNSUPPORTED for tfut outside 1..12288 or
// more than 2^21 cells.
int fut_sum_plan(uint32_t n, uint32_t np, uint32_t wlen, uint32_t tfut, uint32_t cap, FutSumPlan *plan);

// global cell (of 2n+1 per year: hist, then occ in patch order) of LDS cell c
// of a year in k_future_wide's layout, or -1 for a padded patch
// (constexpr: host and device)
constexpr int32_t fut_sum_wide_cell(uint32_t n, uint32_t c)
{
    if (c <= n) return (int32_t)c;
    const uint32_t b = (c - n - 1) >> 6, lam = (c - n - 1) & 63u;
    const uint32_t k = 2 * (lam + 64 * (b >> 1)) + (b & 1u);
    return k < n ? (int32_t)(n + 1 + k) : -1;
}

#endif
