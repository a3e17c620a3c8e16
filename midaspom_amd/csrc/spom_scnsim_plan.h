// midaspom_amd/csrc/spom_scnsim_plan.h -- host planning of the simulated
// scenario likelihoods (spom_scnsim.hip, k_scnsim<NM> and the patch-parallel
// k_scnsim_wave<NP>): the options of mdp_scenario_sim_create and the kernel
// they select, every refusal, the unscaled dispersal table (or, for the wave
// kernel, the two-sided distance image) and the source rows, the row's fixed
// / missing masks with the completion numbering and float priors of
// dieoff.c:205-232, and the cutting of grid points and replicates into
// launches.  No HIP runtime call
// (spom_scnsim_plan.cpp links into scnsim_plan_check.cpp as it links into
// libmidaspom.so).
#ifndef SPOM_SCNSIM_PLAN_H
#define SPOM_SCNSIM_PLAN_H
#include <cstdint>
#include <vector>

#include "mdp_internal.h"

constexpr uint32_t kSimMaxN = 64;                 // k_scnsim<NM>: one 64-bit occupancy mask per replicate
constexpr uint32_t kSimWaveMaxN = 1024;           // k_scnsim_wave<8>: 8 patch pairs per lane
constexpr uint32_t kSimWaveReps = 4;              // replicates per work tile of the wave kernel: one per wave
constexpr uint32_t kSimMaxMatchMissing = 10;      // match: 2^nmiss completions per grid point
constexpr uint32_t kSimMaxYears = 12288;          // ts + tdis, as the future engine's tfut
constexpr uint64_t kSimMaxPoints = 1ull << 20;
constexpr uint64_t kSimMaxCells = 1ull << 24;     // cells of either table (128 MiB of 64-bit counters)
constexpr uint64_t kSimMaxReps = 1ull << 31;      // replicates per call
constexpr uint32_t kSimBlock = 256;               // replicates per work tile (one workgroup pass)
constexpr uint32_t kSimMaxWG = 4096;              // grid-stride cap, as k_future

// padded patch count NM of k_scnsim<NM> for n <= 64 patches
constexpr uint32_t sim_nm(uint32_t n) { return n <= 8 ? 8 : n <= 16 ? 16 : n <= 32 ? 32 : 64; }

// patch pairs per lane NP of k_scnsim_wave<NP> for n <= 1024 patches
constexpr uint32_t sim_np(uint32_t n) { return n <= 128 ? 1 : n <= 256 ? 2 : n <= 512 ? 4 : 8; }

enum SimWaveMode { kSimWaveOff = 0, kSimWaveAuto = 1, kSimWaveOn = 2 };

struct SimOpts {
    uint32_t nm = 0;          // MDP_SIM_NM (0: sim_nm(n))
    uint32_t np = 0;          // MDP_SIM_NP (0: sim_np(n))
    SimWaveMode wave = kSimWaveOff;  // MDP_SIM_WAVE
    uint64_t launch_pts = 0;  // MDP_SIM_LAUNCH_PTS (0: no cap)
};

// "NAME=VALUE" pairs in the grammar of the other _opts calls (separators ';',
// ',' or white space); NULL or "" leaves the defaults.  MDP_SIM_WAVE = 0 |
// auto | 1, MDP_SIM_NM = 8 | 16 | 32 | 64, MDP_SIM_NP = 1 | 2 | 4 | 8,
// MDP_SIM_LAUNCH_PTS = decimal >= 0; anything else is MDP_EINVAL.
int sim_parse_opts(const char *s, SimOpts *o);

// What k_scnsim<NM> or k_scnsim_wave<NP> is given of the survey row and the
// dispersal parameters.  np = 0: the lane kernel (nm, live, fixed, missmask
// and M are its); np > 0: the wave kernel (nm = 0, M empty; wlen, image,
// wfixed, wmissmask and wmiss are its).  Lane lambda of a wave owns the patch
// pairs lambda + 64*j, j < NP; its words hold patch 2*(lambda + 64*j) + p in
// bit 2*j + p (the layout of FutWidePlan, spom_future_plan.h).
struct SimPlan {
    uint32_t n = 0, nm = 0, np = 0, nmiss = 0;
    int kind = 0;                 // 0 die-off, 1 habitat loss
    double m = 400.0;
    uint64_t live = 0;            // bits 0..n-1
    uint64_t fixed = 0;           // bit k = patch k observed occupied
    uint64_t missmask = 0;        // bit k = patch k missing
    std::vector<uint32_t> miss;   // [nmiss] the missing patches, ascending: completion j holds
                                  //   patch miss[q] in bit nmiss-1-q (the first missing is the MSB)
    std::vector<double> M;        // [nm][nm] exp(-(1/m)|l-k|d), 0.0 on the diagonal and in the padding
    std::vector<float> prior;     // [2^nmiss] dieoff.c:230 (empty when nmiss > kSimMaxMatchMissing)
    // doubles per copy of the distance image (even): n + 128*NP, rounded up
    uint32_t wlen = 0;
    // image[0 .. wlen): G, image[wlen .. 2*wlen): G shifted by one double,
    // G[i] = exp(-(1/m)|i - (n-1)|d) for i <= 2n-2 (M's expression and bits),
    // G[n-1] = 0.0, 0.0 beyond; unscaled, so one image serves every grid
    // point.  Slots as fut_wide_slot0 (spom_future_plan.h) addresses them.
    std::vector<double> image;
    std::vector<uint32_t> wfixed;     // [64] observed-occupied bits per lane
    std::vector<uint32_t> wmissmask;  // [64] missing bits per lane
    std::vector<uint32_t> wmiss;      // [nmiss] (lane << 8) | bit of each missing patch, in patch order
    SimOpts opts;
};

// doubles per source row: nm, or 128*NP
inline uint32_t sim_src_ld(const SimPlan &plan) { return plan.np ? 128 * plan.np : plan.nm; }

// refusals of mdp_scenario_sim_create, then the plan
int sim_plan(const int32_t *row, uint32_t n, double m, float p, double d, int kind, const SimOpts &opts,
             SimPlan *plan);

// src[id][k] = exp(-(1/m)(k+1) dsrc[id]) (loss.c:250-251), k < n, 0.0 in the padding: [nd][sim_src_ld]
void sim_src(const SimPlan &plan, const double *dsrc, uint32_t nd, std::vector<double> *src);

// The launches of one call: grid points [p0, p0 + npts) each, every point
// over all the call's replicates in tiles of kSimBlock (lane kernel: one
// replicate per lane) or kSimWaveReps (wave kernel: one per wave).
struct SimLaunch {
    uint64_t p0 = 0, npts = 0;
    uint64_t tiles = 0;   // npts * tiles_per_point
    uint32_t nwg = 0;     // min(tiles, kSimMaxWG)
};

struct SimCall {
    uint64_t G = 0;                // grid points ne*nc*nK*nd
    uint64_t tiles_per_point = 0;  // ceil(nrep / kSimBlock), or ceil(nrep / kSimWaveReps)
    uint64_t hist_cells = 0, match_cells = 0;  // G*(n+1), G << nmiss
    std::vector<SimLaunch> launches;
};

// refusals of mdp_scenario_sim_tables (and _device, _time_kernel), then the cut
int sim_call(const SimPlan &plan, int ts, int tdis, const double *e, uint32_t ne, const double *c, uint32_t nc,
             const double *K, uint32_t nK, const double *dsrc, uint32_t nd, uint64_t nrep, bool want_hist,
             bool want_match, SimCall *call);

// out[g] = (sum_j (double)prior_j * (double)match[g][j], j ascending) * 2^n / nrep
// for n <= 64; ldexp(sum / nrep, n) beyond (2^n itself overflows at n = 1024)
int sim_lik(const SimPlan &plan, const uint64_t *match, size_t npoints, uint64_t nrep, double *out);

#endif
