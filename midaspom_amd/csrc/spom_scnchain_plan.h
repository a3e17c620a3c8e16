// midaspom_amd/csrc/spom_scnchain_plan.h -- host planning of the count-class
// chain likelihoods (spom_scnchain.hip, k_scnchain<NM> and k_chain_eval): the
// options of mdp_scenario_chain_create, every refusal, the unscaled dispersal
// table and the source rows (spom_scn_row.h, the simulator's bytes), the
// default target weights, the cut of a call's grid points into launches with
// the workgroups that share a point, and the host form of the chain
// evaluation.  No HIP runtime call (spom_scnchain_plan.cpp links into
// scnchain_plan_check.cpp as it links into libmidaspom.so).
#ifndef SPOM_SCNCHAIN_PLAN_H
#define SPOM_SCNCHAIN_PLAN_H
#include <cstdint>
#include <vector>

#include "mdp_internal.h"

constexpr uint32_t kChainMaxN = 64;              // one 64-bit occupancy mask per replicate
constexpr uint32_t kChainMaxYears = 12288;       // ts + tdis, as the simulator's
constexpr uint64_t kChainMaxPoints = 1ull << 20;
constexpr uint64_t kChainMaxCells = 1ull << 24;  // cells of a host table of _counts
constexpr uint64_t kChainMaxReps = 1ull << 31;   // replicates per class and call: a cell fits 32 bits
constexpr uint32_t kChainBlock = 256;            // replicates per work tile (one workgroup pass)
constexpr uint32_t kChainMaxWG = 4096;           // grid-stride cap, as k_scnsim
constexpr uint32_t kChainFillWG = 2048;          // workgroups a launch is spread over when its points are fewer
constexpr uint64_t kChainTableBytes = 256ull << 20;  // the device count table of one launch (32-bit cells)
constexpr uint32_t kChainEvalBlock = 128;        // k_chain_eval: one thread per class, two waves for n = 64

// padded patch count NM of k_scnchain<NM>
constexpr uint32_t chain_nm(uint32_t n) { return n <= 8 ? 8 : n <= 16 ? 16 : n <= 32 ? 32 : 64; }

struct ChainOpts {
    uint32_t nm = 0;          // MDP_CHAIN_NM (0: chain_nm(n))
    uint64_t launch_pts = 0;  // MDP_CHAIN_LAUNCH_PTS (0: the planner's cut)
    uint64_t parts = 0;       // MDP_CHAIN_PARTS (0: the planner's choice)
};

// "NAME=VALUE" pairs in the grammar of the other _opts calls; NULL or ""
// leaves the defaults.  MDP_CHAIN_NM = 8 | 16 | 32 | 64, MDP_CHAIN_LAUNCH_PTS
// and MDP_CHAIN_PARTS = decimal >= 0; anything else is MDP_EINVAL.
int chain_parse_opts(const char *s, ChainOpts *o);

struct ChainPlan {
    uint32_t n = 0, nm = 0, nmiss = 0, n1 = 0;  // n1: patches observed occupied
    int kind = 0;                // 0 die-off, 1 habitat loss
    double m = 400.0;
    double p = 0.5;              // (double)(float)p
    std::vector<double> M;       // [nm][nm] exp(-(1/m)|l-k|d), 0.0 on the diagonal and in the padding
    std::vector<double> target;  // [n+1] the default target weights
    ChainOpts opts;
};

// refusals of mdp_scenario_chain_create, then the plan
int chain_plan(const int32_t *row, uint32_t n, double m, float p, double d, int kind, const ChainOpts &opts,
               ChainPlan *plan);

// src[id][k] = exp(-(1/m)(k+1) dsrc[id]) (loss.c:250-251), k < n, 0.0 in the
// padding: [nd][nm]; all 0.0 for die-off and for a baseline table
void chain_src(const ChainPlan &plan, bool baseline, const double *dsrc, uint32_t nd, std::vector<double> *src);

// The launches of one counting call.  A work tile is (point, class, 256
// replicates): tiles_per_class = ceil(nrep / 256) per class, (n+1) times that
// per point, class-major.  A point's tiles are cut into `parts` contiguous
// runs, [T*q/parts, T*(q+1)/parts) for run q; one workgroup takes a run at a
// time (unit = point * parts + run, grid-stride), tallies it in LDS and
// flushes once.  The device table of a launch holds npts*(n+1)^2 32-bit cells.
struct ChainLaunch {
    uint64_t p0 = 0, npts = 0;
    uint64_t parts = 0;   // runs per point
    uint64_t units = 0;   // npts * parts
    uint32_t nwg = 0;     // min(units, kChainMaxWG)
};

struct ChainCall {
    uint64_t G = 0;                // points: ne*nc*nK*nd, or ne*nc of a baseline table
    uint64_t tiles_per_class = 0, tiles_per_point = 0;
    uint64_t cells = 0;            // G*(n+1)^2
    std::vector<ChainLaunch> launches;
};

// refusals of a counting call over one table (mdp_scenario_chain_counts, and
// each half of _lik, _lik_device, _time_kernels), then the cut.  host_table:
// the cells must fit a host table (<= 2^24).  K and dsrc are not looked at
// for a baseline table.
int chain_call(const ChainPlan &plan, bool baseline, const double *e, uint32_t ne, const double *c, uint32_t nc,
               const double *K, uint32_t nK, const double *dsrc, uint32_t nd, uint64_t nrep, bool host_table,
               ChainCall *call);

// refusals of the evaluation (mdp_scenario_chain_eval, _lik, _lik_device):
// durations, replicate counts, weights (NULL: the defaults)
int chain_eval_check(const ChainPlan &plan, int ts, int tdis, uint64_t nrep, uint64_t nbase, const double *start,
                     const double *target);

// start[n+1], target[n+1] as the evaluation uses them: the caller's, or the
// defaults 1/(n+1) and plan.target
void chain_weights(const ChainPlan &plan, const double *start, const double *target, std::vector<double> *w_start,
                   std::vector<double> *w_target);

// The chain evaluation on host tables: for every (ie, ic) v = B^tdis target,
// then for every point of it v = A^ts v, by_class[g][k] = v[k] (may be NULL),
// out[g] = sum_k start[k] v[k]; a = cnt_scn / nrep, b = cnt_base / nbase as
// doubles, every sum ascending from 0.0, each product rounded before its add.
int chain_eval(const ChainPlan &plan, int ts, int tdis, uint32_t ne, uint32_t nc, uint32_t nK, uint32_t nd,
               const uint64_t *cnt_scn, uint64_t nrep, const uint64_t *cnt_base, uint64_t nbase, const double *start,
               const double *target, double *out, double *by_class);

#endif
