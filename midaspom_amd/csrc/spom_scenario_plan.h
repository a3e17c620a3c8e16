// midaspom_amd/csrc/spom_scenario_plan.h -- host planning of the exact
// scenario engine (spom_scenario.hip: k_scn<NL,NH>, k_scn_row, k_scn_big):
// the options of mdp_scenario_create_opts, every refusal, the choice among
// the three kernels, the tables they read (colonisation sums S, prior vector
// w, hi factor offsets, the hi-row wave schedule, the row order), their LDS
// bytes, and per grid the source rows, the buffer sizes and the cut of both
// passes into launches.  No HIP runtime call (spom_scenario_plan.cpp links
// into scenario_plan_check.cpp as it links into libmidaspom.so).  Also the
// K and source-distance grids of the drop-ins (mdp_kgrid, mdp_dgrid).
#ifndef SPOM_SCENARIO_PLAN_H
#define SPOM_SCENARIO_PLAN_H
#include <cstddef>
#include <cstdint>
#include <vector>

#include "mdp_internal.h"

#ifdef __HIPCC__
#define SCN_HD __host__ __device__
#else
#define SCN_HD
#endif

// shared with the kernels
constexpr int kScnBlock = 1024;       // 16 waves: four per SIMD
constexpr int kE = 32;                 // e values per workgroup (lanes mod 32)
constexpr int kWaves = kScnBlock / 64;
constexpr uint32_t kMaxN = 8;          // k_scn: 2 x 2^8 x 32 state values + factor tables in LDS
constexpr uint32_t kBigMaxN = 16;      // k_scn_big: state vectors in HBM
constexpr int kBigBlock = 256;
constexpr size_t kBigScratch = 1ull << 30;  // k_scn_big state-vector scratch per launch (bytes)
constexpr int kRowBlock = 256;              // k_scn_row: one grid point per workgroup
constexpr size_t kRowPer = (size_t)1 << 22;  // k_scn_row: points per launch (grid of < 2^32 threads)
constexpr uint32_t kRowMaxN = 12;           // k_scn_row: 2 x 2^n states + 3 n x 256 per-lane values in LDS

SCN_HD constexpr int pow3(int x)
{
    int r = 1;
    for (; x > 0; --x) r *= 3;
    return r;
}
// k_scn<NL, NH> of n <= kMaxN patches: NL = min(3, n) lo patches, NH = n - NL
constexpr uint32_t scn_nl(uint32_t n) { return n < 3 ? n : 3u; }

struct ScnOpts {
    bool big = false, row = false;  // MDP_SCN_BIG, MDP_SCN_ROW: force k_scn_big / k_scn_row
    uint64_t launch_pts = 0;        // MDP_SCN_LAUNCH_PTS: cap on the points per launch of those two (0: none)
};

// "NAME=VALUE" pairs (spom_opts.h).  A flag without a value is on, its value
// is read by atoi (0 is off); the cap by atol, <= 0 is none, clipped to 2^32.
// An unknown name is MDP_EINVAL.
int scn_parse_opts(const char *s, ScnOpts *o);

enum ScnPath { kScnLds, kScnRow, kScnBig };

struct ScnPlan {
    uint32_t n = 0, ns = 0;  // patches, 2^n states
    int kind = 0;            // 0 die-off, 1 habitat loss
    double m = 400.0, d = 200.0;
    ScnPath path = kScnLds;
    char kname[16] = "";     // "k_scn<3,5>", "k_scn_row", "k_scn_big"
    std::vector<double> S;   // [ns][n] colonisation sums of state j (bit n-1-l = patch l) at patch k
    std::vector<double> w;   // [ns] prior of the observed first-row states
    std::vector<uint32_t> boff, jsched;  // k_scn: hi factor table offsets [2^NH]; hi rows [kWaves][nsched]
    uint32_t nsched = 0, btot = 0;       //   slots per wave (0xffffffff pads); doubles of the hi factor table
    std::vector<uint32_t> jord;          // k_scn_row: the states by ascending occupied count [ns]
    size_t lds = 0;                      // dynamic LDS bytes of a launch (k_scn_big: 0)
    uint64_t launch_pts = 0;
};

// refusals of mdp_scenario_create_opts that need no device, then the plan
int scn_plan(const int32_t *row, uint32_t n, double m, float p, double d, int kind, const ScnOpts &opts,
             ScnPlan *plan);

struct ScnLaunch {
    uint64_t p0 = 0, pts = 0;  // grid points [p0, p0 + pts)
    uint32_t nwg = 0;          // workgroups
};

// One grid: pass 0 stores v = P^tdis w per (c, e), pass 1 L = 1^T PK^ts v per point.
struct ScnGrid {
    int ts = 0, tdis = 0;
    uint32_t ne = 0, nc = 0, nK = 0, nd = 0;  // all 0 for an empty grid
    std::vector<double> src;                  // [nd][n] source rows (0.0 for die-off)
    size_t nV = 0, nY = 0;                    // doubles of v [nc][ns][ne]; of k_scn_big's state scratch
    uint32_t big_pts = 0;                     // k_scn_big: points per launch
    std::vector<ScnLaunch> launches[2];
};

// refusals of mdp_scenario_set_grid, then the sizes and the launches
int scn_grid_plan(const ScnPlan &plan, int ts, int tdis, const double *e, uint32_t ne, const double *c, uint32_t nc,
                  const double *K, uint32_t nK, const double *dsrc, uint32_t nd, ScnGrid *grid);

#endif
