// midaspom_amd/csrc/spom_engine.hip -- MI355X (gfx950) posterior-grid
// likelihood engine for the stochastic patch occupancy model: the device unit.
//
// Files of the engine:
//   spom_engine.h    constants, the plan types (MdpEnginePlan, MdpCTables,
//                    MdpGridPlan) and size helpers shared by the planner, the
//                    kernels and the launchers
//   spom_plan.cpp    host planning: options, the plan tables the kernels
//                    index, the hipRTC sources, per grid the c tables and the
//                    grid plan (mdp_plan_grid: kernel variant, point list,
//                    chunk widths, buffer sizes, launch shape), the work
//                    counts; no HIP runtime call, no sight of a device context
//   spom_engine.hip  (this file) the kernels, the engine (mdp_engine: the plan
//                    plus its device contexts, DevCtx, whose buffers own their
//                    memory: DevBuf, spom_dev.h), device set-up (uploads;
//                    set_grid_dev grows and uploads what the grid plan says),
//                    the launch paths, run_dev, timing and the C ABI
//   spom_jit.cpp     generator of the specialised forward kernel's source
//   spom_jit_rtc.cpp its hipRTC compilation and code-object caches
//
// Paths (mdp_plan_engine picks one per engine, MdpEnginePlan::path: Generic,
// Direct or DirectQGlobal, WideHs / WideMmt / WideMma / WidePlain; per grid
// mdp_plan_steps names what each of the three slots runs, MdpGridPlan::step,
// and launch_slot switches on it; DESIGN.md sections 3-4):
//   generic  any problem (MDP_JIT=0, or hipRTC failed): k_zpv -> k_coefs ->
//            k_forward(_lds), transitions as degree-D polynomials in e;
//            tables from build_plan.
//   direct   years of at most 16 states: k_zrows -> k_qrows -> the forward
//            kernel specialised to the problem, or its fused variant alone;
//            long series as chunks of years (plan_chunks), years of 17-64
//            states with their state vectors in LDS; tables from
//            build_direct_plan and z_split.
//   wide     larger years: k_zrows -> k_witems (+ k_wq) -> k_fwd_hs
//            (build_hs_plan), k_fwd_mmt (build_mmt_plan), k_fwd_mma or
//            k_fwd_wide (build_wide_plan); work items from plan_waves.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <set>
#include <string>
#include <vector>

#include "spom_dev.h"
#include "spom_engine.h"

// ---------------------------------------------------------------------------
// the engine: its plan, its device contexts, its run-time state
// ---------------------------------------------------------------------------
// a kernel instantiation a context has noted (note_launch): the launch
// site's format string, by address, and its arguments
struct LaunchNote {
    const char *fmt;
    uint64_t a[4];
};

// The handles of a device context, as the BASE of DevCtx, which holds the
// buffers.  The release order is by declaration: ~DevCtx's body makes the
// device current, then DevCtx's members go (the buffers), then this base: the
// events, the modules, the stream.  (DevPending: the device forms still
// pending on a caller's stream, spom_dev.h.)
struct DevHandles : DevPending {
    int device = 0;
    hipStream_t stream = nullptr;
    // problem-specialised forward kernel [variant]: 0 reading, 1 fused, 2
    // reading at kJitKblockTall threads (tall grids, mdp_plan_grid)
    hipModule_t jit_mod[3] = {nullptr, nullptr, nullptr};
    std::vector<hipModule_t> cmod;  // a long series: one forward kernel per chunk of years
    std::vector<hipEvent_t> ev;     // kNumEv events per profiled run, reused
    DevHandles() = default;
    DevHandles(const DevHandles &) = delete;
    DevHandles &operator=(const DevHandles &) = delete;
    ~DevHandles()
    {
        for (hipEvent_t x : ev) (void)hipEventDestroy(x);
        for (hipModule_t m : jit_mod)
            if (m) (void)hipModuleUnload(m);
        for (hipModule_t m : cmod) (void)hipModuleUnload(m);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// One device of an engine.  Neither copied nor moved (mdp_engine::devs is
// built at its final size): the base's handles are released exactly once.
struct DevCtx : DevHandles {
    mutable std::vector<LaunchNote> noted;  // what this context has reported to mdp_engine::launched
    DevBuf<double> S;
    DevBuf<uint32_t> var_cols, row_col, pairA, pairB, pairOff, udesc, prog, pairPart0, partP, partK0;
    DevBuf<double> e, c;
    uint32_t ne = 0, nc = 0;
    MdpCTables ct;     // the c tables on the device (host copy and the bound they hold for)
    MdpGridPlan plan;  // the current grid's plan (set_grid_dev)
    // the plan's point list and its e values by position: a listed kernel
    // loads its e values by position, beside the list, instead of through it
    // (position -> row -> e would be two round trips in series)
    DevBuf<uint32_t> plist;
    DevBuf<double> elist, ZPV, R, out, gpart;
    DevBuf<unsigned long long> stamps[3];  // k_zpv, k_coefs, k_forward
    // direct path: k_zrows / k_qrows tables (zs, row-major [row][k], depends
    // on the grid's c range)
    DevBuf<double> zs, sv, Qrow, Zg;
    DevBuf<double> zsq;  // zs chain-major, [row][k mod 4][k / 4] (k_qrows: a lane's chain contiguous)
    DevBuf<double> zc;   // Z-row series coefficients [row][kZTerms]
    DevBuf<uint2> items;  // per item {B | row << 24, j | (row >> 8) << 24}
    DevBuf<uint2> qslot;  // k_qrows phase-3 lane table
    DevBuf<uint32_t> qlane;  // k_qrows phase-3 Pc slots per lane (nvar <= 8)
    DevBuf<uint32_t> islot;  // k_qrows: each item's Pc slot
    DevBuf<uint32_t> qstart, qitem;
    DevBuf<double> coltab;  // fused kernel's column tables (MdpCTables::coltab)
    bool qrows_attr_set = false;  // k_qrows' LDS limit raised on this device
    hipFunction_t jit_fn[3] = {nullptr, nullptr, nullptr};  // of jit_mod
    // the chunks of a long series (cmod): the state vector handed over in
    // vscr[state][c][e] (ldv e values per (state, c))
    std::vector<hipFunction_t> cfn;
    std::vector<DevBuf<uint32_t>> cqidx;  // per chunk: gather indices into the Q row (empty: whole row)
    DevBuf<double> vscr;
    uint32_t ncu = 0;    // the device's compute units (0: not asked yet)
    // wide path: per-chunk item factors, state-vector scratch, tables
    DevBuf<double> Pg, V;
    DevBuf<uint32_t> np_d, udesc_w;
    DevBuf<uint2> mma_kt, mma_wplan;
    DevBuf<uint32_t> mma_kbase, mma_desc, mma_dbase;
    DevBuf<uint2> mmt_kt, mmt_ktile, mmt_wplan;  // k_fwd_mmt tables
    DevBuf<uint32_t> mmt_cidx;
    DevBuf<uint32_t> hs_kt, hs_cidx, hs_pbase, hs_dpos, hs_dbase, hs_pk;
    DevBuf<uint2> hs_ppos, hs_dpk;
    DevBuf<uint4> hs_wplan, hs_pass;  // (hs_*: k_fwd_hs tables)
    std::vector<uint8_t> ev_mask;  // per profiled run: slots whose kernel was launched
    size_t ev_used = 0;          // event sets recorded since the last collect
    ~DevCtx()
    {
        (void)hipSetDevice(device);
        (void)settle();
    }
};

struct mdp_engine : MdpEnginePlan {
    std::vector<DevCtx> devs;
    int layout = MDP_LAYOUT_EC;  // mdp_engine_run's output layout (mdp_engine_set_layout)
    mutable std::set<std::string, std::less<>> launched;  // kernel instantiations launched so far (mdp_engine_launched)
    mutable std::mutex launched_mu;                         // engines may be driven from several host threads
    int profiling = 0;
    double last_ms[3] = {0, 0, 0};  // mean per run over the last collected runs
    int nlast = 0;
    uint64_t runs_collected = 0;
};

namespace {

constexpr int kZpvSlices = 4;   // k_zpv: waves splitting the zero-column product
constexpr int kZpvUnroll = 8;   // k_zpv: S loads in flight per lane
constexpr unsigned kWaitLgkm0 = 0xC07F;  // s_waitcnt lgkmcnt(0), other counters untouched
#ifdef MDP_DIAG_BUILD
constexpr bool kDiagBuild = true;  // the measurement-only options are accepted (parse_engine_opts)
#else
constexpr bool kDiagBuild = false;
#endif

__constant__ double c_binom[kMaxDeg + 1][kMaxDeg + 1];

// Diagnostic phase stamps (MDP_DIAG=1): wave 0 of every workgroup records
// s_memtime at phase boundaries into stamps[block][slot]; a null pointer (the
// default) skips them with one scalar branch.
#define MDP_STAMP(stamps, slot)                                                           \
    do {                                                                                  \
        if ((stamps) && threadIdx.x == 0)                                                 \
            (stamps)[(size_t)(blockIdx.x + gridDim.x * blockIdx.y) * kStampSlots + (slot)] = \
                __builtin_amdgcn_s_memtime();                                             \
    } while (0)
// wall-clock stamps (s_memrealtime, 100 MHz, chip-wide) in the last two slots
#define MDP_RSTAMP(stamps, slot)                                                          \
    do {                                                                                  \
        if ((stamps) && threadIdx.x == 0)                                                 \
            (stamps)[(size_t)(blockIdx.x + gridDim.x * blockIdx.y) * kStampSlots + (slot)] = \
                __builtin_amdgcn_s_memrealtime();                                         \
    } while (0)

// Kernel timing: while an engine is profiled, every launch of a run carries
// its own start/stop events (hipExtLaunchKernel), which the runtime stamps
// from the dispatch itself -- no marker packets between the kernels, so the
// timed run is the production run and the durations agree with rocprofv3.
struct KernelEvents {
    hipEvent_t start = nullptr, stop = nullptr;
};
thread_local KernelEvents t_kev;

#define MDP_LAUNCH(kernel, grid, block, shmem, stream, ...)                                     \
    hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)(shmem), stream, t_kev.start, t_kev.stop, \
                          0u, __VA_ARGS__)

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------

// The generic path replaces the reference's hot loop, main_MIDASPOM.c:341-395
// (colonisation pressure :350-358, compPePc :18-50, P = Pe*Pc dgemm :363,
// forward propagation :368-384, prior sum + log :386-392).
//
// Factorisation.  For observed short states a -> b with bit
// sets A, B and hidden intermediate state j (extinction first, then
// colonisation) the reference forms P[a][b] = sum_j Pe[a][j] Pc[j][b] with
//   Pe[a][j] = [j <= A] x^{|A|-|j|} y^{|j|}        (x = min(e,1), y = 1-x)
//   Pc[j][b] = [j <= B] prod_{k : j_k = 0} (B_k ? pC_jk : 1-pC_jk),
//   pC_jk    = min(1, c * S[j][k]),   S = grid-invariant dispersal sums.
// Pe depends on e only through |j| and Pc on c only, so
//   P[a][b](e,c) = sum_{m=0}^{|A&B|} x^{|A|-m} y^m Q_ab[m](c),
//   Q_ab[m](c)   = sum_{j <= A&B, |j| = m} Pc[j][b](c).
// Multiplying by (x+y)^{D-|A|} = 1 makes every transition a homogeneous
// polynomial of ONE degree D (>= every |A|) with non-negative coefficients
//   P[a][b](e,c) = sum_{r=0}^{D} R_ab[r](c) W_r(e),  W_r = x^{D-r} y^r,
//   R_ab[r]      = sum_m Q_ab[m] C(D-|A|, r-m),
// so a transition costs D+1 FMAs against per-point weights held in VGPRs and
// per-c coefficients that are wave-uniform (scalar loads, no descriptors).
//
// Kernels (per run over an ne x nc grid):
//   k_zpv      [c][j]     Z = prod_{always-zero k} (1-pC_jk), PV_b = pC_j,var(b)
//   k_coefs    one WG / c Q (subset sums, LDS) -> R in forward-use order
//   k_forward  one lane / (e,c) point x EPL: forward recursion over the years,
//              c wave-uniform, R streamed through the scalar cache.
// Once per engine: k_colsum builds S.

// S2[r][j] = S[col(r)][j]: the colonisation sum of column k = col(r) for
// hidden state j, i.e. the sum over set bits of j (ascending variable column
// l, l != k) of M[l][k] -- the reference's per-point sum (:350-357) with its
// zero terms dropped, bit-identical.  Rows are ordered always-zero columns
// first, then variable columns, so k_zpv reads them without indirection.
__global__ __launch_bounds__(kBlock) void k_colsum(const double *__restrict__ M,
                                                   const uint32_t *__restrict__ var_cols,
                                                   const uint32_t *__restrict__ row_col,
                                                   uint32_t n, uint32_t nvar, uint32_t nstates,
                                                   double *__restrict__ S2)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t r = blockIdx.y;
    if (j >= nstates) return;
    const uint32_t k = row_col[r];
    double acc = 0.0;
    for (uint32_t b = 0; b < nvar; ++b) {
        const uint32_t col = var_cols[b];
        if (((j >> (nvar - 1 - b)) & 1u) && col != k) acc += M[(size_t)col * n + k];
    }
    S2[(size_t)r * nstates + j] = acc;
}

// ZPV[c][0][j] = prod over always-zero columns (ascending) of (1 - pC_jk);
// ZPV[c][1+b][j] = pC_j,var(b) = min(1, c S).  A workgroup covers 64 hidden
// states x kZpvCT c values; its 4 waves each take a quarter of the zero
// columns (kZpvUnroll loads in flight per lane) and the partial products are
// multiplied in slice order through LDS.
__global__ __launch_bounds__(kBlock) void k_zpv(
    const double *__restrict__ S2, uint32_t nstates, uint32_t nnv, uint32_t nvar,
    const double *__restrict__ cvals, uint32_t nc, double *__restrict__ ZPV,
    unsigned long long *__restrict__ stamps)
{
    __shared__ double part[kZpvSlices][kZpvCT][kZpvJ];
    MDP_RSTAMP(stamps, 6);
    MDP_STAMP(stamps, 0);
    const uint32_t lane = threadIdx.x % kZpvJ, slice = threadIdx.x / kZpvJ;
    const uint32_t j = blockIdx.x * kZpvJ + lane;
    const uint32_t c0 = blockIdx.y * kZpvCT;
    const bool ok = j < nstates;
    const uint32_t jj = ok ? j : 0;
    double c[kZpvCT], z[kZpvCT];
#pragma unroll
    for (int t = 0; t < kZpvCT; ++t) {
        c[t] = (c0 + t < nc) ? cvals[c0 + t] : 0.0;
        z[t] = 1.0;
    }
    const uint32_t per = (nnv + kZpvSlices - 1) / kZpvSlices;
    const uint32_t q0 = slice * per, q1 = min(nnv, q0 + per);
    uint32_t q = q0;
    for (; q + kZpvUnroll <= q1; q += kZpvUnroll) {
        double sv[kZpvUnroll];
#pragma unroll
        for (int u = 0; u < kZpvUnroll; ++u) sv[u] = S2[(size_t)(q + u) * nstates + jj];
#pragma unroll
        for (int t = 0; t < kZpvCT; ++t) {
            // 1 - min(1, c s), evaluated as max(0, 1 - c s) with one rounding;
            // the batch is multiplied as a tree so only one multiply per
            // batch sits on the dependency chain
            double f[kZpvUnroll];
#pragma unroll
            for (int u = 0; u < kZpvUnroll; ++u) f[u] = fmax(0.0, fma(-c[t], sv[u], 1.0));
#pragma unroll
            for (int w = 1; w < kZpvUnroll; w *= 2)
#pragma unroll
                for (int u = 0; u + w < kZpvUnroll; u += 2 * w) f[u] *= f[u + w];
            z[t] *= f[0];
        }
    }
    for (; q < q1; ++q) {
        const double s0 = S2[(size_t)q * nstates + jj];
#pragma unroll
        for (int t = 0; t < kZpvCT; ++t) z[t] *= fmax(0.0, fma(-c[t], s0, 1.0));
    }
#pragma unroll
    for (int t = 0; t < kZpvCT; ++t) part[slice][t][lane] = z[t];
    MDP_STAMP(stamps, 1);
    __syncthreads();
    const size_t rows = (size_t)nvar + 1;
    if (slice == 0 && ok) {
#pragma unroll
        for (int t = 0; t < kZpvCT; ++t) {
            double zz = part[0][t][lane];
#pragma unroll
            for (int sl = 1; sl < kZpvSlices; ++sl) zz *= part[sl][t][lane];
            if (c0 + t < nc) ZPV[(size_t)(c0 + t) * rows * nstates + j] = zz;
        }
    }
    if (ok)
        for (uint32_t b = slice; b < nvar; b += kZpvSlices) {
            const double sb = S2[(size_t)(nnv + b) * nstates + j];
#pragma unroll
            for (int t = 0; t < kZpvCT; ++t)
                if (c0 + t < nc) {
                    const double pc = c[t] * sb;
                    ZPV[((size_t)(c0 + t) * rows + 1 + b) * nstates + j] = pc > 1.0 ? 1.0 : pc;
                }
        }
    MDP_STAMP(stamps, 2);
    MDP_RSTAMP(stamps, 7);
}

// Z rows of the direct path: Zg[row][c] = prod over the always-zero columns k
// of 1 - min(1, c S[j][k]) for every needed hidden state j ("row").  Lanes run
// over c values and each wave over one row, so the S values are LDS
// broadcasts (the workgroup's rows staged once from zs[k][row]).  A broadcast
// read still returns 8 bytes per lane, so with one c per lane the kernel was
// bound by LDS return bandwidth rather than by its FMAs: each lane now
// carries kZC c values that share every read.  Same multiplication order as
// the fused forward kernel (four chains over k mod 8), so both variants give
// identical bits.
// Product of a Z row's small-column factors: exp(-c (P1 + c (P2/2 + ... +
// c P8/8))), Horner from the top (z_split's coefficients; the fused kernel
// evaluates the same expression)
__device__ __forceinline__ double zseries(const double (&p)[kZTermsDev], double c)
{
    double q = p[kZTermsDev - 1];
#pragma unroll
    for (int i = kZTermsDev - 2; i >= 0; --i) q = fma(q, c, p[i]);
    return exp(-(q * c));
}

constexpr uint32_t kZStage = 4;           // staging loads in flight per thread
constexpr uint32_t kZC = 2;               // c values per lane
__global__ __launch_bounds__(kBlock) void k_zrows(const double *__restrict__ cvals, uint32_t nc,
                                                  uint32_t nrows, uint32_t kmax,
                                                  const double *__restrict__ zsT, const double *__restrict__ zc,
                                                  double *__restrict__ Zg)
{
    extern __shared__ __attribute__((aligned(16))) double zl[];  // [kZRows][kmax]
    const uint32_t r0 = blockIdx.y * kZRows, nr = min(kZRows, nrows - r0);
    // the workgroup's rows are contiguous in the row-major copy zsT[row][k]:
    // coalesced loads, kZStage in flight per thread before any store
    const uint32_t nst = nr * kmax;
    for (uint32_t i0 = threadIdx.x; i0 < kZRows * kmax; i0 += kZStage * kBlock) {
        double t[kZStage];
#pragma unroll
        for (uint32_t u = 0; u < kZStage; ++u) {
            const uint32_t i = i0 + u * kBlock;
            t[u] = i < nst ? zsT[(size_t)r0 * kmax + i] : 0.0;
        }
#pragma unroll
        for (uint32_t u = 0; u < kZStage; ++u)
            if (i0 + u * kBlock < kZRows * kmax) zl[i0 + u * kBlock] = t[u];
    }
    __syncthreads();
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
    if (w >= nr) return;
    // the row's small columns: exp(-c (P1 + c (P2/2 + ...))) (z_split's coefficients)
    double zcoef[kZTermsDev];
#pragma unroll
    for (int i = 0; i < kZTermsDev; ++i) zcoef[i] = zc[(size_t)(r0 + w) * kZTermsDev + i];
    uint32_t ic[kZC];
    double c[kZC], za[kZC], zb[kZC], zc_[kZC], zd[kZC];
#pragma unroll
    for (uint32_t x = 0; x < kZC; ++x) {
        ic[x] = blockIdx.x * (64 * kZC) + x * 64 + (threadIdx.x & 63);
        c[x] = ic[x] < nc ? cvals[ic[x]] : 0.0;
        za[x] = zb[x] = zc_[x] = zd[x] = 1.0;
    }
    const double *z = zl + w * kmax;
    auto chunk = [&](const double *sk) {
#pragma unroll
        for (uint32_t x = 0; x < kZC; ++x) {
            za[x] *= fma(-c[x], sk[0], 1.0) * fma(-c[x], sk[4], 1.0);
            zb[x] *= fma(-c[x], sk[1], 1.0) * fma(-c[x], sk[5], 1.0);
            zc_[x] *= fma(-c[x], sk[2], 1.0) * fma(-c[x], sk[6], 1.0);
            zd[x] *= fma(-c[x], sk[3], 1.0) * fma(-c[x], sk[7], 1.0);
        }
    };
    uint32_t k = 0;
    for (; k + 16 <= kmax; k += 16) {  // two chunks' reads in flight
        double sk[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) sk[u] = z[k + u];
        chunk(sk);
        chunk(sk + 8);
    }
    if (k < kmax) {  // kmax is a multiple of 8
        double sk[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) sk[u] = z[k + u];
        chunk(sk);
    }
#pragma unroll
    for (uint32_t x = 0; x < kZC; ++x) {
        double zz = (za[x] * zb[x]) * (zc_[x] * zd[x]);
        if (kmax && !(fma(-c[x], z[0], 1.0) > 0.0)) zz = 0.0;
        zz *= zseries(zcoef, c[x]);
        if (ic[x] < nc) Zg[(size_t)(r0 + w) * nc + ic[x]] = zz;
    }
}

// Transition coefficients of the direct path, one workgroup per CB (1, 2 or
// 4) consecutive c values, every hidden state j some transition needs
// ("rows", r) and every (j, b) item.  Per-c values sit interleaved in LDS in
// planes of two ([CB/2][r][2], [CB/2][item][2]) so the CB values of one row or
// item are one or two 16-byte accesses and lanes over rows / items touch
// consecutive 16-byte slots:
//  1. threads over (r, c): Z_r(c) = the row's explicit columns (zsT[row][k],
//     16 loads in flight) in k_zrows' four chains and order, the clamp test
//     against the row maximum (stored first), the small columns' series;
//  2. threads over items, all CB c values each: Pc[j][b] = Z_r prod_{var b'
//     not in j} (B_b' ? pC : 1 - pC), pC = min(1, c S[j][b']) from the row's
//     staged var-column S (-1 marks the columns of j: pC = 1.0 there);
//  3. threads over Q entries, all CB c values each: the entry's items summed
//     in CSR (ascending j) order -- written as coalesced rows for the forward
//     kernel.
// Nothing but Q leaves the workgroup.  (Round 1 kept the pressures in a
// [c][row][NV] array whose 64-byte row stride put a wave's reads on a quarter
// of the LDS banks, and ran threads over (c, item): SQ_LDS_BANK_CONFLICT was
// 3x SQ_ACTIVE_INST_LDS.)
// Canonical Q-entry sum -- k_qrows, k_wq and the fused forward kernel
// (spom_jit.cpp) all use it, so their Q rows agree bit for bit: the entry's
// items in CSR order taken in groups of kQGroup, each group summed left to
// right, and the group sums added as a pairwise tree padded with zeros to a
// power of two.  Folding the group sums into a binary counter (level l
// holds the sum of an aligned block of 2^l groups) and then folding the
// occupied levels from the lowest up gives exactly that tree; so does a
// butterfly of xor shuffles over an aligned power-of-two lane segment
// holding the sums of aligned power-of-two blocks of groups (k_qrows).
// A double from the lane DPP control CTRL names (quad_perm 0x00-0xff,
// row_mirror 0x140, row_half_mirror 0x141): no LDS, no wait
template <int CTRL>
__device__ __forceinline__ double quad_dpp(double v)
{
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

constexpr int kQLevels = 24;

constexpr int kQrowsBlock = 1024;
template <int NV, bool EXACT, int CB>  // EXACT: nvar == NV (no padded factor slots)
__global__ __launch_bounds__(kQrowsBlock) void k_qrows(
    const double *__restrict__ cvals, uint32_t nc, uint32_t nvar, uint32_t nrows,
    uint32_t kmax, const double *__restrict__ zsq, const double *__restrict__ zc, const double *__restrict__ sv,
    uint32_t nitems, const uint2 *__restrict__ items, uint32_t ncoef, const uint32_t *__restrict__ qstart,
    uint32_t nqi, const uint32_t *__restrict__ qitem, double *__restrict__ Q, uint32_t ldQ,
    unsigned long long *__restrict__ stamps, uint32_t xcd, const uint2 *__restrict__ qslot, uint32_t nslot,
    uint32_t lglmax, const uint4 *__restrict__ qlane, const uint32_t *__restrict__ islot, uint32_t npl)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    MDP_RSTAMP(stamps, 6);
    MDP_STAMP(stamps, 0);
    // phase 3's lane table does not depend on c: its first pass is loaded
    // now, its latency hidden under phases 0-2
    const uint2 sd0 = threadIdx.x < nslot ? qslot[threadIdx.x] : make_uint2(0xffffffffu, 0u);
    // nvar <= 8: the lane's group of item indices too (qlane, at least 64
    // lanes: the clamped index is in bounds)
    uint4 qa0 = make_uint4(0u, 0u, 0u, 0u), qb0 = qa0;
    if constexpr (NV == 8) {
        const uint32_t l = min(threadIdx.x, max(nslot, 1u) - 1);
        qa0 = qlane[2 * l];
        qb0 = qlane[2 * l + 1];
    }
    // XCD-aware: workgroups are dealt round-robin over the 8 XCDs, so XCD x
    // takes a contiguous eighth of the c range -- the columns the forward
    // kernel's XCD-aware order gives XCD x -- and the forward reads these Q
    // rows from its own L2
    const uint32_t nb = gridDim.x, full = nb & ~7u;
    const uint32_t lb = xcd && blockIdx.x < full ? (blockIdx.x & 7u) * (full >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    const uint32_t c0 = lb * CB, ncb = min((uint32_t)CB, nc - c0);
    // per-c values in planes of two c values ([CB/2][n][2] for CB = 4): a
    // lane's 16-byte access then sits 16 bytes after its neighbour's, not 32,
    // so consecutive items / rows fill all 64 banks (no 2-way conflicts)
    constexpr uint32_t CP = CB < 2 ? CB : 2;
    auto pix = [](uint32_t n, uint32_t x, uint32_t i) -> size_t {
        return (size_t)(i / CP) * CP * n + (size_t)x * CP + i % CP;
    };
    double *Zl = lds;                                  // [CB/CP][nrows][CP]
    // per row, c and var column the pressure min(1, c S[j][b]): rows padded
    // by one double2 so rows read by one wave fall on different banks
    constexpr uint32_t PRS = CB * NV + 2;
    double *Prl = Zl + (((size_t)nrows * CB + 1) & ~(size_t)1);  // [nrows][PRS], 16-byte aligned
    // Pc per item and c in npl slots (host table islot: item -> slot);
    // slots 0-15 hold zeros, the padding phase 3's unconditional gathers
    // read past an entry's end (one per residue mod 16, so each gather group
    // can take one no other lane of it reads)
    double *Pl = Prl + (size_t)nrows * PRS;            // [CB/CP][npl][CP]
    uint32_t *Qs = (uint32_t *)(Pl + (size_t)npl * CB);  // [ncoef + 1] (nvar > 8)
    uint32_t *Qi = Qs + ncoef + 1;                     // [nqi]
    double cv[CB];  // this workgroup's c values (the last one again past the grid: never stored)
#pragma unroll
    for (int i = 0; i < CB; ++i) cv[i] = cvals[c0 + min((uint32_t)i, ncb - 1)];  // no load in a branch
    // phase 1's c value of this lane (lane q of a quad: c value q)
    const double cq = cvals[c0 + min(threadIdx.x & 3u, ncb - 1)];
    // 1. Z and pressures per row, one quad of lanes per row.  Lane q takes
    // the row's product chain q (explicit columns k = q mod 4, k_zrows' chains
    // and order) for all CB c values; the quad combines the chains as
    // (za zb)(zc zd) (exact products commute, so every lane holds the same
    // bits); lane q then finishes c value q (the clamp test against the row
    // maximum, stored first; the small columns' series) and forms var columns
    // [q NV/4, (q + 1) NV/4) of the pressures min(1, c S) of every c value
    // (the columns of j, where sv holds -1, and padded slots select a factor
    // of exactly 1.0 in phase 2 whatever is stored here).  Each row's tables
    // cross the vector cache once per workgroup: threads over (row, c) read
    // them CB times, 4x the bytes on config 3, and the cache's return rate
    // bounded the phase.
    const uint32_t kq = kmax / 4;  // chain length (kmax a multiple of 8)
    constexpr uint32_t NB = NV / 4;  // var columns per lane
    constexpr uint32_t kPre = 3;     // chain pairs loaded up front (kmax <= 24: all)
    struct RowLd {
        double2 t[kPre];  // the chain's first pairs
        double2 zq2;      // the lane's two series coefficients
        double sb[NB];    // the lane's var columns of S
    };
    auto rowload = [&](uint32_t w, RowLd &L) {
        const uint32_t q = w & 3u, r = w >> 2;
        const double2 *zr = (const double2 *)(zsq + (size_t)r * kmax + (size_t)q * kq);
#pragma unroll
        for (uint32_t u = 0; u < kPre; ++u) L.t[u] = zr[2 * u < kq ? u : 0];  // zsq padded: in bounds at kmax 0
        L.zq2 = ((const double2 *)(zc + (size_t)r * kZTermsDev))[q];
#pragma unroll
        for (uint32_t i = 0; i < NB; ++i) {
            const uint32_t b = q * NB + i;
            const double x = sv[(size_t)r * nvar + (EXACT ? b : min(b, nvar - 1))];
            L.sb[i] = (EXACT || b < nvar) ? x : HUGE_VAL;  // padded slot: pressure 1.0
        }
    };
    auto rowwork = [&](uint32_t w, const RowLd &L) {
        const uint32_t q = w & 3u, r = w >> 2;
        const double2 *zr = (const double2 *)(zsq + (size_t)r * kmax + (size_t)q * kq);
        double ch[CB];
#pragma unroll
        for (int i = 0; i < CB; ++i) ch[i] = 1.0;
        auto pair = [&](const double2 p) {
#pragma unroll
            for (int i = 0; i < CB; ++i) ch[i] *= fma(-cv[i], p.x, 1.0) * fma(-cv[i], p.y, 1.0);
        };
#pragma unroll
        for (uint32_t u = 0; u < kPre; ++u)
            if (2 * u < kq) pair(L.t[u]);
        for (uint32_t u = kPre; 2 * u < kq; u += 2) {  // longer rows (|c| > 1)
            const double2 x = zr[u], y = 2 * u + 2 < kq ? zr[u + 1] : make_double2(0.0, 0.0);
            pair(x);
            if (2 * u + 2 < kq) pair(y);
        }
        // (za zb)(zc zd) for c value q in lane q
        double c = cv[0], zz;
        if constexpr (CB == 4) {
            // reduce-scatter: the pairs (0,1), (2,3) each keep two c values
            // (lane q those = q mod 2), then (0,2), (1,3) one
            const bool b0 = q & 1u, b1 = q & 2u;
            const double s0 = b0 ? ch[0] : ch[1], s1 = b0 ? ch[2] : ch[3];
            const double k0 = (b0 ? ch[1] : ch[0]) * quad_dpp<0xB1>(s0);  // quad_perm [1,0,3,2]
            const double k1 = (b0 ? ch[3] : ch[2]) * quad_dpp<0xB1>(s1);
            zz = (b1 ? k1 : k0) * quad_dpp<0x4E>(b1 ? k0 : k1);  // quad_perm [2,3,0,1]
            c = cq;
        } else {
#pragma unroll
            for (int i = 0; i < CB; ++i) {
                ch[i] = ch[i] * quad_dpp<0xB1>(ch[i]);  // quad_perm [1,0,3,2]
                ch[i] = ch[i] * quad_dpp<0x4E>(ch[i]);  // quad_perm [2,3,0,1]
            }
            zz = ch[0];
#pragma unroll
            for (int i = 1; i < CB; ++i)
                if (q == (uint32_t)i) c = cv[i], zz = ch[i];
        }
        const double first = quad_dpp<0x00>(L.t[0].x);  // column 0, the row maximum
        if (kmax && !(fma(-c, first, 1.0) > 0.0)) zz = 0.0;
        double zq[kZTermsDev];
        zq[0] = quad_dpp<0x00>(L.zq2.x), zq[1] = quad_dpp<0x00>(L.zq2.y);
        zq[2] = quad_dpp<0x55>(L.zq2.x), zq[3] = quad_dpp<0x55>(L.zq2.y);
        zq[4] = quad_dpp<0xAA>(L.zq2.x), zq[5] = quad_dpp<0xAA>(L.zq2.y);
        zq[6] = quad_dpp<0xFF>(L.zq2.x), zq[7] = quad_dpp<0xFF>(L.zq2.y);
        zz *= zseries(zq, c);
        if (q < (uint32_t)CB) Zl[pix(nrows, r, q)] = zz;
        // min(1, c S) as the reference clamps it (:355-357): NaN stays NaN;
        // exactly 1.0 for the columns of j (sv -1) and the padded slots, so
        // that phase 2's fma(s, p, n) gives their factor 1.0 with no select
#pragma unroll
        for (int i = 0; i < CB; ++i) {
            double pr[NB];
#pragma unroll
            for (uint32_t j = 0; j < NB; ++j) {
                pr[j] = fmin(cv[i] * L.sb[j], 1.0);  // (+inf marks: 1.0, at c = 0 too -- minNum drops NaN)
            }
            double2 *pd = (double2 *)(Prl + (size_t)r * PRS + i * NV + q * NB);
#pragma unroll
            for (uint32_t j = 0; j < NB / 2; ++j) pd[j] = make_double2(pr[2 * j], pr[2 * j + 1]);
        }
    };
    // the first row's loads (index clamped: no load in a branch), then the
    // first pass of the items and Q CSR staging, both in flight at once; the
    // staging's stores wait until the row's work is done, so its latency
    // hides under phase 1
    const uint32_t nrw = nrows * 4;
    RowLd L0;
    rowload(min(threadIdx.x, nrw - 1), L0);
    constexpr uint32_t kSt = 4;
    uint2 ti[kSt];     // the items of this thread's first kSt phase-2 passes
    uint32_t si[kSt];  // and their Pc slots
    uint32_t ts[kSt], tq[kSt];
    auto stload = [&](uint32_t i0, uint2 *pi, uint32_t *ps, uint32_t *pq) {
#pragma unroll
        for (uint32_t u = 0; u < kSt; ++u) {
            const uint32_t i = i0 + u * kQrowsBlock;
            // clamped, not guarded: a guarded load sits in a branch, and the
            // row's first use then waited for every staging load too
            if (pi) {  // launched only with items
                pi[u] = items[min(i, nitems - 1)];
                si[u] = islot[min(i, nitems - 1)];
            }
            if constexpr (NV != 8) {  // nvar <= 8: phase 3 reads qlane instead
                ps[u] = qstart[min(i, ncoef)];
                pq[u] = nqi ? qitem[min(i, nqi - 1)] : 0u;
            }
        }
    };
    auto ststore = [&](uint32_t i0, const uint32_t *ps, const uint32_t *pq) {
        if constexpr (NV != 8) {
#pragma unroll
            for (uint32_t u = 0; u < kSt; ++u) {
                const uint32_t i = i0 + u * kQrowsBlock;
                if (i <= ncoef) Qs[i] = ps[u];
                if (i < nqi) Qi[i] = pq[u];
            }
        }
    };
    stload(threadIdx.x, ti, ts, tq);
    if (threadIdx.x < nrw) rowwork(threadIdx.x, L0);
    for (uint32_t w = threadIdx.x + kQrowsBlock; w < nrw; w += kQrowsBlock) {
        RowLd L;
        rowload(w, L);
        rowwork(w, L);
    }
    MDP_STAMP(stamps, 4);
    ststore(threadIdx.x, ts, tq);
    if constexpr (NV != 8) {  // a longer Q CSR (items past kSt passes are read in phase 2)
        for (uint32_t i0 = threadIdx.x + kSt * kQrowsBlock; i0 < max(ncoef + 1, nqi); i0 += kSt * kQrowsBlock) {
            uint32_t ps[kSt], pq[kSt];
            stload(i0, nullptr, ps, pq);
            ststore(i0, ps, pq);
        }
    }
    MDP_STAMP(stamps, 5);
    __syncthreads();
    MDP_STAMP(stamps, 1);
    // 2. Pc per item, its CB c values: Z times the product F of the
    // var-column factors f_b = B_b ? pC_b : 1 - pC_b (j <= B, so j's columns
    // give pC = 1.0, a factor of exactly 1.0), in the pairwise tree over NV
    // slots -- the fused kernel's tree over nvar (padded slots are 1.0).  A
    // factor is |n_b - pC_b| with n_b = 1.0 where B_b is clear, 0.0 where set:
    // the same bits as the fused kernel's fma(s_b, pC_b, n_b), s_b = -1 / +1
    // (1 - p rounded once; |0 - p| = p exactly), with the bit converted once
    // per item and the abs folded into the tree's first products.  (Building
    // s_b and n_b as doubles cost 5 integer instructions a slot, a quarter-rate
    // multiply among them: phase 2 is bound by VALU issue.)
    // the first kSt passes' items are still in this thread's staging
    // registers (pass u's item is the one it loaded as ti[u])
    auto pcitem = [&](uint32_t sl, const uint2 t) {
        const uint32_t r = (t.x >> 24) | ((t.y >> 24) << 8), nB = ~t.x;
        double nb[NV];
#pragma unroll
        for (int b = 0; b < NV; ++b) {
            const uint32_t bit = EXACT ? (uint32_t)(NV - 1 - b) : nvar - 1 - (uint32_t)b;  // wraps past nvar
            const uint32_t nbit = !EXACT && (uint32_t)b >= nvar ? 0u : (nB >> bit) & 1u;
            nb[b] = (double)nbit;
        }
        double zr[CB], pc[CB];
#pragma unroll
        for (int i = 0; i < CB; ++i) zr[i] = Zl[pix(nrows, r, i)];
#pragma unroll
        for (int i = 0; i < CB; ++i) {
            double f[NV];
            const double2 *ps = (const double2 *)(Prl + (size_t)r * PRS + i * NV);
#pragma unroll
            for (int b = 0; b < NV / 2; ++b) {
                const double2 p2 = ps[b];
                f[2 * b] = fabs(nb[2 * b] - p2.x) * fabs(nb[2 * b + 1] - p2.y);
            }
#pragma unroll
            for (int sh = 2; sh < NV; sh *= 2)
#pragma unroll
                for (int b = 0; b + sh < NV; b += 2 * sh) f[b] *= f[b + sh];
            pc[i] = zr[i] * f[0];
        }
#pragma unroll
        for (int i = 0; i < CB; ++i) Pl[pix(npl, sl, i)] = pc[i];
    };
#pragma unroll
    for (uint32_t u = 0; u < kSt; ++u)
        if (threadIdx.x + u * kQrowsBlock < nitems) pcitem(si[u], ti[u]);
    for (uint32_t it = threadIdx.x + kSt * kQrowsBlock; it < nitems; it += kQrowsBlock) pcitem(islot[it], items[it]);
    if (threadIdx.x < 16 * CB) Pl[pix(npl, threadIdx.x / CB, threadIdx.x % CB)] = 0.0;
    __syncthreads();
    MDP_STAMP(stamps, 2);
    // 3. Q rows in the canonical order.  Each entry owns an aligned
    // power-of-two segment of L <= kQLanesMax lanes of one wave (host table
    // qslot: {entry, lane in entry | log2 L << 8 | log2 G << 12}, nslot a
    // multiple of 64); a lane sums its 2^G consecutive groups for the CB c
    // values (binary counter), then the segment adds the lanes' sums by a
    // butterfly of xor shuffles, and its first lane stores the entry.  The
    // chain per lane is a few gathers and log2 L shuffles instead of the
    // entry's whole item list (35 on config 3).
    if constexpr (NV == 8) {
        // nvar <= 8: one group per lane (an entry has at most C(8,4) = 70
        // items, 9 groups), its items' Pc slots in registers since the kernel
        // began (qlane: the group padded with a zero slot, x + 0.0 = x for
        // these non-negative, NaN or infinite values), so the gathers follow
        // the barrier directly; the slots are coloured on the host so that
        // each gather group's 16-byte slots fall on distinct banks.  The butterfly runs on DPP: after
        // level l every lane of an aligned 2^(l+1) block holds the same bits
        // (the sums commute exactly), so any lane of the partner block will
        // do -- quad_perm for levels 0-1, row_half_mirror and row_mirror for
        // levels 2-3, an xor shuffle beyond.
        for (uint32_t s0 = 0; s0 < nslot; s0 += kQrowsBlock) {
            const uint32_t sl = s0 + threadIdx.x;
            uint2 sd = sd0;
            uint4 qa = qa0, qb = qb0;
            if (s0 != 0) {
                const uint32_t l = min(sl, nslot - 1);
                sd = sl < nslot ? qslot[l] : make_uint2(0xffffffffu, 0u);
                qa = qlane[2 * l];
                qb = qlane[2 * l + 1];
            }
            const uint32_t q = sd.x, le = sd.y & 0xffu, lgL = (sd.y >> 8) & 0xfu;
            const uint32_t itm[kQGroup] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
            double a[CB];
#pragma unroll
            for (int i = 0; i < CB; ++i) {
                double x = Pl[pix(npl, itm[0], i)];
#pragma unroll
                for (uint32_t u = 1; u < kQGroup; ++u) x = x + Pl[pix(npl, itm[u], i)];
                a[i] = x;
            }
            auto level = [&](uint32_t lv, auto part) {
                if (lv >= lglmax) return;  // uniform
#pragma unroll
                for (int i = 0; i < CB; ++i) {
                    const double o = part(a[i]), t = a[i] + o;
                    a[i] = lv < lgL ? t : a[i];  // a select, not a branch per value
                }
            };
            level(0, [](double v) { return quad_dpp<0xB1>(v); });   // quad_perm [1,0,3,2]
            level(1, [](double v) { return quad_dpp<0x4E>(v); });   // quad_perm [2,3,0,1]
            level(2, [](double v) { return quad_dpp<0x141>(v); });  // row_half_mirror
            level(3, [](double v) { return quad_dpp<0x140>(v); });  // row_mirror
            for (uint32_t lv = 4; lv < lglmax; ++lv)
#pragma unroll
                for (int i = 0; i < CB; ++i) {
                    const double o = __shfl_xor(a[i], 1 << lv);
                    if (lv < lgL) a[i] = a[i] + o;
                }
            if (q < ldQ && le == 0)
#pragma unroll
                for (int i = 0; i < CB; ++i)
                    if ((uint32_t)i < ncb) Q[(size_t)(c0 + i) * ldQ + q] = a[i];
        }
    } else
    for (uint32_t s0 = 0; s0 < nslot; s0 += kQrowsBlock) {
        const uint32_t sl = s0 + threadIdx.x;
        const uint2 sd = s0 == 0 ? sd0 : sl < nslot ? qslot[sl] : make_uint2(0xffffffffu, 0u);
        const uint32_t q = sd.x, le = sd.y & 0xffu, lgL = (sd.y >> 8) & 0xfu, lgG = (sd.y >> 12) & 0xfu;
        double a[CB];
#pragma unroll
        for (int i = 0; i < CB; ++i) a[i] = 0.0;
        if (q < ncoef) {
            const uint32_t i0 = Qs[q], i1 = Qs[q + 1];
            // this lane's group sums: one group (nvar <= 8: an entry has at
            // most C(8,4) = 70 items, 18 groups, so its segment takes them
            // one per lane), else 2^G consecutive groups in a binary counter
            auto group = [&](uint32_t j0, double *sg) {
#pragma unroll
                for (int i = 0; i < CB; ++i) sg[i] = 0.0;
                if (j0 >= i1) return;
                // items past the entry read the zero slot: x + (+0.0) = x for
                // these non-negative (or NaN / inf) values, so the sums are the
                // canonical order's bits without a select per item
                uint32_t itm[kQGroup];
#pragma unroll
                for (uint32_t u = 0; u < kQGroup; ++u) {
                    const uint32_t t_ = Qi[j0 + u < i1 ? j0 + u : j0];
                    itm[u] = j0 + u < i1 ? t_ + 16 : 0u;  // slots (nvar > 8: item + 16)
                }
#pragma unroll
                for (int i = 0; i < CB; ++i) {
                    double x = Pl[pix(npl, itm[0], i)];
#pragma unroll
                    for (uint32_t u = 1; u < kQGroup; ++u) x = x + Pl[pix(npl, itm[u], i)];
                    sg[i] = x;
                }
            };
            if constexpr (NV == 8) {
                group(i0 + le * kQGroup, a);
            } else {
                double lev[CB][kQLevelsRows];
                const uint32_t ng = 1u << lgG;
                for (uint32_t g = 0; g < ng; ++g) {
                    double sg[CB];
                    group(i0 + ((le << lgG) + g) * kQGroup, sg);
#pragma unroll
                    for (int l = 0; l < kQLevelsRows; ++l) {
                        if ((g >> l) & 1u) {
#pragma unroll
                            for (int i = 0; i < CB; ++i) sg[i] = lev[i][l] + sg[i];
                        } else {
#pragma unroll
                            for (int i = 0; i < CB; ++i) lev[i][l] = sg[i];
                            break;
                        }
                    }
                    if (g + 1 == ng)  // 2^G groups: the counter holds one block
#pragma unroll
                        for (int i = 0; i < CB; ++i) a[i] = sg[i];
                }
            }
        }
        // every lane of the wave takes part in every shuffle; a lane adds
        // only the levels inside its entry's segment
        for (uint32_t lv = 0; lv < lglmax; ++lv)  // lglmax: the widest segment's levels (uniform)
#pragma unroll
            for (int i = 0; i < CB; ++i) {
                const double o = __shfl_xor(a[i], 1 << lv);
                if (lv < lgL) a[i] = a[i] + o;
            }
        if (q < ldQ && le == 0)
#pragma unroll
            for (int i = 0; i < CB; ++i)
                if ((uint32_t)i < ncb) Q[(size_t)(c0 + i) * ldQ + q] = a[i];
    }
    MDP_STAMP(stamps, 3);
    MDP_RSTAMP(stamps, 7);
}

// One workgroup per c value.
//  1. stage this c's Z/PV block (LDS_ZPV) and the binomial table in LDS;
//  2. subset products: lane per part (pair p, 16 consecutive subset indexes k
//     of X = A&B): j = deposit(k, X), Pc[j][b] = Z_j prod_{var b not in j}
//     (B_b ? pC : 1-pC) accumulated into the part's per-|j| partial sums;
//  3. Q_ab[m] = sum of the pair's part partials, in part order;
//  4. lane per forward use: R[c][use][r] = sum_m Q[m] C(D-|A|, r-m), padded
//     to the even stride RSP, plus two zero transitions of prefetch padding.
// Every reduction runs in a fixed order, so results are deterministic.
template <bool LDS_ZPV, bool LDS_PART, int NV>
__global__ __launch_bounds__(kBlock) void k_coefs(
    const double *__restrict__ ZPV, uint32_t nstates, uint32_t nvar,
    const uint32_t *__restrict__ pairA, const uint32_t *__restrict__ pairB,
    const uint32_t *__restrict__ pairOff, const uint32_t *__restrict__ pairPart0,
    uint32_t npairs, const uint32_t *__restrict__ partP, const uint32_t *__restrict__ partK0,
    uint32_t nparts, uint32_t ncoef, const uint32_t *__restrict__ udesc, uint32_t nuses,
    uint32_t deg, double *__restrict__ R, size_t ldR, double *__restrict__ gpart,
    unsigned long long *__restrict__ stamps)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    MDP_RSTAMP(stamps, 6);
    MDP_STAMP(stamps, 0);
    const uint32_t ic = blockIdx.x;
    const size_t zsz = (size_t)(nvar + 1) * nstates;
    const double *zg = ZPV + (size_t)ic * zsz;
    double *base = lds;
    const double *zpv = zg;
    if constexpr (LDS_ZPV) {
        for (size_t i0 = 0; i0 < zsz; i0 += 8 * kBlock) {  // 8 loads in flight per lane
            double t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const size_t i = i0 + u * kBlock + threadIdx.x;
                if (i < zsz) t[u] = zg[i];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const size_t i = i0 + u * kBlock + threadIdx.x;
                if (i < zsz) lds[i] = t[u];
            }
        }
        zpv = lds;
        base = lds + zsz;
    }
    const uint32_t pw = nvar + 1;  // partial sums per part
    double *partial = LDS_PART ? base : gpart + (size_t)ic * nparts * pw;
    double *Qs = LDS_PART ? base + (size_t)nparts * pw : base;
    double *binom = Qs + ncoef;  // [kMaxDeg+1][kMaxDeg+1]
    for (uint32_t i = threadIdx.x; i < (kMaxDeg + 1) * (kMaxDeg + 1); i += kBlock)
        binom[i] = c_binom[i / (kMaxDeg + 1)][i % (kMaxDeg + 1)];
    __syncthreads();
    MDP_STAMP(stamps, 1);

    for (uint32_t it = threadIdx.x; it < nparts; it += kBlock) {
        const uint32_t p = partP[it], k0 = partK0[it];
        const uint32_t B = pairB[p], X = pairA[p] & B;
        const uint32_t nX = __popc(X);
        double *acc = partial + (size_t)it * pw;
        for (uint32_t m = 0; m <= nX; ++m) acc[m] = 0.0;
        const uint32_t k1 = min(k0 + kSubPart, 1u << nX);
        for (uint32_t k = k0; k < k1; ++k) {
            // deposit the bits of k into the positions of X (once X's bits are
            // used up `low` is 0 and the remaining steps are no-ops)
            uint32_t sub = 0, xs = X;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const uint32_t low = xs & (0u - xs);
                sub |= ((k >> i) & 1u) ? low : 0u;
                xs ^= low;
            }
            // branch-free: every factor load is issued up front (rows past
            // nvar are clamped and neutralised); bits of j contribute 1.0
            double f[NV];
#pragma unroll
            for (int b = 0; b < NV; ++b) {
                const uint32_t row = (uint32_t)b < nvar ? (uint32_t)b : nvar - 1;
                f[b] = zpv[(size_t)(1 + row) * nstates + sub];
            }
            double prod = zpv[sub];
#pragma unroll
            for (int b = 0; b < NV; ++b) {
                const uint32_t bit = nvar - 1 - (uint32_t)b;  // wraps past nvar: masked below
                const double g = ((B >> bit) & 1u) ? f[b] : 1.0 - f[b];
                const bool skip = (uint32_t)b >= nvar || ((sub >> bit) & 1u);
                prod *= skip ? 1.0 : g;
            }
            acc[__popc(k)] += prod;
        }
    }
    __syncthreads();
    MDP_STAMP(stamps, 2);
    for (uint32_t p = threadIdx.x; p < npairs; p += kBlock) {
        const uint32_t nX = __popc(pairA[p] & pairB[p]);
        const uint32_t q0 = pairPart0[p], q1 = pairPart0[p + 1];
        double *q = Qs + pairOff[p];
        for (uint32_t m = 0; m <= nX; ++m) {
            double a = 0.0;
            for (uint32_t t = q0; t < q1; ++t) a += partial[(size_t)t * pw + m];
            q[m] = a;
        }
    }
    __syncthreads();
    MDP_STAMP(stamps, 3);
    const uint32_t rsp = (deg + 2) & ~1u;
    double *Rc = R + (size_t)ic * ldR;
    for (uint32_t it = nuses * rsp + threadIdx.x; it < (nuses + 2) * rsp; it += kBlock) Rc[it] = 0.0;
    for (uint32_t u = threadIdx.x; u < nuses; u += kBlock) {
        const uint32_t d = udesc[u];
        const double *q = Qs + (d & kOffMask);
        const uint32_t nX = (d >> kOffBits) & 31u, nA = d >> 27;
        const uint32_t lift = deg - nA;
        const double *bl = binom + lift * (kMaxDeg + 1);
        double *dst = Rc + (size_t)u * rsp;
        for (uint32_t r = 0; r < rsp; ++r) {
            double a = 0.0;
            if (r <= deg) {
                const uint32_t m0 = r > lift ? r - lift : 0;
                const uint32_t m1 = r < nX ? r : nX;
                for (uint32_t m = m0; m <= m1; ++m) a += q[m] * bl[r - m];
            }
            dst[r] = a;
        }
    }
    MDP_STAMP(stamps, 4);
    MDP_RSTAMP(stamps, 7);
}

// Dot product of one transition's coefficients (wave-uniform, SGPRs) with a
// point's weights, as two interleaved partial sums for FMA latency.
template <int RS>
__device__ __forceinline__ double tdot(const double (&rc)[RS], const double (&w)[RS])
{
    double a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (int r = 0; r + 1 < RS; r += 2) {
        a0 = fma(rc[r], w[r], a0);
        a1 = fma(rc[r + 1], w[r + 1], a1);
    }
    if constexpr (RS & 1) a0 = fma(rc[RS - 1], w[RS - 1], a0);
    return a0 + a1;
}

// Coefficients are read through the constant address space: the data is
// read-only for the whole launch, so uniform reads become scalar loads even
// next to explicit s_waitcnt / sched_barrier intrinsics.
typedef const __attribute__((address_space(4))) double cdouble;

template <int RS>
__device__ __forceinline__ void tload(double (&dst)[RS], cdouble *src)
{
#pragma unroll
    for (int r = 0; r < RS; ++r) dst[r] = src[r];
}

// RS coefficients from a 16-byte aligned LDS block (ds_read_b128 pairs).
template <int RS>
__device__ __forceinline__ void tload_l(double (&dst)[RS], const double *src)
{
    const double2 *s2 = (const double2 *)src;
#pragma unroll
    for (int r = 0; r + 1 < RS; r += 2) {
        const double2 q = s2[r / 2];
        dst[r] = q.x;
        dst[r + 1] = q.y;
    }
    if constexpr (RS & 1) dst[RS - 1] = src[RS - 1];
}

// Forward recursion, EPL grid points per lane (e values ie, ie+256, ...), one
// c per workgroup.  Program `prog` (padded with one trailing word): one word
// per step, either a run of `count` consecutive 1x1 transitions (v0 *= P) or
// one general year (npp -> npc states, the reference's Pold*Pcur at :379).
// Inside a run the coefficient loads are software-pipelined two transitions
// ahead (R is padded by two transitions per c, so prefetches never leave it).  Q3 semantics (:368-369): start from ones over the
// year-0 states; L = sum_l v_l*prior0.
template <int NPMAX, int DEG, int EPL>
__global__ __launch_bounds__(kBlock) void k_forward(
    const double *__restrict__ R, size_t ldR, const uint32_t *__restrict__ prog, uint32_t nprog,
    uint32_t np0, double prior0, const double *__restrict__ evals, uint32_t ne,
    double *__restrict__ out, uint32_t ld_out, uint32_t out_cs)
{
    constexpr int RS = DEG + 1;
    constexpr int RSP = (DEG + 2) & ~1;  // per-transition stride in R
    const uint32_t ic = blockIdx.x;
    uint32_t ie[EPL];
    double W[EPL][RS];
    double v[EPL][NPMAX];
#pragma unroll
    for (int i = 0; i < EPL; ++i) {
        ie[i] = blockIdx.y * (kBlock * EPL) + i * kBlock + threadIdx.x;
        const double e = ie[i] < ne ? evals[ie[i]] : 0.0;
        const double x = e > 1.0 ? 1.0 : e;
        const double y = 1.0 - x;
        double yp[RS];
        yp[0] = 1.0;
#pragma unroll
        for (int r = 1; r < RS; ++r) yp[r] = yp[r - 1] * y;
        double xp = 1.0;
#pragma unroll
        for (int r = DEG; r >= 0; --r) {
            W[i][r] = xp * yp[r];
            xp *= x;
        }
#pragma unroll
        for (int k = 0; k < NPMAX; ++k) v[i][k] = (uint32_t)k < np0 ? 1.0 : 0.0;
    }

    cdouble *rp = (cdouble *)(R + (size_t)ic * ldR);  // next transition
    uint32_t op = prog[0];
    for (uint32_t pi = 0; pi < nprog; ++pi) {
        const uint32_t op_next = prog[pi + 1];
        if ((op & 1u) == 0) {
            // run of 1x1 transitions: ping-pong coefficient buffers.  Scalar
            // loads return out of order, so the only usable wait is
            // lgkmcnt(0): each half waits for its buffer, THEN issues the
            // other buffer's loads, then computes -- the loads fly under the
            // compute (sched_barrier keeps the compiler from sinking them).
            uint32_t cnt = op >> 1;
            double r0[RS], r1[RS];
            tload(r0, rp);
            for (; cnt >= 2; cnt -= 2) {
                double P[EPL];
                __builtin_amdgcn_s_waitcnt(kWaitLgkm0);
                __builtin_amdgcn_sched_barrier(0);
                tload(r1, rp + RSP);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < EPL; ++i) P[i] = tdot(r0, W[i]);
#pragma unroll
                for (int i = 0; i < EPL; ++i) v[i][0] = v[i][0] * P[i];
                __builtin_amdgcn_s_waitcnt(kWaitLgkm0);
                __builtin_amdgcn_sched_barrier(0);
                tload(r0, rp + 2 * RSP);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < EPL; ++i) P[i] = tdot(r1, W[i]);
#pragma unroll
                for (int i = 0; i < EPL; ++i) v[i][0] = v[i][0] * P[i];
                rp += 2 * RSP;
            }
            if (cnt) {
#pragma unroll
                for (int i = 0; i < EPL; ++i) v[i][0] = v[i][0] * tdot(r0, W[i]);
                rp += RSP;
            }
        } else {
            const uint32_t npp = (op >> 8) & 0xffu, npc = (op >> 16) & 0xffu;
            double vn[EPL][NPMAX];
#pragma unroll
            for (int l = 0; l < NPMAX; ++l) {
#pragma unroll
                for (int i = 0; i < EPL; ++i) vn[i][l] = 0.0;
                if ((uint32_t)l < npc) {
#pragma unroll
                    for (int k = 0; k < NPMAX; ++k) {
                        if ((uint32_t)k < npp) {
                            double rc[RS];
                            tload(rc, rp);
                            rp += RSP;
#pragma unroll
                            for (int i = 0; i < EPL; ++i) vn[i][l] = fma(v[i][k], tdot(rc, W[i]), vn[i][l]);
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < EPL; ++i)
#pragma unroll
                for (int l = 0; l < NPMAX; ++l) v[i][l] = vn[i][l];
        }
        op = op_next;
    }
    // v beyond the last year's state count is zero: the in-order sum over all
    // NPMAX slots adds exact zeros only
#pragma unroll
    for (int i = 0; i < EPL; ++i) {
        double L = 0.0;
#pragma unroll
        for (int l = 0; l < NPMAX; ++l) L += v[i][l] * prior0;
        if (ie[i] < ne) out[(size_t)ie[i] * ld_out + (size_t)ic * out_cs] = log(L);
    }
}



// Same recursion with the workgroup's whole coefficient block (and the step
// program) staged in LDS by wide coalesced loads: transitions are then read
// with in-order ds_read_b128 broadcasts instead of scalar loads, so there is no
// scalar-cache miss on the critical path.  Used when the block fits kFwdLds.
template <int NPMAX, int DEG, int EPL>
__global__ __launch_bounds__(kBlock) void k_forward_lds(
    const double *__restrict__ R, size_t ldR, const uint32_t *__restrict__ prog, uint32_t nprog,
    uint32_t np0, double prior0, const double *__restrict__ evals, uint32_t ne,
    double *__restrict__ out, uint32_t ld_out, uint32_t out_cs, unsigned long long *__restrict__ stamps)
{
    constexpr int RS = DEG + 1;
    constexpr int RSP = (DEG + 2) & ~1;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    MDP_RSTAMP(stamps, 6);
    MDP_STAMP(stamps, 0);
    double *Rl = lds;
    uint32_t *pl = (uint32_t *)(lds + ldR);
    const uint32_t ic = blockIdx.x;
    {
        const double2 *src = (const double2 *)(R + (size_t)ic * ldR);
        double2 *dst = (double2 *)Rl;
        const uint32_t n2 = (uint32_t)(ldR / 2);
        for (uint32_t i0 = threadIdx.x; i0 < n2; i0 += 4 * kBlock) {  // 4 loads in flight per lane
            const uint32_t i1 = i0 + kBlock, i2 = i0 + 2 * kBlock, i3 = i0 + 3 * kBlock;
            const double2 t0 = src[i0];
            const double2 t1 = src[i1 < n2 ? i1 : i0];
            const double2 t2 = src[i2 < n2 ? i2 : i0];
            const double2 t3 = src[i3 < n2 ? i3 : i0];
            dst[i0] = t0;
            if (i1 < n2) dst[i1] = t1;
            if (i2 < n2) dst[i2] = t2;
            if (i3 < n2) dst[i3] = t3;
        }
        for (uint32_t i = threadIdx.x; i <= nprog; i += kBlock) pl[i] = prog[i];
    }
    uint32_t ie[EPL];
    double W[EPL][RS];
    double v[EPL][NPMAX];
#pragma unroll
    for (int i = 0; i < EPL; ++i) {
        ie[i] = blockIdx.y * (kBlock * EPL) + i * kBlock + threadIdx.x;
        const double e = ie[i] < ne ? evals[ie[i]] : 0.0;
        const double x = e > 1.0 ? 1.0 : e;
        const double y = 1.0 - x;
        double yp[RS];
        yp[0] = 1.0;
#pragma unroll
        for (int r = 1; r < RS; ++r) yp[r] = yp[r - 1] * y;
        double xp = 1.0;
#pragma unroll
        for (int r = DEG; r >= 0; --r) {
            W[i][r] = xp * yp[r];
            xp *= x;
        }
#pragma unroll
        for (int k = 0; k < NPMAX; ++k) v[i][k] = (uint32_t)k < np0 ? 1.0 : 0.0;
    }
    __syncthreads();
    MDP_STAMP(stamps, 1);
    const double *rp = Rl;
    unsigned long long cyc_run = 0, cyc_gen = 0;  // diagnostic accounting only
    for (uint32_t pi = 0; pi < nprog; ++pi) {
        const uint32_t op = pl[pi];
        const unsigned long long t_op = stamps ? __builtin_amdgcn_s_memtime() : 0ull;
        if ((op & 1u) == 0) {
            uint32_t cnt = op >> 1;
            for (; cnt >= 2; cnt -= 2, rp += 2 * RSP) {
                double ra[RS], rb[RS];
                tload_l(ra, rp);
                tload_l(rb, rp + RSP);
#pragma unroll
                for (int i = 0; i < EPL; ++i) v[i][0] = v[i][0] * tdot(ra, W[i]);
#pragma unroll
                for (int i = 0; i < EPL; ++i) v[i][0] = v[i][0] * tdot(rb, W[i]);
            }
            if (cnt) {
                double ra[RS];
                tload_l(ra, rp);
                rp += RSP;
#pragma unroll
                for (int i = 0; i < EPL; ++i) v[i][0] = v[i][0] * tdot(ra, W[i]);
            }
        } else {
            const uint32_t npp = (op >> 8) & 0xffu, npc = (op >> 16) & 0xffu;
            double vn[EPL][NPMAX];
#pragma unroll
            for (int l = 0; l < NPMAX; ++l) {
#pragma unroll
                for (int i = 0; i < EPL; ++i) vn[i][l] = 0.0;
                if ((uint32_t)l < npc) {
#pragma unroll
                    for (int k = 0; k < NPMAX; ++k) {
                        if ((uint32_t)k < npp) {
                            double rc[RS];
                            tload_l(rc, rp);
                            rp += RSP;
#pragma unroll
                            for (int i = 0; i < EPL; ++i) vn[i][l] = fma(v[i][k], tdot(rc, W[i]), vn[i][l]);
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < EPL; ++i)
#pragma unroll
                for (int l = 0; l < NPMAX; ++l) v[i][l] = vn[i][l];
        }
        if (stamps) {
            const unsigned long long dt = __builtin_amdgcn_s_memtime() - t_op;
            if (op & 1u) cyc_gen += dt;
            else cyc_run += dt;
        }
    }
    if (stamps && threadIdx.x == 0) {
        stamps[(size_t)(blockIdx.x + gridDim.x * blockIdx.y) * kStampSlots + 3] = cyc_run;
        stamps[(size_t)(blockIdx.x + gridDim.x * blockIdx.y) * kStampSlots + 4] = cyc_gen;
    }
#pragma unroll
    for (int i = 0; i < EPL; ++i) {
        double L = 0.0;
#pragma unroll
        for (int l = 0; l < NPMAX; ++l) L += v[i][l] * prior0;
        if (ie[i] < ne) out[(size_t)ie[i] * ld_out + (size_t)ic * out_cs] = log(L);
    }
    MDP_STAMP(stamps, 2);
    MDP_RSTAMP(stamps, 7);
}

// ---------------------------------------------------------------------------
// wide path: years with more observed states than the register-resident
// forward kernels hold (npmax > 16, i.e. more than 4 missing patches in one
// year; main_MIDASPOM.c:225-251 expands 2^k states for any k and propagates
// them with dgemm, :371-384).  Same direct-path algebra (Q per (X, B) group,
// DESIGN.md §3), but nothing has to fit a workgroup: the item factors and Q
// rows go through HBM/L2, and the state vectors live in an HBM scratch laid
// out [state][point] so every lane's access is coalesced.
// ---------------------------------------------------------------------------

// Pg[cl * ldp + it] = Pc[j][B] of item `it` at c = cvals[c0 + cl] (ldp: nitems,
// or nitems + 1 for k_fwd_hs, whose rows end in a zero slot): Z_row(c) times the
// var-column factors f_b = B_b ? pC_b : 1 - pC_b, pC_b = min(1, c S[j][b])
// (1.0 for the columns of j, marked +inf in sv: fmin(c inf, 1) = 1.0),
// combined in k_qrows' pairwise tree over NV slots -- the same bits k_qrows
// produces.
template <int NV>
__global__ __launch_bounds__(kBlock) void k_witems(const double *__restrict__ cvals, uint32_t nc, uint32_t c0,
                                                   uint32_t nvar, const double *__restrict__ Zg,
                                                   const double *__restrict__ sv, uint32_t nitems,
                                                   const uint2 *__restrict__ items, double *__restrict__ Pg,
                                                   uint32_t ldp)
{
    const uint32_t it = blockIdx.x * kBlock + threadIdx.x, cl = blockIdx.y;
    if (it >= nitems) return;
    const double c = cvals[c0 + cl];
    const uint2 t = items[it];
    const uint32_t r = (t.x >> 24) | ((t.y >> 24) << 8), nB = ~t.x;
    double f[NV];
#pragma unroll
    for (int b = 0; b < NV; ++b) {
        const double sb = (uint32_t)b < nvar ? sv[(size_t)r * nvar + b] : HUGE_VAL;
        const double p = fmin(c * sb, 1.0);  // (k_qrows' form: +inf marks give 1.0)
        const uint32_t nbit = (uint32_t)b < nvar ? (nB >> (nvar - 1 - (uint32_t)b)) & 1u : 0u;
        f[b] = (double)nbit - p;  // |n - p|: k_qrows' fold
    }
#pragma unroll
    for (int b = 0; b < NV; b += 2) f[b] = fabs(f[b]) * fabs(f[b + 1]);
#pragma unroll
    for (int sh = 2; sh < NV; sh *= 2)
#pragma unroll
        for (int b = 0; b + sh < NV; b += 2 * sh) f[b] *= f[b + sh];
    Pg[(size_t)cl * ldp + it] = Zg[(size_t)r * nc + c0 + cl] * f[0];
}

// Q[c0 + cl][q] = the q-th entry's items summed in CSR (ascending j) order,
// as k_qrows sums them; zero in the padding slots up to ldQ.
__global__ __launch_bounds__(kBlock) void k_wq(uint32_t c0, uint32_t nitems, const double *__restrict__ Pg,
                                               uint32_t ncoef, const uint32_t *__restrict__ qstart,
                                               const uint32_t *__restrict__ qitem, double *__restrict__ Q,
                                               uint32_t ldQ)
{
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x, cl = blockIdx.y;
    if (q >= ldQ) return;
    double a = 0.0;
    if (q < ncoef) {  // the canonical order (kQGroup): groups, binary counter, fold
        const double *pl = Pg + (size_t)cl * nitems;
        const uint32_t i0 = qstart[q], i1 = qstart[q + 1];
        double lev[kQLevels];
        uint32_t g = 0;
        for (uint32_t i = i0; i < i1; i += kQGroup, ++g) {
            double sg = pl[qitem[i]];
            for (uint32_t u = 1; u < kQGroup && i + u < i1; ++u) sg = sg + pl[qitem[i + u]];
#pragma unroll
            for (int l = 0; l < kQLevels; ++l) {
                if ((g >> l) & 1u) {
                    sg = lev[l] + sg;
                } else {
                    lev[l] = sg;
                    break;
                }
            }
        }
        bool have = false;
#pragma unroll
        for (int l = 0; l < kQLevels; ++l)
            if ((g >> l) & 1u) {
                a = have ? lev[l] + a : lev[l];
                have = true;
            }
    }
    Q[(size_t)(c0 + cl) * ldQ + q] = a;
}

// Wide years on the matrix cores (FP64 MFMA, v_mfma_f64_16x16x4_f64).  For
// one column c and a block of PTS points, year t's new state vector is
//     n[p][l] = sum_(k, m) W[p][(k, m)] C[(k, m)][l],
//     W[p][(k, m)] = v[p][k] x_p^(|A_k| - m) y_p^m,   C[(k, m)][l] = Q_kl[m]
// (0 past the transition's nX): the transition P[k][l] = sum_m Q_kl[m]
// x^(|A|-m) y^m of the wide kernels (direct weights, as k_fwd_wide), summed
// over K = every source's (k, m <= |A_k|) -- one GEMM per year of M = the
// points, N = the new states, K = sum_k (|A_k| + 1), on the matrix cores with
// the states of the block's points in LDS.  Each MFMA computes the transposed
// tile n^T = C^T W^T (A operand: the gathered C values, states x K; B: the
// W values, K x points), so a lane's accumulators are 4 states of one point
// and the year's stores are rows of 16 consecutive points (conflict-free).
// C's fragments are gathered from the column's Q row: a lane's K entry (k, m,
// the LDS rows of v_k, x^(|A_k|-m) and y^m) names the transition descriptor
// (k, l) (host table, c-independent: the Q-row offset of the transition's
// coefficients and its nX), and m <= nX picks the slot, else the zero slot.
// 16 waves, one work item each per year: (column tile, every row tile, slice
// of the year's K chunks) -- with S = min(16 / ncol, room, nch / 2) slices, so
// that up to 16 waves are busy in a year of any size.  Slice 1 leaves its
// partial products in the year's own destination rows, later slices in the
// state buffer's rows past the year's column tiles; slice 0 adds them in
// slice order (deterministic).  Each lane's K entries run three chunks ahead
// in a ring of four register slots (loaded once, straight from the table in
// HBM: staging three years of them in LDS was 1-5 % slower), the
// transition descriptors two and the C gathers one; the loop body is
// unrolled four times so the slots are fixed.  The products sum in another
// order than k_fwd_wide's (positive terms: ~1e-15 relative).
typedef double mdp_d4 __attribute__((ext_vector_type(4)));
template <int NPM>  // states per year, padded (64, 128 or 256)
__global__ __launch_bounds__(kMmaThreads) void k_fwd_mma(
    const double *__restrict__ Q, uint32_t ldQ, const uint32_t *__restrict__ np, const uint2 *__restrict__ kt,
    const uint32_t *__restrict__ kbase, const uint32_t *__restrict__ desc, const uint32_t *__restrict__ dbase,
    const uint2 *__restrict__ wplan, uint32_t tmax, double prior0, const double *__restrict__ evals, uint32_t ne,
    uint32_t c0, uint32_t maxA, uint32_t ktmax, uint32_t zslot, double *__restrict__ out, uint32_t ld_out,
    uint32_t out_cs)
{
    constexpr uint32_t PTS = mma_pts(NPM), ROWS = mma_rows(NPM), PS = mma_ps(NPM), RT = PTS / 16;
    static_assert(NPM <= (int)ROWS && NPM <= 256, "state rows");
    extern __shared__ __attribute__((aligned(16))) double mlds[];
    double *Va = mlds, *Vb = mlds + (size_t)ROWS * PTS;  // [state][point]
    double *xp = Vb + (size_t)ROWS * PTS, *yp = xp + (size_t)(maxA + 1) * PS;  // [r][point]
    const uint32_t lane = threadIdx.x & 63u, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform
    const uint32_t p0 = blockIdx.x * PTS, ic = c0 + blockIdx.y;
    if (threadIdx.x < PTS) {
        const uint32_t ie = p0 + threadIdx.x;
        const double e = ie < ne ? evals[ie] : 0.0;
        const double x = e > 1.0 ? 1.0 : e, y = 1.0 - x;
        double a = 1.0, b = 1.0;
        for (uint32_t r = 0; r <= maxA; ++r) {
            xp[r * PS + threadIdx.x] = a;
            yp[r * PS + threadIdx.x] = b;
            a *= x;
            b *= y;
        }
    }
    const uint32_t np0 = np[0];
    for (uint32_t i = threadIdx.x; i < (uint32_t)NPM * PTS; i += kMmaThreads) Va[i] = i / PTS < np0 ? 1.0 : 0.0;
    __syncthreads();
    const double *q = Q + (size_t)ic * ldQ;
    const uint32_t kk = lane >> 4, col = lane & 15u;
    // this wave's work item of year t
    struct Item {
        uint32_t npc, npcp, nch, nit, S, item, ks, cb, ce, sh, lc4;
        bool active;
        const uint2 *kl;
        const uint32_t *dt;
    };
    // (the host's work split, mma_wave_plan: one scalar load, no divisions)
    auto plan = [&](uint32_t t) {
        Item it;
        it.npc = np[t];
        const uint32_t ncol = (it.npc + 15) / 16;
        it.npcp = ncol * 16;
        it.nch = (kbase[t + 1] - kbase[t]) / (4 * kMmaU);
        it.nit = ncol;
        const uint2 wp = wplan[t * 16 + wv];
        it.cb = wp.x & 0xffffu;
        it.ce = wp.x >> 16;
        it.item = wp.y & 0xffu;
        it.ks = (wp.y >> 8) & 0xffu;
        it.S = (wp.y >> 16) & 0xffu;
        it.active = (wp.y >> 24) != 0u;
        // descriptor rows [k][2^sh >= npcp] (row npp: the padded entries')
        it.sh = 32u - (uint32_t)__builtin_clz(it.npcp - 1u);
        it.lc4 = (it.item * 16 + col) << 2;
        it.kl = kt + __builtin_amdgcn_readfirstlane(kbase[t]);
        it.dt = desc + __builtin_amdgcn_readfirstlane(dbase[t]);
        return it;
    };
    // the lane's K entry (kk) of step u of chunk ch (clamped into the year)
    auto kent = [&](const Item &it, uint32_t ch, uint32_t u) {
        const uint32_t c = ch < it.nch ? ch : it.nch - 1;
        return it.kl[(c * kMmaU + u) * 4 + kk];
    };
    // (32-bit byte offsets from uniform bases: the loads take the scalar-base
    // form, with no 64-bit address arithmetic per lane)
    auto dsc = [&](const Item &it, uint2 en) {
        const uint32_t k = (en.y >> 21) & 0xffu;
        return *(const uint32_t *)((const char *)it.dt + ((k << (it.sh + 2)) + it.lc4));
    };
    // C[(k, m)][l]: the slot of Q_kl[m], or the Q row's zero slot (ldQ > ncoef;
    // absent transitions' descriptors name it with nX = 0)
    auto cval = [&](uint2 en, uint32_t d) {
        const uint32_t m = (en.y >> 16) & 31u;
        return *(const double *)((const char *)q + ((m <= ((d >> kOffBits) & 31u) ? (d & kOffMask) + m : zslot) << 3));
    };
    // rings by chunk position j = ch - cb (mod 4 / mod 2): K entries of ch ..
    // ch + 3, descriptors of ch + 1 and ch + 2, C values of ch and ch + 1
    uint2 ee[4][kMmaU];
    uint32_t dd[2][kMmaU];
    double bb[2][kMmaU];
    // an item's first chunks, in two parts: the K entries and descriptors
    // (prime_a), the first C gathers once the descriptors are in (prime_b)
    auto prime_a = [&](const Item &it) {
#pragma unroll
        for (uint32_t u = 0; u < kMmaU; ++u) {
            ee[0][u] = kent(it, it.cb, u);
            ee[1][u] = kent(it, it.cb + 1, u);
            ee[2][u] = kent(it, it.cb + 2, u);
        }
#pragma unroll
        for (uint32_t u = 0; u < kMmaU; ++u) {
            dd[0][u] = dsc(it, ee[0][u]);
            dd[1][u] = dsc(it, ee[1][u]);
        }
    };
    auto prime_b = [&]() {
#pragma unroll
        for (uint32_t u = 0; u < kMmaU; ++u) bb[0][u] = cval(ee[0][u], dd[0][u]);
    };
    Item cur = plan(tmax > 1 ? 1u : 0u);
    if (tmax > 1 && cur.active) {
        prime_a(cur);
        prime_b();
    }
    for (uint32_t t = 1; t < tmax; ++t) {
        mdp_d4 acc[RT];
#pragma unroll
        for (uint32_t h = 0; h < RT; ++h) acc[h] = mdp_d4{0.0, 0.0, 0.0, 0.0};
        // one chunk at ring position j: the K entries of ch + 3, the
        // descriptors of ch + 2, the C values of ch + 1, then ch's products (W
        // formed unconditionally: padded entries name row 0 and meet C = 0)
        auto chunk = [&](uint32_t ch, auto jc) {
            constexpr uint32_t j = decltype(jc)::value;
#pragma unroll
            for (uint32_t u = 0; u < kMmaU; ++u) ee[(j + 3) & 3][u] = kent(cur, ch + 3, u);
#pragma unroll
            for (uint32_t u = 0; u < kMmaU; ++u) dd[j & 1][u] = dsc(cur, ee[(j + 2) & 3][u]);
#pragma unroll
            for (uint32_t u = 0; u < kMmaU; ++u) bb[(j + 1) & 1][u] = cval(ee[(j + 1) & 3][u], dd[(j + 1) & 1][u]);
#pragma unroll
            for (uint32_t u = 0; u < kMmaU; ++u) {
                const uint2 en = ee[j][u];
#pragma unroll
                for (uint32_t h = 0; h < RT; ++h) {
                    const uint32_t pb = (h * 16 + col) * 8u;
                    const double wt = *(const double *)((const char *)xp + (en.x >> 16) + pb) *
                                      *(const double *)((const char *)yp + (en.y & 0xffffu) + pb);
                    const double av = *(const double *)((const char *)Va + (en.x & 0xffffu) + pb) * wt;
                    acc[h] = __builtin_amdgcn_mfma_f64_16x16x4f64(bb[j & 1][u], av, acc[h], 0, 0, 0);
                }
            }
        };
        if (cur.active)
        {
            // whole rounds of four chunks with no branch between them (a
            // branch join made the compiler wait for every load in flight at
            // each chunk), then the last one to three
            uint32_t ch = cur.cb;
            for (; ch + 4 <= cur.ce; ch += 4) {
                chunk(ch, std::integral_constant<uint32_t, 0>{});
                chunk(ch + 1, std::integral_constant<uint32_t, 1>{});
                chunk(ch + 2, std::integral_constant<uint32_t, 2>{});
                chunk(ch + 3, std::integral_constant<uint32_t, 3>{});
            }
            if (ch < cur.ce) chunk(ch, std::integral_constant<uint32_t, 0>{});
            if (ch + 1 < cur.ce) chunk(ch + 1, std::integral_constant<uint32_t, 1>{});
            if (ch + 2 < cur.ce) chunk(ch + 2, std::integral_constant<uint32_t, 2>{});
        }
        // next year's first chunks in flight across this year's barriers
        // (its K entries were staged a year ago): descriptors now, C values
        // after the partial sums
        const Item nxt = plan(t + 1 < tmax ? t + 1 : t);
        const bool pnext = t + 1 < tmax && nxt.active;
        if (pnext) prime_a(nxt);
        // the lane's accumulators: states item * 16 + kk + 4 r of point
        // h * 16 + col; slice 1 stores them in place, slice j >= 2 past row
        // npcp ((S - 2) x ncol x 16 PTS doubles at most, within the buffer)
        double *dst = Vb + (size_t)(cur.item * 16 + kk) * PTS + col;
        auto part = [&](uint32_t j) {
            return Vb + (size_t)cur.npcp * PTS + (size_t)((j - 2) * cur.nit + cur.item) * (RT * 256) + lane;
        };
        if (cur.active && cur.ks == 1)
#pragma unroll
            for (uint32_t h = 0; h < RT; ++h)
#pragma unroll
                for (uint32_t r = 0; r < 4; ++r) dst[(size_t)(4 * r) * PTS + h * 16] = acc[h][r];
        if (cur.active && cur.ks >= 2) {
            double *pk = part(cur.ks);
#pragma unroll
            for (uint32_t h = 0; h < RT; ++h)
#pragma unroll
                for (uint32_t r = 0; r < 4; ++r) pk[(h * 4 + r) * 64] = acc[h][r];
        }
        if (cur.S > 1) __syncthreads();
        if (cur.active && cur.ks == 0) {
            if (cur.S > 1)
#pragma unroll
                for (uint32_t h = 0; h < RT; ++h)
#pragma unroll
                    for (uint32_t r = 0; r < 4; ++r) acc[h][r] = acc[h][r] + dst[(size_t)(4 * r) * PTS + h * 16];
            for (uint32_t j = 2; j < cur.S; ++j) {
                const double *pj = part(j);
#pragma unroll
                for (uint32_t h = 0; h < RT; ++h)
#pragma unroll
                    for (uint32_t r = 0; r < 4; ++r) acc[h][r] = acc[h][r] + pj[(h * 4 + r) * 64];
            }
            // (padded states l >= npc hold 0: their C values are the zero slot)
#pragma unroll
            for (uint32_t h = 0; h < RT; ++h)
#pragma unroll
                for (uint32_t r = 0; r < 4; ++r) dst[(size_t)(4 * r) * PTS + h * 16] = acc[h][r];
        }
        if (pnext) prime_b();
        __syncthreads();
        double *tv = Va;
        Va = Vb;
        Vb = tv;
        cur = nxt;
    }
    if (threadIdx.x < PTS) {
        const uint32_t ie = p0 + threadIdx.x, npl = np[tmax - 1];
        double L = 0.0;
        for (uint32_t l = 0; l < npl; ++l) L += Va[l * PTS + threadIdx.x] * prior0;
        if (ie < ne) out[(size_t)ie * ld_out + (size_t)ic * out_cs] = log(L);
    }
}

// k_fwd_mmt<RT, ROWS, DB> (round 6): the per-year GEMM of k_fwd_mma, for
// years of up to 1 024 states, with three changes.
//  * K lists per (year, column tile): the entry (k, m) only for m <= the
//    largest nX over the tile's 16 new states (k_fwd_mma ran m up to |A_k|
//    for every tile and multiplied the rest through zero slots), and the
//    gathers' Q-row offsets per (entry, new state) from a host table, so no
//    descriptor lookup sits between a K entry and its gather.
//  * Years of more than 128 states (ROWS 256 / 512 / 1 024, 32 / 32 / 16
//    points a block): ONE state buffer in LDS (DB = false, 64 / 128 / 128
//    KiB): a wave keeps its tiles' new states in registers until every wave
//    has read the year's old ones (a barrier), then stores them in place.  A
//    wave owns up to ROWS / 256 tiles a year (17-64 tiles over 16 waves,
//    longest lists first).  Years of up to 128 states keep k_fwd_mma's two
//    buffers (DB = true, 64 points a block, one barrier a year).
//  * Years of at most 16 tiles give every tile a wave and the spare waves to
//    the tiles with the longest lists (a tile's list split into slices of at
//    least two chunks); slice 1 parks its partial products in the tile's own
//    destination rows (two buffers) or past the year's tiles (one buffer),
//    later slices past the year's tiles, and slice 0 adds them in slice
//    order after a barrier (deterministic).
// Workgroups are dealt XCD-aware (the point blocks of one column on one XCD,
// so the column's Q row is gathered from that XCD's L2).  The products sum
// in another order than k_fwd_wide's (positive terms: ~1e-15 relative).
// the instantiations (RT point tiles of 16, ROWS state rows, two buffers or
// one): <4, 128, true> years of up to 128 states, <2, 256, false> 256,
// <2, 512, false> 512, <1, 1 024, false> 1 024 (mmt_shape)
template <int RT, int ROWS, bool DB>
__global__ __launch_bounds__(kMmaThreads) void k_fwd_mmt(
    const double *__restrict__ Q, uint32_t ldQ, const uint32_t *__restrict__ np, const uint2 *__restrict__ kt,
    const uint32_t *__restrict__ cidx, const uint2 *__restrict__ ktile, const uint2 *__restrict__ wplan, uint32_t tmax,
    double prior0, const double *__restrict__ evals, uint32_t ne, uint32_t maxA, double *__restrict__ out,
    uint32_t ld_out, uint32_t out_cs)
{
    constexpr uint32_t PTS = mmt_pts(RT), PS = mmt_ps(RT), TMAX = ROWS > 256 ? ROWS / 256 : 1, U = mmt_u(RT);
    static_assert(TMAX * RT <= 4 && (ROWS <= 256 || TMAX * 256 == ROWS), "tiles per wave");
    extern __shared__ __attribute__((aligned(16))) double mlds[];
    double *Va = mlds, *Vb = DB ? mlds + (size_t)ROWS * PTS : mlds;  // [state][point]: read / written
    double *xp = mlds + (DB ? 2 : 1) * (size_t)ROWS * PTS, *yp = xp + (size_t)(maxA + 1) * PS;  // [r][point]
    const uint32_t lane = threadIdx.x & 63u, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // XCD-aware: workgroups are dealt round-robin over the 8 XCDs; XCD x
    // takes a contiguous range of logical blocks, i.e. whole columns
    const uint32_t npb = (ne + PTS - 1) / PTS, full = gridDim.x & ~7u, b = blockIdx.x;
    const uint32_t lb = b < full ? (b & 7u) * (full >> 3) + (b >> 3) : b;
    const uint32_t p0 = (lb % npb) * PTS, ic = lb / npb;
    if (threadIdx.x < PTS) {
        const uint32_t ie = p0 + threadIdx.x;
        const double e = ie < ne ? evals[ie] : 0.0;
        const double x = e > 1.0 ? 1.0 : e, y = 1.0 - x;
        double a = 1.0, c = 1.0;
        for (uint32_t r = 0; r <= maxA; ++r) {
            xp[r * PS + threadIdx.x] = a;
            yp[r * PS + threadIdx.x] = c;
            a *= x;
            c *= y;
        }
    }
    const uint32_t np0 = np[0];
    for (uint32_t i = threadIdx.x; i < ROWS * PTS; i += kMmaThreads) Va[i] = i / PTS < np0 ? 1.0 : 0.0;
    __syncthreads();
    const double *q = Q + (size_t)ic * ldQ;
    const uint32_t kk = lane >> 4, col = lane & 15u;
    struct Item {
        uint32_t tile, ks, S, pbase, cb, ce, nch, npcp;
        bool active, split;
        const uint2 *kl;
        const uint32_t *cl;
    };
    // item i of this wave in year t (host table mmt_wplan: no divisions here)
    auto plan = [&](uint32_t t, uint32_t i) {
        Item it;
        it.npcp = (np[t] + 15) / 16 * 16;
        const uint2 wp = wplan[(t * 16 + wv) * TMAX + i];
        it.cb = wp.x & 0xffffu;
        it.ce = wp.x >> 16;
        it.tile = wp.y & 0xffu;
        it.ks = (wp.y >> 8) & 15u;      // slice of the tile's K list
        it.S = (wp.y >> 12) & 31u;      // the tile's slices
        it.pbase = (wp.y >> 17) & 31u;  // its partial blocks (slices 1 .. S - 1) from here
        it.split = (wp.y >> 22) & 1u;   // some tile of the year is sliced (uniform)
        it.active = (wp.y >> 24) != 0u;
        const uint2 kt2 = ktile[t * kMmtMaxTiles + it.tile];
        const uint32_t k0 = __builtin_amdgcn_readfirstlane(kt2.x);
        it.kl = kt + k0;
        it.cl = cidx + (size_t)k0 * 16;
        it.nch = kt2.y;
        return it;
    };
    // K entry (uint2, one per 16 lanes): x = V row byte offset (18 bits) |
    // y^m row offset << 18, y = x^(|A|-m) row offset (16 bits) | m << 16 | k
    // << 21; and per lane the byte offset in the Q row of C[(k, m)][l] --
    // Q_kl[m], or the zero slot where m > nX or l is a padded state (host
    // table, so no descriptor lookup is on the gather's path)
    auto kent = [&](const Item &it, uint32_t ch, uint32_t u) {
        const uint32_t c = ch < it.nch ? ch : it.nch - 1;
        return it.kl[(c * U + u) * 4 + kk];
    };
    auto coff = [&](const Item &it, uint32_t ch, uint32_t u) {
        const uint32_t c = ch < it.nch ? ch : it.nch - 1;
        return it.cl[(c * U + u) * 64 + lane];
    };
    auto cval = [&](uint32_t o) { return *(const double *)((const char *)q + o); };
    // rings by chunk position j = ch - cb: K entries of ch .. ch + 3 (mod
    // 4), C offsets of ch + 1 and ch + 2 (mod 2; ch's were consumed by its
    // gathers), C values of ch and ch + 1 (mod 2)
    uint2 ee[4][U];
    uint32_t dd[2][U];
    double bb[2][U];
    auto prime_a = [&](const Item &it) {
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            ee[0][u] = kent(it, it.cb, u);
            ee[1][u] = kent(it, it.cb + 1, u);
            ee[2][u] = kent(it, it.cb + 2, u);
            dd[0][u] = coff(it, it.cb, u);
            dd[1][u] = coff(it, it.cb + 1, u);
        }
    };
    auto prime_b = [&]() {
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) bb[0][u] = cval(dd[0][u]);
    };
    Item cur = plan(tmax > 1 ? 1u : 0u, 0);
    if (tmax > 1 && cur.active) {
        prime_a(cur);
        prime_b();
    }
    for (uint32_t t = 1; t < tmax; ++t) {
        mdp_d4 acc[TMAX][RT];
        const Item first = cur;
#pragma unroll
        for (uint32_t i = 0; i < TMAX; ++i) {
#pragma unroll
            for (uint32_t h = 0; h < RT; ++h) acc[i][h] = mdp_d4{0.0, 0.0, 0.0, 0.0};
            if (i > 0) {
                cur = plan(t, i);
                if (!cur.active) break;  // a wave's items are its first ones
                prime_a(cur);
                prime_b();
            }
            if (!cur.active) break;
            mdp_d4(&ac)[RT] = acc[i];  // (i is a constant once unrolled)
            // one chunk at ring position j: the K entries of ch + 3, the C
            // values of ch + 1 (their offsets loaded a chunk ago), the C
            // offsets of ch + 2, then ch's products
            auto chunk = [&](uint32_t ch, auto jc) {
                constexpr uint32_t j = decltype(jc)::value;
#pragma unroll
                for (uint32_t u = 0; u < U; ++u) ee[(j + 3) & 3][u] = kent(cur, ch + 3, u);
#pragma unroll
                for (uint32_t u = 0; u < U; ++u) bb[(j + 1) & 1][u] = cval(dd[(j + 1) & 1][u]);
#pragma unroll
                for (uint32_t u = 0; u < U; ++u) dd[j & 1][u] = coff(cur, ch + 2, u);
#pragma unroll
                for (uint32_t u = 0; u < U; ++u) {
                    const uint2 en = ee[j][u];
#pragma unroll
                    for (uint32_t h = 0; h < RT; ++h) {
                        const uint32_t pb = (h * 16 + col) * 8u;
                        const double wt = *(const double *)((const char *)xp + (en.y & 0xffffu) + pb) *
                                          *(const double *)((const char *)yp + (en.x >> 18) + pb);
                        const double av = *(const double *)((const char *)Va + (en.x & 0x3ffffu) + pb) * wt;
                        ac[h] = __builtin_amdgcn_mfma_f64_16x16x4f64(bb[j & 1][u], av, ac[h], 0, 0, 0);
                    }
                }
            };
            uint32_t ch = cur.cb;
            for (; ch + 4 <= cur.ce; ch += 4) {
                chunk(ch, std::integral_constant<uint32_t, 0>{});
                chunk(ch + 1, std::integral_constant<uint32_t, 1>{});
                chunk(ch + 2, std::integral_constant<uint32_t, 2>{});
                chunk(ch + 3, std::integral_constant<uint32_t, 3>{});
            }
            if (ch < cur.ce) chunk(ch, std::integral_constant<uint32_t, 0>{});
            if (ch + 1 < cur.ce) chunk(ch + 1, std::integral_constant<uint32_t, 1>{});
            if (ch + 2 < cur.ce) chunk(ch + 2, std::integral_constant<uint32_t, 2>{});
        }
        // next year's first item: K entries and descriptors in flight across
        // this year's barriers, its first C values after them
        const Item nxt = plan(t + 1 < tmax ? t + 1 : t, 0);
        const bool pnext = t + 1 < tmax && nxt.active;
        if (pnext) prime_a(nxt);
        if constexpr (!DB) __syncthreads();  // one buffer: every wave has read the year's old states
        // the lane's accumulators: states tile * 16 + kk + 4 r of point
        // h * 16 + col.  A sliced tile's slices ks >= 1 park theirs: slice 1
        // of two buffers in the tile's destination rows, the rest past row
        // npcp in partial block pbase + ks - (DB ? 2 : 1) of the year (the
        // host keeps them within ROWS rows)
        auto dst_of = [&](uint32_t tile) { return Vb + (size_t)(tile * 16 + kk) * PTS + col; };
        auto park = [&](uint32_t ks) {
            return Vb + (size_t)(first.npcp + (first.pbase + ks - (DB ? 2u : 1u)) * 16) * PTS + lane;
        };
        if (first.split) {
            if (first.active && first.ks >= 1) {
                if (DB && first.ks == 1) {
                    double *dst = dst_of(first.tile);
#pragma unroll
                    for (uint32_t h = 0; h < RT; ++h)
#pragma unroll
                        for (uint32_t r = 0; r < 4; ++r) dst[(size_t)(4 * r) * PTS + h * 16] = acc[0][h][r];
                } else {
                    double *pk = park(first.ks);
#pragma unroll
                    for (uint32_t h = 0; h < RT; ++h)
#pragma unroll
                        for (uint32_t r = 0; r < 4; ++r) pk[(h * 4 + r) * 64] = acc[0][h][r];
                }
            }
            __syncthreads();
            if (first.active && first.ks == 0)
                for (uint32_t j = 1; j < first.S; ++j) {
                    if (DB && j == 1) {
                        const double *dst = dst_of(first.tile);
#pragma unroll
                        for (uint32_t h = 0; h < RT; ++h)
#pragma unroll
                            for (uint32_t r = 0; r < 4; ++r)
                                acc[0][h][r] = acc[0][h][r] + dst[(size_t)(4 * r) * PTS + h * 16];
                    } else {
                        const double *pj = park(j);
#pragma unroll
                        for (uint32_t h = 0; h < RT; ++h)
#pragma unroll
                            for (uint32_t r = 0; r < 4; ++r) acc[0][h][r] = acc[0][h][r] + pj[(h * 4 + r) * 64];
                    }
                }
            // (the final stores below go to rows < npcp, never to a parked
            // block, and a tile's slice-1 rows are read only by its slice 0)
        }
        // (padded states l >= npc hold 0: their C values are the zero slot)
#pragma unroll
        for (uint32_t i = 0; i < TMAX; ++i) {
            const Item it = i == 0 ? first : plan(t, i);
            if (!it.active || it.ks != 0) break;
            double *dst = dst_of(it.tile);
#pragma unroll
            for (uint32_t h = 0; h < RT; ++h)
#pragma unroll
                for (uint32_t r = 0; r < 4; ++r) dst[(size_t)(4 * r) * PTS + h * 16] = acc[i][h][r];
        }
        if (pnext) prime_b();
        __syncthreads();
        if constexpr (DB) {
            double *tv = Va;
            Va = Vb;
            Vb = tv;
        }
        cur = nxt;
    }
    if (threadIdx.x < PTS) {
        const uint32_t ie = p0 + threadIdx.x, npl = np[tmax - 1];
        double L = 0.0;
        for (uint32_t l = 0; l < npl; ++l) L += Va[l * PTS + threadIdx.x] * prior0;
        if (ie < ne) out[(size_t)ie * ld_out + (size_t)ic * out_cs] = log(L);
    }
}

// k_fwd_hs<RT, NB, NW> (round 6): the wide forward through the hidden
// states.  The reference's own factorisation (main_MIDASPOM.c:18-50, :363,
// :371-384): P = Pe Pc over the hidden states j, so year t is
//     U[p][j] = y^|j| sum_{k: A_k >= j} v[p][k] x^(|A_k| - |j|)    (v Pe)
//     n[p][l] = sum_{j <= B_l} Pc[j][B_l] U[p][j]                  (U Pc)
// instead of one (nX+1)-term polynomial per transition (k, l): for a year of
// 2^f completions of f unvisited patches that is ~3^f (j, l) terms per
// point, not ~2^f 2^f (|A|+1) -- 10-25x fewer for years of 256-1 024 states.
// An NW-wave block's 16 RT points keep one vector over the whole 2^NB cube
// of hidden states in LDS, V[j][p] (NB = max(8, nvar) <= 10; 64 or 128 KiB),
// plus a y^k table:
//  * v Pe: Pe is a tensor product over the patches (per patch: occupied ->
//    extinct w.p. x, survives w.p. y), applied in place by passes of up to
//    kHsRadix patches of W = the bits occupied in some state of year t - 1:
//    a thread loads a coset's positions, runs the butterflies V[j] +=
//    x V[j | b] in registers and writes back, y^|j| applied in the year's
//    last pass.  The host's pass tables (build_hs_plan) name per coset the
//    positions to read and to write -- only those whose value still reaches
//    a hidden state the year's products read -- and give a wave's cosets the
//    same masks, so uniform branches skip the rest;
//  * U Pc: the per-year GEMM on the matrix cores as k_fwd_mmt's, with K = the
//    hidden states j a column tile of new states reaches, the W operand
//    U[j][p] read straight from the cube, and the C operand Pc[j][B_l]
//    gathered from the column's item factors (k_witems' Pg rows, ld =
//    nitems + 1: a zero slot at nitems for j not <= B_l) through a host
//    table of offsets;
//  * the year's new states are stored at their own cube positions B_l (after
//    a barrier: U is dead by then), ready for the next year's passes.
// Tiles are dealt to waves as k_fwd_mmt's (longest lists first past NW
// tiles; smaller years give the spare waves slices of the longest lists,
// parked in 16-row cube blocks that hold none of the year's states).  Q3
// semantics: ones at year 0's states; L = prior0 x the sum over the last
// year's states.  Sums reordered against the reference's (positive terms
// for e in [0, 1]: ~1e-15 relative).
constexpr uint32_t kHsPre = 4;    // k_fwd_hs: v Pe passes a year whose descriptors are loaded up front
// diag build, MDP_HS_PROBE bit 2: workgroup 0's wave 0 stamps the shader
// clock at each phase of each year into out[] (results not stored)
#ifdef MDP_DIAG_BUILD
#define MDP_HS_STAMP(k)                                                                                      \
    do {                                                                                                     \
        if ((probe & 4u) && blockIdx.x == 0 && threadIdx.x == 0) out[(size_t)t * 8 + (k)] = (double)clock64(); \
    } while (0)
#else
#define MDP_HS_STAMP(k) do { } while (0)
#endif
template <int RT, int NB, int NW>
__global__ __launch_bounds__(NW * 64, 4) void k_fwd_hs(  // (4 waves a SIMD: two 8-wave blocks a CU)
    const double *__restrict__ Pg, uint32_t ldp, uint32_t c0, const uint32_t *__restrict__ np,
    const uint32_t *__restrict__ kt, const uint32_t *__restrict__ cidx, const uint4 *__restrict__ wplan,
    const uint4 *__restrict__ pass, const uint32_t *__restrict__ pbase, const uint2 *__restrict__ ppos, const uint32_t *__restrict__ dpos, const uint32_t *__restrict__ dbase,
    const uint2 *__restrict__ dpk, const uint32_t *__restrict__ pk, uint32_t tmax, double prior0, const double *__restrict__ evals, uint32_t ne,
    double *__restrict__ out, uint32_t ld_out, uint32_t out_cs, uint32_t probe)
{
    constexpr uint32_t PTS = mmt_pts(RT), NC = 1u << NB, NTH = NW * 64, TMAX = NC / 16 > NW ? NC / 16 / NW : 1,
                       U = mmt_u(RT);
    static_assert(TMAX * RT <= 4 && NC * PTS <= 16384 && NTH % PTS == 0, "cube and tiles");
    extern __shared__ __attribute__((aligned(16))) double mlds[];
    double *V = mlds;  // [j][point]
    const uint32_t lane = threadIdx.x & 63u, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // XCD-aware: XCD x takes a contiguous range of logical blocks (whole columns)
    const uint32_t npb = (ne + PTS - 1) / PTS, full = gridDim.x & ~7u, b = blockIdx.x;
    const uint32_t lb = b < full ? (b & 7u) * (full >> 3) + (b >> 3) : b;
    const uint32_t p0 = (lb % npb) * PTS, cl = lb / npb, ic = c0 + cl;
    // this thread's point in the pass loops (NTH is a multiple of PTS)
    const uint32_t pp = threadIdx.x % PTS;
    double xq, yq;
    {
        const uint32_t ie = p0 + pp;
        const double e = ie < ne ? evals[ie] : 0.0;
        xq = e > 1.0 ? 1.0 : e;
        yq = 1.0 - xq;
    }
    // the cube starts at zero (a position no year has written holds a finite
    // value whenever it is read: padded K entries meet it with C = 0), then
    // ones at year 0's states (Q3)
    for (uint32_t i = threadIdx.x; i < NC * PTS; i += NTH) V[i] = 0.0;
    __syncthreads();
    {
        const uint32_t n0 = (np[0] + 15) / 16 * 16, d0 = dbase[0];
        for (uint32_t i = threadIdx.x; i < n0 * PTS; i += NTH) {
            const uint32_t pos = dpos[d0 + i / PTS];
            if (pos != ~0u) V[pos * PTS + i % PTS] = 1.0;
        }
    }
    __syncthreads();
    const double *q = Pg + (size_t)cl * ldp;
    const uint32_t kk = lane >> 4, col = lane & 15u;
    struct Item {
        uint32_t tile, ks, S, pbase, cb, ce, nch;
        bool active, split;
        const uint32_t *kl, *cl;
    };
    // item i of this wave in year t (wplan: chunk range, tile | slice |
    // slices | park base | split | valid, the tile's K-list start and
    // chunks: one scalar load, no dependent one)
    auto plan = [&](uint32_t t, uint32_t i) {
        Item it;
        const uint4 wp = wplan[(t * NW + wv) * TMAX + i];
        it.cb = wp.x & 0xffffu;
        it.ce = wp.x >> 16;
        it.tile = wp.y & 0xffu;
        it.ks = (wp.y >> 8) & 15u;
        it.S = (wp.y >> 12) & 31u;
        it.pbase = (wp.y >> 17) & 31u;
        it.split = (wp.y >> 22) & 1u;
        it.active = (wp.y >> 24) != 0u;
        const uint32_t k0 = __builtin_amdgcn_readfirstlane(wp.z);
        it.kl = kt + k0;
        it.cl = cidx + (size_t)k0 * 16;
        it.nch = wp.w;
        return it;
    };
    // K entry (one per 16 lanes): the LDS byte offset of U's row j; per lane
    // the byte offset of Pc[j][B_l] in the column's Pg row (or its zero slot)
    auto kent = [&](const Item &it, uint32_t ch, uint32_t u) {
        const uint32_t c = ch < it.nch ? ch : it.nch - 1;
        return it.kl[(c * U + u) * 4 + kk];
    };
    auto coff = [&](const Item &it, uint32_t ch, uint32_t u) {
        const uint32_t c = ch < it.nch ? ch : it.nch - 1;
        return it.cl[(c * U + u) * 64 + lane];
    };
    auto cval = [&](uint32_t o) { return *(const double *)((const char *)q + o); };
    uint32_t ee[4][U];
    uint32_t dd[2][U];
    double bb[2][U];
    auto prime = [&](const Item &it) {
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            ee[0][u] = kent(it, it.cb, u);
            ee[1][u] = kent(it, it.cb + 1, u);
            ee[2][u] = kent(it, it.cb + 2, u);
            dd[0][u] = coff(it, it.cb, u);
            dd[1][u] = coff(it, it.cb + 1, u);
        }
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) bb[0][u] = cval(dd[0][u]);
    };
    // y^k of the thread's point (the v Pe passes' last scaling)
    double *ypw = mlds + (size_t)NC * PTS;  // [k][point], k <= NB
    if (threadIdx.x < PTS) {
        double a = 1.0;
        for (uint32_t k = 0; k <= (uint32_t)NB; ++k, a *= yq) ypw[k * PTS + threadIdx.x] = a;
    }
    __syncthreads();
    // one coset of a v Pe pass (R patches, bit masks mb): read the positions
    // of mask inm (the rest count as 0), the R butterflies V[j] += x V[j | b]
    // in registers, write the positions of mask outm (those some later pass
    // or the year's products read) -- in the year's last pass times y^|j|
    // (a wave's cosets share their masks, build_hs_plan: uniform branches
    // skip the positions no lane of the wave reads or writes)
    auto coset = [&](auto rc, uint2 ce, const uint32_t (&mb)[kHsRadix], bool last) {
        constexpr uint32_t R = decltype(rc)::value, NQ = 1u << R;
        const uint32_t my = __builtin_amdgcn_readfirstlane(ce.y);
        const uint32_t g = ce.x, inm = my & 0xffffu, outm = my >> 16;
        auto pos = [&](uint32_t qq) {
            uint32_t o = g;
#pragma unroll
            for (uint32_t k = 0; k < R; ++k) o |= (qq >> k) & 1u ? mb[k] : 0u;
            return o;
        };
        double v[NQ];
#pragma unroll
        for (uint32_t qq = 0; qq < NQ; ++qq) {
            if ((inm >> qq) & 1u)
                v[qq] = V[(size_t)pos(qq) * PTS + pp];
            else
                v[qq] = 0.0;
        }
#pragma unroll
        for (uint32_t k = 0; k < R; ++k)
#pragma unroll
            for (uint32_t qq = 0; qq < NQ; ++qq)
                if (qq & (1u << k)) v[qq ^ (1u << k)] = fma(xq, v[qq], v[qq ^ (1u << k)]);
        if (last) {
            double sc[R + 1];
            sc[0] = ypw[__builtin_popcount(g) * PTS + pp];
#pragma unroll
            for (uint32_t k = 1; k <= R; ++k) sc[k] = sc[k - 1] * yq;
#pragma unroll
            for (uint32_t qq = 0; qq < NQ; ++qq) v[qq] *= sc[__builtin_popcount(qq)];
        }
#pragma unroll
        for (uint32_t qq = 0; qq < NQ; ++qq)
            if ((outm >> qq) & 1u) V[(size_t)pos(qq) * PTS + pp] = v[qq];
    };
    // v Pe pass tables of a year: the pass range, the first kHsPre passes'
    // descriptors and this thread's first coset of each -- loaded a year
    // ahead (during the previous year's products), so no year waits on them
    const uint32_t i0 = threadIdx.x / PTS;
    uint32_t pb0 = 0, pb1 = 0;
    uint4 pdp[kHsPre];
    uint2 cep[kHsPre];
    auto load_passes = [&](uint32_t ty) {
        pb0 = pbase[ty];
        pb1 = (probe & 1u) ? pb0 : pbase[ty + 1];
#pragma unroll
        for (uint32_t k = 0; k < kHsPre; ++k)
            if (pb0 + k < pb1) {
                pdp[k] = pass[pb0 + k];
                cep[k] = i0 < pdp[k].z ? ppos[pdp[k].w + i0] : make_uint2(0u, 0u);
            }
    };
    if (tmax > 1) load_passes(1);
    for (uint32_t t = 1; t < tmax; ++t) {
        // the year's first work item: its K entries, C offsets and first C
        // values do not depend on the cube, so their loads are in flight
        // through the v Pe passes; so are the positions its new states are
        // stored at (dpk: 4 x 16 bits per lane and tile, 0xffff: padding)
        mdp_d4 acc[TMAX][RT];
        Item cur = plan(t, 0);
        const Item first = cur;
        if (cur.active && !(probe & 2u)) prime(cur);
        const uint32_t db = dbase[t];
        uint2 dk[TMAX];
#pragma unroll
        for (uint32_t i = 0; i < TMAX; ++i) {
            const uint4 w2 = wplan[(t * NW + wv) * TMAX + i];
            dk[i] = (w2.y >> 24) ? dpk[(db / 16 + (w2.y & 0xffu)) * 4 + kk] : make_uint2(~0u, ~0u);
        }
        // v Pe: U[j] = y^|j| sum_{A >= j} v[A] x^(|A| - |j|), the patches of
        // W up to kHsRadix at a time (pass table: the r patches' bit
        // positions, r, cosets, coset-list base)
        MDP_HS_STAMP(0);
        for (uint32_t ps = pb0; ps < pb1; ++ps) {
            const uint32_t k0 = ps - pb0;
            if (ps == pb0) MDP_HS_STAMP(1);
            uint4 pd;
            if (k0 < kHsPre) {
                pd = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
                for (uint32_t k = 0; k < kHsPre; ++k)
                    if (k == k0) pd = pdp[k];
            } else {
                pd = pass[ps];
            }
            const uint32_t r = pd.y, ncos = pd.z, base = pd.w;
            const bool last = ps + 1 == pb1;
            uint32_t mb[kHsRadix];
#pragma unroll
            for (uint32_t k = 0; k < kHsRadix; ++k) mb[k] = k < r ? 1u << ((pd.x >> (5 * k)) & 31u) : 0u;
            for (uint32_t i = i0; i < ncos; i += NTH / PTS) {
                uint2 ce;
                if (i == i0 && k0 < kHsPre) {
                    ce = make_uint2(0u, 0u);
#pragma unroll
                    for (uint32_t k = 0; k < kHsPre; ++k)
                        if (k == k0) ce = cep[k];
                } else {
                    ce = ppos[base + i];
                }
                if (r == 4) coset(std::integral_constant<uint32_t, 4>{}, ce, mb, last);
                else if (r == 3) coset(std::integral_constant<uint32_t, 3>{}, ce, mb, last);
                else if (r == 2) coset(std::integral_constant<uint32_t, 2>{}, ce, mb, last);
                else coset(std::integral_constant<uint32_t, 1>{}, ce, mb, last);
            }
            __syncthreads();
        }
        MDP_HS_STAMP(2);
        // U Pc on the matrix cores
#pragma unroll
        for (uint32_t i = 0; i < TMAX; ++i) {
#pragma unroll
            for (uint32_t h = 0; h < RT; ++h) acc[i][h] = mdp_d4{0.0, 0.0, 0.0, 0.0};
            if (i > 0) cur = plan(t, i);
            if (!cur.active || (probe & 2u)) break;  // a wave's items are its first ones
            if (i > 0) prime(cur);
            mdp_d4(&ac)[RT] = acc[i];  // (i is a constant once unrolled)
            auto chunk = [&](uint32_t ch, auto jc) {
                constexpr uint32_t j = decltype(jc)::value;
#pragma unroll
                for (uint32_t u = 0; u < U; ++u) ee[(j + 3) & 3][u] = kent(cur, ch + 3, u);
#pragma unroll
                for (uint32_t u = 0; u < U; ++u) bb[(j + 1) & 1][u] = cval(dd[(j + 1) & 1][u]);
#pragma unroll
                for (uint32_t u = 0; u < U; ++u) dd[j & 1][u] = coff(cur, ch + 2, u);
#pragma unroll
                for (uint32_t u = 0; u < U; ++u) {
                    const uint32_t joff = ee[j][u];
#pragma unroll
                    for (uint32_t h = 0; h < RT; ++h) {
                        const double av = *(const double *)((const char *)V + joff + (h * 16 + col) * 8u);
                        ac[h] = __builtin_amdgcn_mfma_f64_16x16x4f64(bb[j & 1][u], av, ac[h], 0, 0, 0);
                    }
                }
            };
            uint32_t ch = cur.cb;
            for (; ch + 4 <= cur.ce; ch += 4) {
                chunk(ch, std::integral_constant<uint32_t, 0>{});
                chunk(ch + 1, std::integral_constant<uint32_t, 1>{});
                chunk(ch + 2, std::integral_constant<uint32_t, 2>{});
                chunk(ch + 3, std::integral_constant<uint32_t, 3>{});
            }
            if (ch < cur.ce) chunk(ch, std::integral_constant<uint32_t, 0>{});
            if (ch + 1 < cur.ce) chunk(ch + 1, std::integral_constant<uint32_t, 1>{});
            if (ch + 2 < cur.ce) chunk(ch + 2, std::integral_constant<uint32_t, 2>{});
        }
        MDP_HS_STAMP(3);
        if (t + 1 < tmax) load_passes(t + 1);
        __syncthreads();  // every wave has read U
        MDP_HS_STAMP(4);
        // the lane's accumulators: new states tile * 16 + kk + 4 r (tile
        // order) of point h * 16 + col
        auto store = [&](uint2 d2, const mdp_d4 (&a)[RT]) {
#pragma unroll
            for (uint32_t r = 0; r < 4; ++r) {
                const uint32_t pos = ((r < 2 ? d2.x : d2.y) >> (16 * (r & 1))) & 0xffffu;
                if (pos == 0xffffu) continue;
                double *dst = V + (size_t)pos * PTS + col;
#pragma unroll
                for (uint32_t h = 0; h < RT; ++h) dst[h * 16] = a[h][r];
            }
        };
        // a sliced tile's slices ks >= 1 park their partials in 16-row
        // blocks of the cube that hold none of the year's states (host table
        // pk: U is dead, and the next year's butterflies write such a
        // position before reading it); slice 0 adds them in slice order
        if (first.split) {
            auto park = [&](uint32_t ks) { return V + (size_t)pk[t * 16 + first.pbase + ks - 1] * PTS + lane; };
            if (first.active && first.ks >= 1) {
                double *pkp = park(first.ks);
#pragma unroll
                for (uint32_t h = 0; h < RT; ++h)
#pragma unroll
                    for (uint32_t r = 0; r < 4; ++r) pkp[(h * 4 + r) * 64] = acc[0][h][r];
            }
            __syncthreads();
            if (first.active && first.ks == 0)
                for (uint32_t j = 1; j < first.S; ++j) {
                    const double *pj = park(j);
#pragma unroll
                    for (uint32_t h = 0; h < RT; ++h)
#pragma unroll
                        for (uint32_t r = 0; r < 4; ++r) acc[0][h][r] = acc[0][h][r] + pj[(h * 4 + r) * 64];
                }
            __syncthreads();  // parked blocks read before any tile's store
        }
#pragma unroll
        for (uint32_t i = 0; i < TMAX; ++i) {
            const Item it = i == 0 ? first : plan(t, i);
            if (!it.active || it.ks != 0) break;
            store(dk[i], acc[i]);
        }
        MDP_HS_STAMP(5);
        __syncthreads();
        MDP_HS_STAMP(6);
    }
    if (threadIdx.x < PTS && !(probe & 4u)) {
        const uint32_t ie = p0 + threadIdx.x, dl = dbase[tmax - 1], npl = (np[tmax - 1] + 15) / 16 * 16;
        double L = 0.0;
        for (uint32_t l = 0; l < npl; ++l) {
            const uint32_t pos = dpos[dl + l];
            if (pos != ~0u) L += V[pos * PTS + threadIdx.x] * prior0;
        }
        if (ie < ne) out[(size_t)ie * ld_out + (size_t)ic * out_cs] = log(L);
    }
}

typedef const __attribute__((address_space(4))) uint32_t cuint;

// Forward recursion with the state vectors in HBM: lane per e value, one c
// per workgroup row (blockIdx.y = c0 + row).  Year t's vector is formed
// kWideLB target states at a time, each source state's probability loaded
// once per block of targets; a transition's coefficients (its group's Q
// entries) and its use descriptor are wave-uniform scalar loads.  The weight
// x^(|A|-m) y^m is xp[|A|-m] yp[m] from per-lane power tables in LDS.  Q3
// semantics (:368-369, :386-392): ones over the year-0 states, L = prior0 sum v.
constexpr uint32_t kWideLB = 4;
__global__ __launch_bounds__(kBlock) void k_fwd_wide(
    const double *__restrict__ Q, uint32_t ldQ, const uint32_t *__restrict__ udesc,
    const uint32_t *__restrict__ np, uint32_t tmax, double prior0, const double *__restrict__ evals, uint32_t ne,
    uint32_t c0, uint32_t maxA, double *__restrict__ V, uint32_t npmax, double *__restrict__ out, uint32_t ld_out,
    uint32_t out_cs)
{
    extern __shared__ double xy[];  // [2][maxA + 1][kBlock]: x^r, y^r per lane
    const uint32_t ie = blockIdx.x * kBlock + threadIdx.x, cl = blockIdx.y, ic = c0 + cl;
    const double e = ie < ne ? evals[ie] : 0.0;
    const double x = e > 1.0 ? 1.0 : e, y = 1.0 - x;
    double *xp = xy + threadIdx.x, *yp = xy + (size_t)(maxA + 1) * kBlock + threadIdx.x;
    {
        double a = 1.0, b = 1.0;
        for (uint32_t r = 0; r <= maxA; ++r) {
            xp[r * kBlock] = a;
            yp[r * kBlock] = b;
            a *= x;
            b *= y;
        }
    }
    cdouble *q = (cdouble *)(Q + (size_t)ic * ldQ);
    cuint *ud = (cuint *)udesc;
    cuint *npc_ = (cuint *)np;
    // V[buf][state][row][lane]: rows of this launch x the padded e extent
    const size_t cs = (size_t)gridDim.y * gridDim.x * kBlock;  // one state's stride
    double *va = V + (size_t)cl * gridDim.x * kBlock + ie;
    double *vb = va + (size_t)npmax * cs;
    const uint32_t np0 = npc_[0];
    for (uint32_t k = 0; k < np0; ++k) va[k * cs] = 1.0;
    uint32_t ubase = 0, npp = np0;
    for (uint32_t t = 1; t < tmax; ++t) {
        const uint32_t npc = npc_[t];
        for (uint32_t l0 = 0; l0 < npc; l0 += kWideLB) {
            double acc[kWideLB];
#pragma unroll
            for (uint32_t i = 0; i < kWideLB; ++i) acc[i] = 0.0;
            for (uint32_t k = 0; k < npp; ++k) {
                const double vk = va[k * cs];
#pragma unroll
                for (uint32_t i = 0; i < kWideLB; ++i) {
                    if (l0 + i >= npc) break;
                    const uint32_t d = ud[ubase + (l0 + i) * npp + k];
                    const uint32_t off = d & kOffMask, nX = (d >> kOffBits) & 31u, nA = d >> 27;
                    double P = 0.0;
                    for (uint32_t m = 0; m <= nX; ++m) P = fma(q[off + m], xp[(nA - m) * kBlock] * yp[m * kBlock], P);
                    acc[i] = fma(vk, P, acc[i]);
                }
            }
#pragma unroll
            for (uint32_t i = 0; i < kWideLB; ++i)
                if (l0 + i < npc) vb[(l0 + i) * cs] = acc[i];
        }
        ubase += npp * npc;
        npp = npc;
        double *tmp = va;
        va = vb;
        vb = tmp;
    }
    double L = 0.0;
    for (uint32_t l = 0; l < npp; ++l) L += va[l * cs] * prior0;
    if (ie < ne) out[(size_t)ie * ld_out + (size_t)ic * out_cs] = log(L);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

constexpr int kNumEv = 6;  // start/stop per kernel: k_zpv, k_coefs, k_forward

// record a launched kernel instantiation ("k_qrows<16,0,2>", ...): the name
// is formatted and looked up in the engine's set (fmt is a launch site's
// literal, handed on by note_launch)
void note_launch_fmt(const mdp_engine *eng, const char *fmt, ...)
{
    char b[96];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(b, sizeof b, fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> lk(eng->launched_mu);
    if (eng->launched.find(b) == eng->launched.end()) eng->launched.emplace(b);
}

inline uint64_t note_arg(const char *s) { return (uint64_t)(uintptr_t)s; }  // (a string literal: by address)
template <typename T>
inline uint64_t note_arg(T v) { return (uint64_t)v; }

// Every launch site notes its instantiation, so on the hot path this runs
// once per kernel launch: a context remembers the (format, arguments) it has
// noted -- a few words compared in place, no formatting, lock or allocation
// -- and only one it has not seen yet goes through note_launch_fmt.
template <typename... A>
inline void note_launch(const mdp_engine *eng, const DevCtx &d, const char *fmt, A... a)
{
    static_assert(sizeof...(A) <= 4, "LaunchNote holds four arguments");
    const LaunchNote n{fmt, {note_arg(a)...}};
    for (const LaunchNote &m : d.noted)
        if (m.fmt == n.fmt && memcmp(m.a, n.a, sizeof n.a) == 0) return;
    d.noted.push_back(n);
    note_launch_fmt(eng, fmt, a...);
}

// the device's LDS per workgroup (the current device; 160 KiB on gfx950)
size_t device_lds_max()
{
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess && v > 0)
        return (size_t)v;
    return 160 * 1024;
}

// raise a kernel's dynamic LDS limit
template <typename K>
int set_lds_limit(K *kernel, size_t bytes)
{
    HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return MDP_OK;
}

// the LDS limits of the wide path's forward kernels: the plan's matrix-core
// instantiation and k_fwd_wide
int wide_lds_limits(const mdp_engine *eng)
{
    int rc = MDP_OK;
    if (eng->path == MdpPath::WideMma)
        rc = for_mma(eng, [&](auto npm) { return set_lds_limit(k_fwd_mma<npm()>, mma_lds(eng)); });
    if (eng->path == MdpPath::WideMmt)
        rc = for_mmt(eng, [&](auto rt, auto rows, auto db) {
            return set_lds_limit(k_fwd_mmt<rt(), rows(), db()>, mmt_lds(eng));
        });
    if (eng->path == MdpPath::WideHs)
        rc = for_hs(eng, [&](auto rt, auto nb, auto nw) { return set_lds_limit(k_fwd_hs<rt(), nb(), nw()>, hs_lds(eng)); });
    return rc ? rc : set_lds_limit(k_fwd_wide, wide_lds(eng));
}

// the c tables of a grid plan onto the device
int upload_ctables(DevCtx &d)
{
    const MdpCTables &t = d.ct;
    int rc;
    if ((rc = d.zs.assign(t.zs)) || (rc = d.zsq.assign(t.zsq)) || (rc = d.zc.assign(t.zc))) return rc;
    return t.coltab.empty() ? MDP_OK : d.coltab.assign(t.coltab);
}

// Load a code object; if the runtime refuses it (a stale or foreign object
// from the disk cache), rebuild it from its source once and retry.
hipError_t load_module(std::vector<char> &code, const std::string &src, hipModule_t *m)
{
    hipError_t e = hipModuleLoadData(m, code.data());
    if (e == hipSuccess || src.empty()) return e;
    std::string log;
    if (mdp_jit_compile(src, code, log, true) != 0) return e;
    return hipModuleLoadData(m, code.data());
}

// Load a forward kernel variant (jit_build's) into the device, compiling it if needed.
int jit_load(mdp_engine *eng, DevCtx &d, int variant)
{
    if (!eng->chunks.empty()) {  // a long series: its chunk kernels (never fused)
        const size_t nch = eng->chunks.size();
        if (d.cfn.size() == nch) return MDP_OK;
        int rc = jit_build_chunks(eng);
        if (rc) return rc;
        HIP_TRY(hipSetDevice(d.device));
        // every chunk loads into locals first and is committed to the device
        // context only when all have: a failure part-way leaves nothing
        // loaded, so a later call retries instead of running some chunks
        std::vector<hipModule_t> mods;
        std::vector<hipFunction_t> fns;
        std::vector<DevBuf<uint32_t>> qidx(nch);  // (freed with this scope unless committed)
        auto unload = [&]() { for (hipModule_t m : mods) (void)hipModuleUnload(m); };
        for (size_t i = 0; i < nch; ++i) {
            hipModule_t m;
            hipFunction_t f;
            hipError_t e = load_module(eng->chunk_code[i], i < eng->chunk_src.size() ? eng->chunk_src[i] : std::string(), &m);
            if (e == hipSuccess) {
                mods.push_back(m);
                e = hipModuleGetFunction(&f, m, "mdp_fwd_jit");
            }
            if (e != hipSuccess) {
                unload();
                return mdp_set_error(MDP_EHIP, "loading forward chunk %zu failed: %s", i, hipGetErrorString(e));
            }
            fns.push_back(f);
            if (!eng->chunks[i].qidx.empty() && (rc = qidx[i].assign(eng->chunks[i].qidx))) {
                unload();
                return rc;
            }
        }
        d.cmod = std::move(mods);
        d.cfn = std::move(fns);
        d.cqidx = std::move(qidx);
        return MDP_OK;
    }
    if (d.jit_fn[variant]) return MDP_OK;
    int rc = jit_build(eng, variant);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(d.device));
    hipModule_t m = nullptr;
    hipFunction_t f = nullptr;
    HIP_TRY(load_module(eng->jit_code[variant], eng->jit_src[variant], &m));
    const hipError_t e = hipModuleGetFunction(&f, m, "mdp_fwd_jit");
    if (e != hipSuccess) {
        (void)hipModuleUnload(m);
        return mdp_set_error(MDP_EHIP, "hipModuleGetFunction(mdp_fwd_jit) failed: %s", hipGetErrorString(e));
    }
    d.jit_mod[variant] = m;
    d.jit_fn[variant] = f;
    return MDP_OK;
}

int upload_binomials()  // into the current device's constant bank
{
    double h[kMaxDeg + 1][kMaxDeg + 1] = {};
    for (int a = 0; a <= kMaxDeg; ++a) {
        h[a][0] = 1.0;
        for (int b = 1; b <= a; ++b) h[a][b] = h[a][b - 1] * (double)(a - b + 1) / (double)b;
    }
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_binom), h, sizeof(h)));
    return MDP_OK;
}

// The generic path's device tables: colonisation sums S of every state
// (k_colsum), the binomial table, the pair plans, k_coefs' LDS limit.
int init_generic(mdp_engine *eng, DevCtx &d, const mdp_problem *p)
{
    int rc = upload_binomials();
    if (rc) return rc;
    std::vector<uint32_t> var(p->var_cols, p->var_cols + p->nvar), row_col;
    std::vector<uint8_t> isvar(p->n, 0);
    for (uint32_t b = 0; b < p->nvar; ++b) isvar[p->var_cols[b]] = 1;
    for (uint32_t k = 0; k < p->n; ++k)
        if (!isvar[k]) row_col.push_back(k);
    for (uint32_t b = 0; b < p->nvar; ++b) row_col.push_back(p->var_cols[b]);
    std::vector<double> M(p->M, p->M + (size_t)p->n * p->n);
    DevBuf<double> dM;  // k_colsum's input only
    if ((rc = dM.assign(M))) return rc;
    if ((rc = d.var_cols.assign(var)) || (rc = d.row_col.assign(row_col)) ||
        (rc = d.pairA.assign(eng->pairA)) || (rc = d.pairB.assign(eng->pairB)) ||
        (rc = d.pairOff.assign(eng->pairOff)) || (rc = d.udesc.assign(eng->udesc)) ||
        (rc = d.pairPart0.assign(eng->pairPart0)) || (rc = d.partP.assign(eng->partP)) ||
        (rc = d.partK0.assign(eng->partK0)) ||
        (rc = d.prog.assign(eng->prog)) ||
        (rc = d.S.grow((size_t)p->n * eng->nstates)))
        return rc;
    dim3 grid((eng->nstates + kBlock - 1) / kBlock, p->n);
    hipLaunchKernelGGL(k_colsum, grid, dim3(kBlock), 0, d.stream, dM.get(), d.var_cols.get(), d.row_col.get(), p->n, p->nvar,
                       eng->nstates, d.S.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(d.stream));
    if (eng->coef_lds > 64 * 1024)
        return for_coefs(eng, [&](auto ldsz, auto ldsp, auto nv) {
            return set_lds_limit(k_coefs<ldsz(), ldsp(), nv()>, eng->coef_lds);
        });
    return MDP_OK;
}

int init_device(mdp_engine *eng, DevCtx &d, const mdp_problem *p)
{
    HIP_TRY(hipSetDevice(d.device));
    HIP_TRY(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
    mdp_plan_steps(eng, d.plan);  // until a grid is set: the steps the path alone implies (mdp_engine_kernel_name)
    // the generic path's tables (k_zpv / k_coefs / k_forward: colonisation
    // sums of every state, binomials, pair plans) only for an engine that
    // runs it: the direct and wide paths never touch them, so their set-up
    // does not load the library's precompiled kernels at all (CLI start-up)
    if (eng->path == MdpPath::Generic) return init_generic(eng, d, p);
    int rc = MDP_OK;
    std::vector<double> sv;
    std::vector<uint2> items;
    mdp_plan_item_tables(eng, sv, items);
    std::vector<uint32_t> qitem = eng->qitem;
    qitem.push_back(0u);
    if ((rc = d.sv.assign(sv)) || (rc = d.items.assign(items)) ||
        (rc = d.qstart.assign(eng->qstart)) || (rc = d.qitem.assign(qitem)) ||
        (rc = d.qslot.assign(eng->qslot)) || (rc = d.qlane.assign(eng->qlane)) ||
        (rc = d.islot.assign(eng->islot)))
        return rc;
    // (k_qrows' LDS attribute is set before its first launch and the forward
    // kernel loaded by set_grid_dev: nothing here loads a module)
    if (!path_is_wide(eng->path)) return MDP_OK;
    if ((rc = d.np_d.assign(eng->np)) || (rc = d.udesc_w.assign(eng->udesc_d))) return rc;
    switch (eng->path) {
    case MdpPath::WideMma:
        if ((rc = d.mma_kt.assign(eng->mma_kt)) || (rc = d.mma_kbase.assign(eng->mma_kbase)) ||
            (rc = d.mma_wplan.assign(eng->mma_wplan)) ||
            (rc = d.mma_desc.assign(eng->mma_desc)) || (rc = d.mma_dbase.assign(eng->mma_dbase)))
            return rc;
        break;
    case MdpPath::WideMmt:
        if ((rc = d.mmt_kt.assign(eng->mmt_kt)) || (rc = d.mmt_ktile.assign(eng->mmt_ktile)) ||
            (rc = d.mmt_wplan.assign(eng->mmt_wplan)) || (rc = d.mmt_cidx.assign(eng->mmt_cidx)))
            return rc;
        break;
    case MdpPath::WideHs:
        if ((rc = d.hs_kt.assign(eng->hs_kt)) || (rc = d.hs_cidx.assign(eng->hs_cidx)) ||
            (rc = d.hs_pbase.assign(eng->hs_pbase)) || (rc = d.hs_ppos.assign(eng->hs_ppos)) ||
            (rc = d.hs_dpos.assign(eng->hs_dpos)) || (rc = d.hs_dbase.assign(eng->hs_dbase)) ||
            (rc = d.hs_pk.assign(eng->hs_pk)) ||
            (rc = d.hs_wplan.assign(eng->hs_wplan)) || (rc = d.hs_pass.assign(eng->hs_pass)) ||
            (rc = d.hs_dpk.assign(eng->hs_dpk)))
            return rc;
        break;
    default: break;  // (k_fwd_wide reads the tables above)
    }
    return wide_lds_limits(eng);
}

// k_qrows may take more than 64 KB of dynamic LDS: raise its limit once per
// device, just before its first launch
int qrows_attrs(const mdp_engine *eng, DevCtx &d)
{
    if (d.qrows_attr_set) return MDP_OK;
    const size_t lds_max = qrows_lds(eng, kQrowsMaxC);
    if (lds_max > 64 * 1024)
        for (uint32_t cb = 1; cb <= kQrowsMaxC; cb *= 2)  // every instantiation a grid of this engine may run
            if (int rc = for_qrows(eng, cb, [&](auto nv, auto ex, auto c) {
                    return set_lds_limit(k_qrows<nv(), ex(), c()>, std::min(lds_max, kQrowsLdsMax));
                }))
                return rc;
    d.qrows_attr_set = true;
    return MDP_OK;
}

// A new grid: plan it on the host (mdp_plan_grid: the refusals, the kernel
// variant, the point list, the chunk widths, every buffer size), then grow
// and upload what the plan says and load the forward kernel it names.  The
// uploads are synchronous copies and a memset on the null stream, which
// nothing orders against a caller's non-blocking stream: a mdp_engine_run
// still pending there is waited for first (settle), or it would read this
// grid's axes, point list and tables.
int set_grid_dev(mdp_engine *eng, DevCtx &d, const double *e, uint32_t ne, const double *c,
                 uint32_t nc)
{
    HIP_TRY(hipSetDevice(d.device));
    if (int prc = d.settle()) return prc;
    if (!d.ncu && path_is_jit(eng->path)) {
        int v = 0;
        d.ncu = hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, d.device) == hipSuccess && v > 0
                    ? (uint32_t)v : 256u;
    }
    MdpGridPlan g;
    int rc = mdp_plan_grid(eng, d.ct, e, ne, c, nc, d.ncu, g);
    if (g.tables_new) {  // (also when the plan then refused the grid: d.ct holds the new bound)
        const int urc = upload_ctables(d);
        if (urc) {
            d.ct.cmax = -1.0;  // nothing usable on the device: the next grid builds them again
            return urc;
        }
    }
    if (rc) return rc;
    if ((rc = d.e.assign(e, ne)) || (rc = d.c.assign(c, nc)) || (g.n_qrow && (rc = d.Qrow.grow(g.n_qrow))) ||
        (g.n_zg && (rc = d.Zg.grow(g.n_zg))) || (g.n_pg && (rc = d.Pg.grow(g.n_pg))) || (g.n_v && (rc = d.V.grow(g.n_v))) ||
        (g.n_vscr && (rc = d.vscr.grow(g.n_vscr))) || (g.n_zpv && (rc = d.ZPV.grow(g.n_zpv))) ||
        (g.n_r && (rc = d.R.grow(g.n_r))) || (g.n_gpart && (rc = d.gpart.grow(g.n_gpart))))
        return rc;
    if (g.pg_zero && g.n_pg) HIP_TRY(hipMemset(d.Pg.get(), 0, g.n_pg * sizeof(double)));
    if (g.zrows_lds > 64 * 1024 && (rc = set_lds_limit(k_zrows, g.zrows_lds))) return rc;
    if (!g.plist_identity && ((rc = d.plist.assign(g.plist)) || (rc = d.elist.assign(g.elist)))) return rc;
    if (path_is_jit(eng->path)) {
        if ((rc = jit_load(eng, d, g.variant))) return rc;
        mdp_plan_fwd_launch(eng, d.ct, ne, nc, g);  // (the variant's shape is settled once it is built)
    }
    for (int k = 0; k < 3 && eng->diag; ++k) {
        if ((rc = d.stamps[k].grow(g.nst[k] * kStampSlots))) return rc;
        HIP_TRY(hipMemset(d.stamps[k].get(), 0, d.stamps[k].cap() * sizeof(unsigned long long)));
    }
    d.ne = ne;
    d.nc = nc;
    d.plan = std::move(g);
    return MDP_OK;
}

template <int NP, int DEG, int EPL>
void launch_fwd_epl(const mdp_engine *eng, const DevCtx &d, double *out, OutStrides os, hipStream_t s)
{
    uint32_t se = os.se, sc = os.sc;
    dim3 grid(d.nc, (d.ne + kBlock * EPL - 1) / (kBlock * EPL));
    const uint32_t nprog = (uint32_t)eng->prog.size() - 1;
    note_launch(eng, d, "%s<%d,%d,%d>", eng->fwd_lds ? "k_forward_lds" : "k_forward", NP, DEG, EPL);
    if (eng->fwd_lds)
        MDP_LAUNCH((k_forward_lds<NP, DEG, EPL>), grid, dim3(kBlock), eng->fwd_lds_bytes, s,
                           d.R.get(), ldR_of(eng), d.prog.get(), nprog, eng->np[0], eng->prior0, d.e.get(), d.ne, out, se,
                           sc, d.stamps[2].get());
    else
        MDP_LAUNCH((k_forward<NP, DEG, EPL>), grid, dim3(kBlock), 0, s, d.R.get(), ldR_of(eng),
                           d.prog.get(), nprog, eng->np[0], eng->prior0, d.e.get(), d.ne, out, se, sc);
}

template <int NP, int DEG>
void launch_fwd(const mdp_engine *eng, const DevCtx &d, double *out, OutStrides os, hipStream_t s)
{
    if constexpr (NP <= 4 && DEG <= 8) {
        if (eng->epl == 1) return launch_fwd_epl<NP, DEG, 1>(eng, d, out, os, s);
        if (eng->epl == 4) return launch_fwd_epl<NP, DEG, 4>(eng, d, out, os, s);
    }
    launch_fwd_epl<NP, DEG, kEPL>(eng, d, out, os, s);
}

template <int NP>
int launch_fwd_deg(const mdp_engine *eng, const DevCtx &d, double *out, OutStrides os, hipStream_t s)
{
    switch (eng->deg) {
    case 4: launch_fwd<NP, 4>(eng, d, out, os, s); break;
    case 8: launch_fwd<NP, 8>(eng, d, out, os, s); break;
    case 16: launch_fwd<NP, 16>(eng, d, out, os, s); break;
    case 24: launch_fwd<NP, 24>(eng, d, out, os, s); break;
    default: return mdp_set_error(MDP_EUNSUPPORTED, "no forward kernel for degree %u", eng->deg);
    }
    return MDP_OK;
}

// Slot 2 of the direct paths: the specialised forward kernel (a long series:
// its chunk kernels)
int launch_fwd_jit(const mdp_engine *eng, const DevCtx &d, double *out, OutStrides os, hipStream_t s)
{
    // the launch as the grid plan shaped it (mdp_plan_fwd_launch)
    const MdpGridPlan &g = d.plan;
    if (g.fwd_threads > 0xffffffffull)
        return mdp_set_error(MDP_EUNSUPPORTED, "grid %u x %u too large", d.ne, d.nc);
    const uint32_t nthreads = (uint32_t)(g.fwd_threads * g.fwd_pro);
    // mdp_fwd_jit's parameters (spom_jit.h declares them once, for the
    // generated signature and for this struct)
    MdpFwdJitArgs a;
    a.tab = g.fused ? d.coltab.get() : d.Qrow.get();  // the table the variant stages first
    a.cvals = d.c.get();
    a.evals = g.fwd_listed ? d.elist.get() : d.e.get();  // a listed kernel reads e by list position
    a.ct_len = d.ct.ct_len;
    a.nlist = g.fwd_nlist;
    a.ne = d.ne;
    a.nc = d.nc;
    a.plist = g.fwd_listed ? d.plist.get() : nullptr;
    a.nblk = (uint32_t)g.fwd_nblk;
    a.kmax = d.ct.kmax;
    a.one = 1;
    a.out = out;
    a.ld_out = os.se;
    a.out_cs = os.sc;
    a.prior0 = eng->prior0;
    a.vscr = d.vscr.get();
    a.ldv = g.ldv;
    a.stamps = d.stamps[2].get();
    auto args = a.params();
    static_assert(std::tuple_size<decltype(args)>::value == 19, "one kernelParams entry per parameter of mdp_fwd_jit");
    if (g.step[2] == MdpStep::FwdJitChunks) {  // a long series: its chunks in order on the stream
        const size_t nch = d.cfn.size();
        if (nch != eng->chunks.size() || d.cqidx.size() != nch)
            return mdp_set_error(MDP_EHIP, "forward chunks not loaded (%zu of %zu)", nch, eng->chunks.size());
        for (size_t i = 0; i < nch; ++i) {
            a.qidx = d.cqidx[i].get();  // the chunk's gather list (args points at the member)
            HIP_TRY(hipExtModuleLaunchKernel(d.cfn[i], nthreads, 1, 1, g.fwd_block, 1, 1, 0, s,
                                             args.data(), nullptr, i == 0 ? t_kev.start : nullptr,
                                             i + 1 == nch ? t_kev.stop : nullptr, 0));
        }
        note_launch(eng, d, kFmtJitChunks, eng->maxA, nch,
                    eng->chunks[0].qidx.empty() ? "" : ",gather");
        return MDP_OK;
    }
    HIP_TRY(hipExtModuleLaunchKernel(d.jit_fn[g.variant], nthreads, 1, 1, g.fwd_block, 1, 1, g.fwd_lds, s, args.data(),
                                     nullptr, t_kev.start, t_kev.stop, 0));
    note_launch(eng, d, kFmtJit, g.fused ? "fused" : "reading", eng->maxA);
    if (g.tall) note_launch(eng, d, kFmtJitTall, kJitKblockTall);
    return MDP_OK;
}

// Slot 2 of the generic path
int launch_fwd_generic(const mdp_engine *eng, const DevCtx &d, double *out, OutStrides os, hipStream_t s)
{
    int rc;
    switch (eng->variant / 100) {
    case 1: rc = launch_fwd_deg<1>(eng, d, out, os, s); break;
    case 2: rc = launch_fwd_deg<2>(eng, d, out, os, s); break;
    case 4: rc = launch_fwd_deg<4>(eng, d, out, os, s); break;
    case 8: rc = launch_fwd_deg<8>(eng, d, out, os, s); break;
    case 16: rc = launch_fwd_deg<16>(eng, d, out, os, s); break;
    default: return mdp_set_error(MDP_EUNSUPPORTED, "no forward kernel variant %u", eng->variant);
    }
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return MDP_OK;
}

int launch_coefs(const mdp_engine *eng, const DevCtx &d, hipStream_t s)
{
    for_coefs(eng, [&](auto ldsz, auto ldsp, auto nv) {
        note_launch(eng, d, kFmtCoefs, (int)ldsz(), (int)ldsp(), nv());
        MDP_LAUNCH((k_coefs<ldsz(), ldsp(), nv()>), dim3(d.nc), dim3(kBlock), eng->coef_lds, s, d.ZPV.get(), eng->nstates,
                   eng->nvar, d.pairA.get(), d.pairB.get(), d.pairOff.get(), d.pairPart0.get(), eng->npairs, d.partP.get(),
                   d.partK0.get(), (uint32_t)eng->partP.size(), eng->ncoef, d.udesc.get(), eng->nuses, eng->deg, d.R.get(),
                   ldR_of(eng), d.gpart.get(), d.stamps[1].get());
    });
    HIP_TRY(hipGetLastError());
    return MDP_OK;
}

// k_witems: the item factors of n c values from c0, in Pg rows of ldp
void launch_witems(const mdp_engine *eng, const DevCtx &d, uint32_t c0, uint32_t n, uint32_t ldp, hipStream_t s)
{
    const dim3 gi((eng->nitems + kBlock - 1) / kBlock, n);
    for_nv(eng, [&](auto nv) {
        note_launch(eng, d, kFmtWitems, nv());
        hipLaunchKernelGGL((k_witems<nv()>), gi, dim3(kBlock), 0, s, d.c.get(), d.nc, c0, eng->nvar, d.Zg.get(), d.sv.get(),
                           eng->nitems, d.items.get(), d.Pg.get(), ldp);
    });
}

// A slot of several launches (the Q-global paths' chunks of c values).  A
// profiled run times the slot as a whole: events recorded around its launches.
template <typename F>
int launch_bracketed(hipStream_t s, F &&launches)
{
    const KernelEvents ev = t_kev;
    t_kev = KernelEvents{};
    if (ev.start) HIP_TRY(hipEventRecord(ev.start, s));
    if (int rc = launches()) return rc;
    HIP_TRY(hipGetLastError());
    if (ev.stop) HIP_TRY(hipEventRecord(ev.stop, s));
    return MDP_OK;
}

// What slot k of the grid runs (MdpGridPlan::step, mdp_plan_steps): one case
// per step, none left to a default.
int launch_slot(mdp_engine *eng, DevCtx &d, int k, double *out, OutStrides os, hipStream_t s)
{
    switch (d.plan.step[k]) {
    case MdpStep::None: return MDP_OK;
    case MdpStep::Zpv: {
        dim3 grid((eng->nstates + kZpvJ - 1) / kZpvJ, (d.nc + kZpvCT - 1) / kZpvCT);
        note_launch(eng, d, "k_zpv");
        MDP_LAUNCH(k_zpv, grid, dim3(kBlock), 0, s, d.S.get(), eng->nstates, eng->n - eng->nvar, eng->nvar, d.c.get(),
                   d.nc, d.ZPV.get(), d.stamps[0].get());
        HIP_TRY(hipGetLastError());
        return MDP_OK;
    }
    case MdpStep::Coefs: return launch_coefs(eng, d, s);
    case MdpStep::FwdGeneric: return launch_fwd_generic(eng, d, out, os, s);
    case MdpStep::Zrows: {
        const uint32_t kmax = d.ct.kmax;
        const dim3 grid((d.nc + 64 * kZC - 1) / (64 * kZC), (eng->nj + kZRows - 1) / kZRows);
        note_launch(eng, d, "k_zrows");
        MDP_LAUNCH(k_zrows, grid, dim3(kBlock), (size_t)kZRows * kmax * sizeof(double), s, d.c.get(), d.nc, eng->nj,
                   kmax, d.zs.get(), d.zc.get(), d.Zg.get());
        HIP_TRY(hipGetLastError());
        return MDP_OK;
    }
    case MdpStep::Qrows: {
        if (int rc = qrows_attrs(eng, d)) return rc;
        const uint32_t cb = d.plan.qrows_cb;
        const dim3 grid((d.nc + cb - 1) / cb);
        const size_t lds = qrows_lds(eng, cb);
        for_qrows(eng, cb, [&](auto nv, auto ex, auto CB) {
            note_launch(eng, d, kFmtQrows, nv(), (int)ex(), CB());
            MDP_LAUNCH((k_qrows<nv(), ex(), CB()>), grid, dim3(kQrowsBlock), lds, s, d.c.get(), d.nc, eng->nvar, eng->nj,
                       d.ct.kmax, d.zsq.get(), d.zc.get(), d.sv.get(), eng->nitems, d.items.get(), eng->ncoef_d, d.qstart.get(),
                       (uint32_t)eng->qitem.size(), d.qitem.get(), d.Qrow.get(), (uint32_t)eng->ldQ, d.stamps[1].get(),
                       (uint32_t)(eng->qrows_xcd ? 1u : 0u), d.qslot.get(), (uint32_t)eng->qslot.size(), eng->qslot_lglmax,
                       (const uint4 *)d.qlane.get(), d.islot.get(), eng->npl_slots);
        });
        HIP_TRY(hipGetLastError());
        return MDP_OK;
    }
    case MdpStep::ItemsQ:  // k_witems + k_wq per chunk of c values
        return launch_bracketed(s, [&]() {
            const uint32_t cb = d.plan.wide_cb_items;
            for (uint32_t c0 = 0; c0 < d.nc; c0 += cb) {
                const uint32_t n = std::min(cb, d.nc - c0);
                launch_witems(eng, d, c0, n, eng->nitems, s);
                const dim3 gq((uint32_t)((eng->ldQ + kBlock - 1) / kBlock), n);
                note_launch(eng, d, "k_wq");
                hipLaunchKernelGGL(k_wq, gq, dim3(kBlock), 0, s, c0, eng->nitems, d.Pg.get(), eng->ncoef_d, d.qstart.get(),
                                   d.qitem.get(), d.Qrow.get(), (uint32_t)eng->ldQ);
            }
            return MDP_OK;
        });
    case MdpStep::ItemsAll:  // k_fwd_hs: the item factors of every column when they fit one Pg block (kHsPgBytes), else nothing
        return launch_bracketed(s, [&]() {
            if (d.plan.wide_cb_items >= d.nc) launch_witems(eng, d, 0, d.nc, eng->nitems + 1, s);
            return MDP_OK;
        });
    case MdpStep::FwdJit:
    case MdpStep::FwdJitChunks: return launch_fwd_jit(eng, d, out, os, s);
    case MdpStep::FwdHs:  // k_fwd_hs, or per column chunk k_witems then k_fwd_hs
        return launch_bracketed(s, [&]() {
            const uint32_t cb = d.plan.wide_cb_items, ldp = eng->nitems + 1;
            const bool one = cb >= d.nc;
            const uint32_t rt = eng->hs_rt, nb = eng->hs_nb, npb = (d.ne + mmt_pts(rt) - 1) / mmt_pts(rt);
            for (uint32_t c0 = 0; c0 < d.nc; c0 += cb) {
                const uint32_t n = std::min(cb, d.nc - c0);
                if (!one && eng->nitems) launch_witems(eng, d, c0, n, ldp, s);
                const uint64_t nbk = (uint64_t)npb * n;
                if (nbk > 0x7fffffffull) return mdp_set_error(MDP_EUNSUPPORTED, "grid of %llu k_fwd_hs workgroups", (unsigned long long)nbk);
                note_launch(eng, d, kFmtHs, rt, nb);
                for_hs(eng, [&](auto RT, auto NB, auto NW) {
                    hipLaunchKernelGGL((k_fwd_hs<RT(), NB(), NW()>), dim3((uint32_t)nbk), dim3(NW() * 64), hs_lds(eng), s,
                                       d.Pg.get(), ldp, c0, d.np_d.get(), d.hs_kt.get(), d.hs_cidx.get(), d.hs_wplan.get(),
                                       d.hs_pass.get(), d.hs_pbase.get(), d.hs_ppos.get(), d.hs_dpos.get(), d.hs_dbase.get(),
                                       d.hs_dpk.get(), d.hs_pk.get(), eng->tmax, eng->prior0, d.e.get(),
                                       d.ne, out, os.se, os.sc, eng->hs_probe);
                });
            }
            return MDP_OK;
        });
    case MdpStep::FwdMmt:  // the matrix-core forward: every c in one launch, blocks dealt XCD-aware
        return launch_bracketed(s, [&]() {
            const uint32_t rt = eng->mmt_rt, rows = eng->mmt_rows, npb = (d.ne + mmt_pts(rt) - 1) / mmt_pts(rt);
            const bool db = mmt_shape(eng).db;
            const uint64_t nb = (uint64_t)npb * d.nc;
            if (nb > 0x7fffffffull) return mdp_set_error(MDP_EUNSUPPORTED, "grid of %llu k_fwd_mmt workgroups", (unsigned long long)nb);
            note_launch(eng, d, kFmtMmt, rt, rows, db ? "2buf" : "1buf");
            for_mmt(eng, [&](auto RT, auto ROWS, auto DB) {
                hipLaunchKernelGGL((k_fwd_mmt<RT(), ROWS(), DB()>), dim3((uint32_t)nb), dim3(kMmaThreads), mmt_lds(eng), s,
                                   d.Qrow.get(), (uint32_t)eng->ldQ, d.np_d.get(), d.mmt_kt.get(), d.mmt_cidx.get(), d.mmt_ktile.get(),
                                   d.mmt_wplan.get(), eng->tmax, eng->prior0, d.e.get(), d.ne, eng->maxA, out, os.se, os.sc);
            });
            return MDP_OK;
        });
    case MdpStep::FwdMma:  // round 5's matrix-core forward (MDP_WIDE_MMA=1; years of up to 256 states)
        return launch_bracketed(s, [&]() {
            uint32_t se = os.se, sc = os.sc;
            for (uint32_t c0 = 0; c0 < d.nc; c0 += 65535) {
                const uint32_t n = std::min(65535u, d.nc - c0);
                const uint32_t pts = mma_pts(eng->mma_npm);
                const dim3 g((d.ne + pts - 1) / pts, n);
                note_launch(eng, d, kFmtMma, eng->mma_npm);
                for_mma(eng, [&](auto NPM) {
                    hipLaunchKernelGGL((k_fwd_mma<NPM()>), g, dim3(kMmaThreads), mma_lds(eng), s, d.Qrow.get(), (uint32_t)eng->ldQ,
                                       d.np_d.get(), d.mma_kt.get(), d.mma_kbase.get(), d.mma_desc.get(), d.mma_dbase.get(),
                                       d.mma_wplan.get(), eng->tmax, eng->prior0, d.e.get(), d.ne, c0, eng->maxA, eng->mma_ktmax,
                                       eng->ncoef_d, out, se, sc);
                });
            }
            return MDP_OK;
        });
    case MdpStep::FwdPlain:  // k_fwd_wide per chunk of c values
        return launch_bracketed(s, [&]() {
            const uint32_t cb = d.plan.wide_cb_fwd;
            uint32_t se = os.se, sc = os.sc;
            for (uint32_t c0 = 0; c0 < d.nc; c0 += cb) {
                const uint32_t n = std::min(cb, d.nc - c0);
                const dim3 g((d.ne + kBlock - 1) / kBlock, n);
                note_launch(eng, d, "k_fwd_wide");
                hipLaunchKernelGGL(k_fwd_wide, g, dim3(kBlock), wide_lds(eng), s, d.Qrow.get(), (uint32_t)eng->ldQ, d.udesc_w.get(),
                                   d.np_d.get(), eng->tmax, eng->prior0, d.e.get(), d.ne, c0, eng->maxA, d.V.get(), eng->npmax, out, se,
                                   sc);
            }
            return MDP_OK;
        });
    }
    return MDP_OK;  // (not reached: every step returns above)
}

int run_dev(mdp_engine *eng, DevCtx &d, double *out, OutStrides os, hipStream_t s)
{
    HIP_TRY(hipSetDevice(d.device));
    if (d.ne == 0 || d.nc == 0) return MDP_OK;
    if ((d.ne + kBlock - 1) / kBlock > 65535u || d.nc > 0x7fffffffu)
        return mdp_set_error(MDP_EUNSUPPORTED, "grid %u x %u too large", d.ne, d.nc);
    const bool prof = eng->profiling != 0;
    hipEvent_t *ev = nullptr;
    if (prof) {
        if ((d.ev_used + 1) * kNumEv > d.ev.size()) {
            for (int i = 0; i < kNumEv; ++i) {
                hipEvent_t x;
                HIP_TRY(hipEventCreate(&x));
                d.ev.push_back(x);
            }
        }
        ev = &d.ev[d.ev_used * kNumEv];
        ++d.ev_used;
        d.ev_mask.resize(d.ev_used);
        d.ev_mask.back() = 0;
    }
    struct Reset {
        ~Reset() { t_kev = KernelEvents{}; }
    } reset;
    for (int k = 0; k < 3; ++k) {
        if (d.plan.step[k] == MdpStep::None) continue;
        // only launched kernels carry events (no marker packets between kernels)
        t_kev = prof ? KernelEvents{ev[2 * k], ev[2 * k + 1]} : KernelEvents{};
        if (prof) d.ev_mask.back() |= (uint8_t)(1u << k);
        int rc = launch_slot(eng, d, k, out, os, s);
        if (rc) return rc;
    }
    return MDP_OK;
}

// Mean duration of each kernel of the run: one full run, then every kernel
// launched `reps` times back to back between two events on the stream (no
// per-launch events, so the figure is the kernel's own, as rocprofv3 sees it).
int time_kernels(mdp_engine *eng, DevCtx &d, double *out, OutStrides os, hipStream_t s, int reps, double *ms)
{
    int rc = run_dev(eng, d, out, os, s);
    if (rc) return rc;
    hipEvent_t a, b;
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    for (int k = 0; k < 3; ++k) {
        ms[k] = 0.0;
        if (d.plan.step[k] == MdpStep::None) continue;
        if ((rc = launch_slot(eng, d, k, out, os, s))) break;  // warm
        (void)hipEventRecord(a, s);
        for (int r = 0; r < reps && !rc; ++r) rc = launch_slot(eng, d, k, out, os, s);
        (void)hipEventRecord(b, s);
        if (rc) break;
        float t = 0;
        (void)hipEventSynchronize(b);
        (void)hipEventElapsedTime(&t, a, b);
        ms[k] = t / reps;
    }
    // leave the output as a full run computes it
    if (!rc) rc = run_dev(eng, d, out, os, s);
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return rc;
}

// A device form on the caller's stream st (spom_dev.h, the stream rule): a run
// still pending on another stream shares this one's scratch (Q rows, Z, the
// wide path's state vectors) and is waited for; on the same stream the stream
// orders them.  Whatever `launch` queued is noted as pending, after an error
// too.  No HIP call when nothing is pending elsewhere.
template <typename F>
int run_pending(DevCtx &d, hipStream_t st, F launch)
{
    if (d.pending && d.pending_on != st) {
        HIP_TRY(hipSetDevice(d.device));
        if (int rc = d.settle()) return rc;
    }
    d.launched_on(st);
    return launch();
}

// Mean kernel durations over every profiled run since the last collect.
int collect_times(mdp_engine *eng, DevCtx &d)
{
    if (d.ev_used == 0) return MDP_OK;
    HIP_TRY(hipSetDevice(d.device));
    HIP_TRY(hipEventSynchronize(d.ev[(d.ev_used - 1) * kNumEv + kNumEv - 1]));
    double sum[3] = {0, 0, 0};
    size_t cnt[3] = {0, 0, 0};
    for (size_t r = 0; r < d.ev_used; ++r)
        for (int k = 0; k < 3; ++k) {
            if (!((d.ev_mask[r] >> k) & 1u)) continue;
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, d.ev[r * kNumEv + 2 * k], d.ev[r * kNumEv + 2 * k + 1]));
            sum[k] += ms;
            ++cnt[k];
        }
    for (int k = 0; k < 3; ++k) eng->last_ms[k] = cnt[k] ? sum[k] / (double)cnt[k] : 0.0;
    eng->nlast = 3;
    eng->runs_collected = d.ev_used;
    d.ev_used = 0;
    return MDP_OK;
}

}  // namespace

extern "C" {

int mdp_engine_create(const mdp_problem *p, const int *devices, int n_devices, mdp_engine **out)
{
    return mdp_engine_create_opts(p, devices, n_devices, nullptr, out);
}

int mdp_engine_create_opts(const mdp_problem *p, const int *devices, int n_devices, const char *options,
                           mdp_engine **out)
{
    if (!p || !out || n_devices < 0) return mdp_set_error(MDP_EINVAL, "null argument");
    *out = nullptr;
    // MDP_SETUP_TIMING=1: the set-up's split on stderr (planning, hipRTC /
    // code-object cache, device set-up)
    const bool st_on = getenv("MDP_SETUP_TIMING") && atoi(getenv("MDP_SETUP_TIMING")) != 0;
    auto st_now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double st0 = st_now();
    double st_jit[2] = {st0, st0};  // around the hipRTC step (mdp_plan_engine)
    MdpOpts opts;
    if (int orc = parse_engine_opts(options, opts, kDiagBuild)) return orc;
    if (p->n == 0 || p->tmax == 0 || !p->M || !p->year_off || !p->year_ids || !p->prior ||
        !p->short_state || (p->nvar && !p->var_cols))
        return mdp_set_error(MDP_EINVAL, "incomplete problem description");
    int ndev = 0;
    // MDP_JIT_CHECK=1 without a device: plan and compile both forward
    // variants (hipRTC runs offline), then report MDP_ENODEV -- the CPU
    // test that the generated sources compile for gfx950
    const bool jit_check = opts.jit_check;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        ndev = 0;
        if (!jit_check) return mdp_set_error(MDP_ENODEV, "no HIP device available");
    }
    mdp_engine *eng = new (std::nothrow) mdp_engine();
    if (!eng) return mdp_set_error(MDP_ENOMEM, "out of host memory");
    eng->opts = std::move(opts);
    const bool offline_check = jit_check && ndev == 0;
    int rc = mdp_plan_engine(eng, p, device_lds_max(), offline_check ? MdpPlanMode::OfflineCheck : MdpPlanMode::Compile,
                             st_jit);
    if (rc) {
        delete eng;
        return rc;
    }
    std::vector<int> ids;
    if (n_devices == 0) {
        int cur = 0;
        (void)hipGetDevice(&cur);
        ids.push_back(cur);
    } else {
        for (int i = 0; i < n_devices; ++i) ids.push_back(devices ? devices[i] : i);
    }
    for (int id : ids)
        if (id < 0 || id >= ndev) {
            delete eng;
            return mdp_set_error(MDP_ENODEV, "device %d not present (%d visible)", id, ndev);
        }
    eng->devs = std::vector<DevCtx>(ids.size());  // at its final size: a context is neither copied nor moved
    const double st_dev0 = st_now();
    for (size_t i = 0; i < ids.size(); ++i) {
        eng->devs[i].device = ids[i];
        rc = init_device(eng, eng->devs[i], p);
        if (rc) {
            delete eng;
            return rc;
        }
    }
    if (st_on)
        fprintf(stderr, "mdp setup (s): plan %.3f jit %.3f plan2 %.3f devices %.3f\n", st_jit[0] - st0, st_jit[1] - st_jit[0],
                st_dev0 - st_jit[1], st_now() - st_dev0);
    *out = eng;
    return MDP_OK;
}

void mdp_engine_destroy(mdp_engine *eng)
{
    delete eng;  // (every device context releases its own: ~DevCtx)
}

int mdp_engine_set_grid(mdp_engine *eng, const double *e, uint32_t ne, const double *c, uint32_t nc)
{
    if (!eng || (ne && !e) || (nc && !c)) return mdp_set_error(MDP_EINVAL, "null argument");
    if (eng->devs.size() != 1)
        return mdp_set_error(MDP_EINVAL, "mdp_engine_set_grid needs a single-device engine");
    return set_grid_dev(eng, eng->devs[0], e, ne, c, nc);
}

int mdp_engine_set_cbound(mdp_engine *eng, double cbound)
{
    if (!eng) return mdp_set_error(MDP_EINVAL, "null argument");
    if (!(cbound >= 0.0) || std::isinf(cbound)) return mdp_set_error(MDP_EINVAL, "cbound %g (want a finite value >= 0)", cbound);
    eng->cbound = cbound;
    return MDP_OK;
}

int mdp_engine_set_layout(mdp_engine *eng, int layout)
{
    if (!eng) return mdp_set_error(MDP_EINVAL, "null argument");
    if (layout != MDP_LAYOUT_EC && layout != MDP_LAYOUT_CE) return mdp_set_error(MDP_EINVAL, "unknown layout %d", layout);
    eng->layout = layout;
    return MDP_OK;
}

int mdp_engine_run(mdp_engine *eng, double *d_out, uint32_t ld_out, void *stream)
{
    if (!eng || !d_out) return mdp_set_error(MDP_EINVAL, "null argument");
    if (eng->devs.size() != 1)
        return mdp_set_error(MDP_EINVAL, "mdp_engine_run needs a single-device engine");
    DevCtx &d = eng->devs[0];
    if (eng->layout == MDP_LAYOUT_CE ? ld_out < d.ne : ld_out < d.nc)
        return mdp_set_error(MDP_EINVAL, "ld_out %u < %s %u", ld_out, eng->layout == MDP_LAYOUT_CE ? "ne" : "nc",
                             eng->layout == MDP_LAYOUT_CE ? d.ne : d.nc);
    // the caller's stream as given: NULL is HIP's null stream (torch's default
    // stream), never the engine's private non-blocking stream
    return run_pending(d, (hipStream_t)stream, [&]() {
        return run_dev(eng, d, d_out, layout_strides(eng->layout, ld_out), (hipStream_t)stream);
    });
}

int mdp_loglik_grid(mdp_engine *eng, const double *e, uint32_t ne, const double *c, uint32_t nc,
                    double *out)
{
    return mdp_loglik_grid_layout(eng, e, ne, c, nc, MDP_LAYOUT_EC, out);
}

int mdp_loglik_grid_layout(mdp_engine *eng, const double *e, uint32_t ne, const double *c, uint32_t nc, int layout,
                           double *out)
{
    if (!eng || !out || (ne && !e) || (nc && !c)) return mdp_set_error(MDP_EINVAL, "null argument");
    if (layout != MDP_LAYOUT_EC && layout != MDP_LAYOUT_CE) return mdp_set_error(MDP_EINVAL, "unknown layout %d", layout);
    const bool ce = layout == MDP_LAYOUT_CE;
    const uint32_t nd = (uint32_t)eng->devs.size();
    const uint32_t avg = ne / nd, rem = ne % nd;
    std::vector<uint32_t> r0(nd), r1(nd);
    int rc;
    for (uint32_t r = 0; r < nd; ++r) {
        r0[r] = r == 0 ? 0 : r * avg + rem;
        r1[r] = (r + 1) * avg + rem;
        DevCtx &d = eng->devs[r];
        const uint32_t rows = r1[r] - r0[r];
        if ((rc = set_grid_dev(eng, d, e + r0[r], rows, c, nc))) return rc;
        if ((rc = d.out.grow((size_t)rows * nc))) return rc;
        // the layout asked of this call (not the engine's mdp_engine_run
        // layout): the slab [e][c] (ld nc) or [c][e] (ld = the slab's rows)
        if ((rc = run_dev(eng, d, d.out.get(), ce ? OutStrides{1u, rows} : OutStrides{nc, 1u}, d.stream))) return rc;
    }
    for (uint32_t r = 0; r < nd; ++r) {
        DevCtx &d = eng->devs[r];
        const uint32_t rows = r1[r] - r0[r];
        HIP_TRY(hipSetDevice(d.device));
        if (rows && !ce)
            HIP_TRY(hipMemcpyAsync(out + (size_t)r0[r] * nc, d.out.get(), (size_t)rows * nc * sizeof(double),
                                   hipMemcpyDeviceToHost, d.stream));
        else if (rows && nc)  // the slab's columns into out[c][e] at e offset r0
            HIP_TRY(hipMemcpy2DAsync(out + r0[r], (size_t)ne * sizeof(double), d.out.get(), (size_t)rows * sizeof(double),
                                     (size_t)rows * sizeof(double), nc, hipMemcpyDeviceToHost, d.stream));
    }
    for (uint32_t r = 0; r < nd; ++r) {
        HIP_TRY(hipSetDevice(eng->devs[r].device));
        HIP_TRY(hipStreamSynchronize(eng->devs[r].stream));
    }
    for (uint32_t r = nd; r-- > 0;)  // device 0 last: its means are reported
        if ((rc = collect_times(eng, eng->devs[r]))) return rc;
    return MDP_OK;
}

int mdp_engine_diag_report(mdp_engine *eng, char *buf, size_t len)
{
    if (!eng || !buf || !len) return mdp_set_error(MDP_EINVAL, "null argument");
    buf[0] = 0;
    if (!eng->diag || eng->devs.empty()) return 0;
    DevCtx &d = eng->devs[0];
    HIP_TRY(hipSetDevice(d.device));
    HIP_TRY(hipDeviceSynchronize());
    const char *names[3] = {"k_zpv", "k_coefs", "k_forward_lds"};
    int slots[3] = {3, 5, 3};
    const bool jit = path_is_jit(eng->path);
    if (jit) {  // direct path: k_qrows and the hipRTC forward kernel
        names[1] = "k_qrows";
        names[2] = "k_forward(jit)";
        slots[0] = 0;
        slots[1] = 6;  // k_qrows stamps slots 4 and 5 inside phase 1
        slots[2] = d.plan.fused ? 6 : 4;
    }
    size_t used = 0;
    for (int k = 0; k < 3; ++k) {
        if (d.stamps[k].empty() || !d.plan.nst[k] || !slots[k]) continue;
        std::vector<unsigned long long> h(d.plan.nst[k] * kStampSlots);
        HIP_TRY(hipMemcpy(h.data(), d.stamps[k].get(), h.size() * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost));
        unsigned long long t0 = ~0ull, t1 = 0, rs0 = ~0ull, rs1 = 0, re1 = 0;
        double rdur = 0.0;
        std::vector<double> mean(slots[k], 0.0);
        size_t nb = 0;
        for (size_t b = 0; b < d.plan.nst[k]; ++b) {
            const unsigned long long *st = &h[b * kStampSlots];
            const int last = ((k == 2 && d.plan.fused) || k == 1) && jit ? 3 : slots[k] - 1;
            if (!st[0] || !st[last] || st[last] < st[0]) continue;
            ++nb;
            rs0 = std::min(rs0, st[6]);
            rs1 = std::max(rs1, st[6]);
            re1 = std::max(re1, st[7]);
            rdur += (double)(st[7] - st[6]);
            t0 = std::min(t0, st[0]);
            t1 = std::max(t1, st[last]);
            // the fused forward kernel stamps slots 4 and 5 between 0 and 1
            const bool fz = ((k == 2 && d.plan.fused) || k == 1) && jit && slots[k] == 6;
            static const int seq_plain[6] = {0, 1, 2, 3, 4, 5}, seq_fused[6] = {0, 4, 5, 1, 2, 3};
            const int *seq = fz ? seq_fused : seq_plain;
            for (int q = 1; q < slots[k]; ++q) mean[q] += (double)(st[seq[q]] - st[seq[q - 1]]);
        }
        int w = snprintf(buf + used, len - used,
                         "%s: blocks=%zu wall_us=%.2f last_start_us=%.2f mean_block_us=%.2f cycles:",
                         names[k], nb, nb ? (re1 - rs0) * 0.01 : 0.0, nb ? (rs1 - rs0) * 0.01 : 0.0,
                         nb ? rdur / nb * 0.01 : 0.0);
        if (w > 0) used = std::min(len - 1, used + (size_t)w);
        for (int q = 1; q < slots[k]; ++q) {
            w = snprintf(buf + used, len - used, " ph%d=%.0f", q, nb ? mean[q] / nb : 0.0);
            if (w > 0) used = std::min(len - 1, used + (size_t)w);
        }
        {   // block start / end spread (wall clock): percentiles, and the latest start per XCD
            std::vector<double> st0, en;
            double xmax[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (size_t b = 0; b < d.plan.nst[k]; ++b) {
                const unsigned long long *st = &h[b * kStampSlots];
                if (!st[6] || !st[7] || st[7] < st[6] || st[6] < rs0) continue;
                st0.push_back((st[6] - rs0) * 0.01);
                en.push_back((st[7] - rs0) * 0.01);
                xmax[b % 8] = std::max(xmax[b % 8], (st[6] - rs0) * 0.01);
            }
            if (!st0.empty()) {
                std::sort(st0.begin(), st0.end());
                std::sort(en.begin(), en.end());
                auto pc = [](const std::vector<double> &v, double f) { return v[(size_t)(f * (v.size() - 1))]; };
                w = snprintf(buf + used, len - used,
                             " start_us p10=%.2f p50=%.2f p90=%.2f p99=%.2f end_us p1=%.2f p50=%.2f max=%.2f "
                             "xcd_last_start_us=%.2f,%.2f,%.2f,%.2f,%.2f,%.2f,%.2f,%.2f",
                             pc(st0, 0.1), pc(st0, 0.5), pc(st0, 0.9), pc(st0, 0.99), pc(en, 0.01), pc(en, 0.5),
                             en.back(), xmax[0], xmax[1], xmax[2], xmax[3], xmax[4], xmax[5], xmax[6], xmax[7]);
                if (w > 0) used = std::min(len - 1, used + (size_t)w);
            }
        }
        if (k == 2 && nb && !jit) {  // forward: cycles summed over run ops / general ops (wave 0)
            double cr = 0, cg = 0;
            for (size_t b = 0; b < d.plan.nst[k]; ++b) {
                const unsigned long long *st = &h[b * kStampSlots];
                if (!st[0] || !st[2]) continue;
                cr += (double)st[3];
                cg += (double)st[4];
            }
            w = snprintf(buf + used, len - used, " run_ops=%.0f general_ops=%.0f", cr / nb, cg / nb);
            if (w > 0) used = std::min(len - 1, used + (size_t)w);
        }
        w = snprintf(buf + used, len - used, "\n");
        if (w > 0) used = std::min(len - 1, used + (size_t)w);
        HIP_TRY(hipMemset(d.stamps[k].get(), 0, h.size() * sizeof(unsigned long long)));
    }
    return (int)used;
}

int mdp_engine_set_profiling(mdp_engine *eng, int enable)
{
    if (!eng) return mdp_set_error(MDP_EINVAL, "null engine");
    eng->profiling = enable;
    return MDP_OK;
}

int mdp_engine_time_kernels(mdp_engine *eng, double *d_out, uint32_t ld_out, void *stream, int reps,
                            double *ms, int max_k)
{
    if (!eng || !d_out || !ms || reps < 1) return mdp_set_error(MDP_EINVAL, "bad argument");
    if (eng->devs.size() != 1)
        return mdp_set_error(MDP_EINVAL, "mdp_engine_time_kernels needs a single-device engine");
    DevCtx &d = eng->devs[0];
    if (eng->layout == MDP_LAYOUT_CE ? ld_out < d.ne : ld_out < d.nc)
        return mdp_set_error(MDP_EINVAL, "ld_out %u < %s %u", ld_out, eng->layout == MDP_LAYOUT_CE ? "ne" : "nc",
                             eng->layout == MDP_LAYOUT_CE ? d.ne : d.nc);
    double t[3];
    const int saved = eng->profiling;
    eng->profiling = 0;
    int rc = run_pending(d, (hipStream_t)stream, [&]() {
        return time_kernels(eng, d, d_out, layout_strides(eng->layout, ld_out), (hipStream_t)stream, reps, t);
    });
    eng->profiling = saved;
    if (rc) return rc;
    const int k = std::min(max_k, 3);
    for (int i = 0; i < k; ++i) ms[i] = t[i];
    return k;
}

int mdp_engine_kernel_ms(mdp_engine *eng, double *ms, int max_k)
{
    if (!eng || !ms) return mdp_set_error(MDP_EINVAL, "null argument");
    if (!eng->devs.empty()) {
        int rc = collect_times(eng, eng->devs[0]);
        if (rc) return rc;
    }
    const int k = std::min(max_k, eng->nlast);
    for (int i = 0; i < k; ++i) ms[i] = eng->last_ms[i];
    return k;
}

const char *mdp_engine_kernel_name(const mdp_engine *eng, int k)
{
    if (!eng || k < 0 || k >= 3) return "";
    // the slot's step in the first context's grid plan (before a grid is set:
    // the one the path alone implies, init_device); an engine without a
    // device names what a fused grid would run
    MdpGridPlan g;
    g.fused = true;
    if (eng->devs.empty()) mdp_plan_steps(eng, g);
    switch (eng->devs.empty() ? g.step[k] : eng->devs[0].plan.step[k]) {
    case MdpStep::None: return "";
    case MdpStep::Zpv: return "k_zpv";
    case MdpStep::Coefs: return "k_coefs";
    case MdpStep::Zrows: return "k_zrows";
    case MdpStep::Qrows: return "k_qrows";
    case MdpStep::ItemsQ: return "k_witems+k_wq";
    case MdpStep::ItemsAll: return "k_witems";
    case MdpStep::FwdGeneric:
    case MdpStep::FwdJit:
    case MdpStep::FwdJitChunks: return "k_forward";
    case MdpStep::FwdHs: return "k_fwd_hs";
    case MdpStep::FwdMmt: return "k_fwd_mmt";
    case MdpStep::FwdMma: return "k_fwd_mma";
    case MdpStep::FwdPlain: return "k_fwd_wide";
    }
    return "";
}

int mdp_log_check(const double *x, double *y, size_t n)
{
    if ((n && (!x || !y))) return mdp_set_error(MDP_EINVAL, "null argument");
    if (!n) return MDP_OK;
    std::vector<char> code;
    std::string log;
    if (mdp_jit_compile(mdp_jit_log_source(), code, log) != 0)
        return mdp_set_error(MDP_EHIP, "hipRTC compilation of mdp_log failed: %s", log.c_str());
    hipModule_t mod = nullptr;
    hipFunction_t fn;
    DevBuf<double> dx, dy;
    int rc = MDP_OK;
    auto fail = [&](hipError_t e, const char *what) {
        rc = mdp_set_error(MDP_EHIP, "%s failed: %s", what, hipGetErrorString(e));
    };
    hipError_t e;
    if ((e = hipModuleLoadData(&mod, code.data())) != hipSuccess) fail(e, "hipModuleLoadData");
    else if ((e = hipModuleGetFunction(&fn, mod, "mdp_log_apply")) != hipSuccess) fail(e, "hipModuleGetFunction");
    else if (!(rc = dx.assign(x, n)) && !(rc = dy.grow(n))) {
        unsigned long long nn = n;
        double *px = dx.get(), *py = dy.get();
        void *args[] = {(void *)&px, (void *)&py, (void *)&nn};
        const uint32_t nb = (uint32_t)((n + kBlock - 1) / kBlock);
        if ((e = hipModuleLaunchKernel(fn, nb, 1, 1, kBlock, 1, 1, 0, nullptr, args, nullptr)) != hipSuccess)
            fail(e, "hipModuleLaunchKernel");
        else if ((e = hipMemcpy(y, py, n * sizeof(double), hipMemcpyDeviceToHost)) != hipSuccess) fail(e, "hipMemcpy");
    }
    dx.reset(), dy.reset();  // (as before: the buffers, then the module)
    if (mod) (void)hipModuleUnload(mod);
    return rc;
}

int mdp_engine_get_info(const mdp_engine *eng, mdp_engine_info *info)
{
    if (!eng || !info) return mdp_set_error(MDP_EINVAL, "null argument");
    mdp_plan_info(eng, (int)eng->devs.size(), info);
    return MDP_OK;
}

int mdp_engine_work(const mdp_engine *eng, uint64_t ne, uint64_t nc, double *flop_impl, double *flop_survey,
                    double *bytes_min)
{
    if (!eng) return mdp_set_error(MDP_EINVAL, "null engine");
    mdp_plan_work(eng, ne, nc, flop_impl, flop_survey, bytes_min);
    return MDP_OK;
}

int mdp_engine_work_fact(const mdp_engine *eng, uint64_t ne, uint64_t nc, mdp_work *w)
{
    if (!eng || !w) return mdp_set_error(MDP_EINVAL, "null argument");
    double ns = 0.0, nall = 0.0;
    for (const DevCtx &d : eng->devs) {
        ns += d.plan.ne_sform;
        nall += d.ne;
    }
    mdp_plan_work_fact(eng, ne, nc, eng->devs.empty() ? -1.0 : eng->devs[0].ct.cmax, ns, nall, w);
    return MDP_OK;
}

unsigned long long mdp_dev_live_bytes(void) { return g_dev_live_bytes.load(std::memory_order_relaxed); }

int mdp_engine_launched(const mdp_engine *eng, char *buf, size_t len)
{
    if (!eng || !buf || !len) return mdp_set_error(MDP_EINVAL, "null argument");
    std::string all;
    {
        std::lock_guard<std::mutex> lk(eng->launched_mu);
        for (const std::string &k : eng->launched) all += (all.empty() ? "" : " ") + k;
    }
    snprintf(buf, len, "%s", all.c_str());
    return (int)all.size();
}

}  // extern "C"
