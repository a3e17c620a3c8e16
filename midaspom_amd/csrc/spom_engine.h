// midaspom_amd/csrc/spom_engine.h -- internal to the posterior engine (not
// installed; the public ABI is include/midaspom.h).  Shared by
//   spom_plan.cpp    host planning: the options (parsed once into MdpOpts,
//                    every later reader takes a field), plan tables, the
//                    engine's path (MdpPath), hipRTC sources, and per grid the
//                    c tables and the grid plan (each slot's step, MdpStep,
//                    kernel variant, point list, chunk widths, buffer sizes,
//                    launch shape)
//   spom_engine.hip  the kernels; the engine (the plan plus its device contexts
//                    and run-time state); device set-up, uploads and launches
//                    as the plans say; timing
//   plan_check.cpp   the planner's stand-alone driver
// (the forward kernel's generator and its hipRTC unit, spom_jit.cpp and
// spom_jit_rtc.cpp, share spom_jit.h, included here)
// Plain C++17: the HIP header below gives the vector types (uint2, uint4) only.
#ifndef MDP_SPOM_ENGINE_H
#define MDP_SPOM_ENGINE_H

#include <hip/hip_vector_types.h>

#include <cstddef>
#include <cstdint>
#include <optional>
#include <string>
#include <type_traits>
#include <vector>

#include "mdp_internal.h"
#include "spom_jit.h"

// ---------------------------------------------------------------------------
// The contract between the plan tables (spom_plan.cpp) and the kernels and
// launchers that read them (spom_engine.hip): packed bit fields, LDS image
// sizes, per-wave work item shapes.
// ---------------------------------------------------------------------------
constexpr int kBlock = 256;
constexpr int kEPL = 2;         // k_forward: default grid points (e values) per lane
constexpr int kMaxDeg = 24;
constexpr uint32_t kSubPart = 16;   // k_coefs: subsets per work part
constexpr uint32_t kOffBits = 22;   // coefficient offset bits in a use descriptor
constexpr uint32_t kOffMask = (1u << kOffBits) - 1u;
constexpr size_t kFwdLds = 48 * 1024;      // max coefficient block staged by k_forward_lds
constexpr int kZTermsDev = 8;    // terms of a Z row's small-column series (zseries, z_split)
constexpr uint32_t kQGroup = 8;  // config 3: 808 lanes, one pass of k_qrows, <= 3 shuffle levels
constexpr uint32_t kQLanesMax = 64;  // k_qrows: lanes per entry (a power of two, <= a wave)
constexpr int kQLevelsRows = 16;     // k_qrows: groups per lane <= 2^(kQLevelsRows - 1)
constexpr uint32_t kMmaThreads = 1024;  // 16 waves
constexpr uint32_t kMmaU = 2;           // K steps (of 4) per pipeline chunk: years padded to 8 entries
constexpr uint32_t kMmaDummy = 1u << 21; // K-entry field of the descriptor row k (bits 21-28)
// the kernel's shape for NPM states a year (padded to 16): points per block,
// state buffer rows (>= 128, for the slices' partial sums), power-table row
// stride (rows r and r + 1 on different LDS bank halves)
constexpr uint32_t mma_pts(uint32_t npm) { return npm > 128 ? 32u : 64u; }
constexpr uint32_t mma_rows(uint32_t npm) { return npm > 128 ? npm : 128u; }
constexpr uint32_t mma_ps(uint32_t npm) { return mma_pts(npm) + 16u; }
// K steps (of 4 entries) per pipeline chunk: 2, or 1 with 4 point tiles
// (their 4 W operands a step leave no registers for a second step in flight)
constexpr uint32_t mmt_u(uint32_t rt) { return rt == 4 ? 1u : 2u; }
constexpr uint32_t kMmtMaxTiles = 64;   // column tiles a year (1 024 states)
constexpr uint32_t mmt_pts(uint32_t rt) { return 16u * rt; }
// power-table row stride (doubles): rows r and r + 1 on different LDS bank halves
constexpr uint32_t mmt_ps(uint32_t rt) { return rt % 2 ? 16u * rt : 16u * rt + 16u; }
constexpr uint32_t kHsRadix = 4;  // k_fwd_hs: patches per v Pe pass (at most; the plan's default)
constexpr size_t kQrowsLdsMax = 160 * 1024;  // k_qrows: every table of its c values (else MDP_QGLOBAL's path)
constexpr size_t kFusedLdsMax = 64 * 1024;  // fused forward kernel: every table of one column
constexpr int kZTerms = kZTermsDev;  // z_split: terms of the small columns' series
constexpr int kJitKblockTall = 512;  // threads of the reading kernel's tall variant (jit_build)
constexpr uint32_t kZRows = kBlock / 64;  // k_zrows: rows per workgroup (staged in dynamic LDS)
constexpr uint32_t kQrowsMaxC = 4;        // k_qrows: most c values per workgroup
constexpr int kZpvJ = 64;                 // k_zpv: hidden states per workgroup
constexpr int kZpvCT = 2;                 // k_zpv: c values per thread
constexpr int kStampSlots = 8;            // diagnostic stamps per workgroup
constexpr size_t kWidePgBytes = 256ull << 20;  // wide path: item-factor chunk
constexpr size_t kHsPgBytes = 2048ull << 20;   // k_fwd_hs: item factors of the columns of one launch
constexpr size_t kWideVBytes = 1ull << 30;     // wide path: state-vector scratch

// ---------------------------------------------------------------------------
// types
// ---------------------------------------------------------------------------
// What an engine runs: one path, decided once (mdp_plan_engine's last
// statement).  jit_plan.vlds and chunks are sub-modes of the direct paths.
enum class MdpPath : uint8_t {
    Generic,        // k_zpv -> k_coefs -> k_forward(_lds): MDP_JIT=0, or hipRTC failed
    Direct,         // k_qrows -> the forward kernel specialised with hipRTC, or its fused variant alone
    DirectQGlobal,  // its Q rows built in HBM instead (k_qrows' tables exceed the LDS, or MDP_QGLOBAL=1)
    WideHs,         // years of more than 16 states, or MDP_WIDE=1: k_zrows -> k_witems -> k_fwd_hs
    WideMmt,        // ... k_zrows -> k_witems + k_wq -> k_fwd_mmt
    WideMma,        // ... -> k_fwd_mma
    WidePlain       // ... -> k_fwd_wide
};
constexpr bool path_is_wide(MdpPath p) { return p >= MdpPath::WideHs; }
constexpr bool path_is_jit(MdpPath p) { return p == MdpPath::Direct || p == MdpPath::DirectQGlobal; }
// Q rows from k_zrows + k_witems + k_wq (k_fwd_hs reads the item factors themselves)
constexpr bool path_q_global(MdpPath p) { return p >= MdpPath::DirectQGlobal; }

// What one of a grid's three slots (0: Z rows / k_zpv, 1: Q rows / k_coefs,
// 2: forward) runs: one case per launcher body (launch_slot).  mdp_plan_steps
// is the only place that picks them.
enum class MdpStep : uint8_t {
    None,
    Zpv,
    Coefs,
    FwdGeneric,
    Zrows,
    Qrows,
    ItemsQ,        // k_witems + k_wq per chunk of c values
    ItemsAll,      // k_fwd_hs's k_witems: every column's item factors, when they fit one Pg block (wide_cb_items
                   // >= nc); else the slot stays, timed and named, with nothing in it, and FwdHs takes them
    FwdJit,
    FwdJitChunks,
    FwdHs,         // with k_witems per chunk of columns when the factors do not fit one Pg block
    FwdMmt,
    FwdMma,
    FwdPlain
};

// The tables that depend on the grid's |c| bound (mdp_plan_grid builds them;
// z_split prunes the Z rows for the bound).  Cached by cmax: a grid under the
// same bound neither rebuilds nor re-uploads them.
struct MdpCTables {
    double cmax = -1.0;          // the bound they were pruned for (-1: none yet)
    uint32_t kmax = 0;           // padded length of the longest pruned row
    uint32_t ct_len = 0;         // doubles of coltab (0: the plan never runs fused)
    std::vector<double> zs;      // k_zrows: row-major [row][k]
    std::vector<double> zsq;     // k_qrows: chain-major [row][k mod 4][k / 4] (a lane's chain contiguous)
    std::vector<double> zc;      // Z-row series coefficients [row][kZTerms]
    std::vector<double> coltab;  // the fused kernel's column image (plan offsets, zs last), 1 KiB padded
};

// What one grid runs (mdp_plan_grid): every per-grid choice of the engine,
// made on the host without a device.  set_grid_dev grows and uploads what it
// says, the launchers read it.
struct MdpGridPlan {
    MdpStep step[3] = {MdpStep::None, MdpStep::None, MdpStep::None};  // what each slot runs (mdp_plan_steps)
    uint32_t ne_sform = 0;  // e rows on the s-form (x < y), for the work count
    bool tables_new = false;  // the c tables were rebuilt for this grid (upload them)
    // forward kernels with several points per lane: list positions -> e rows
    // (bit 31: a duplicate that is computed, not stored), grouped by ratio
    // form; elist: e by list position, then e[0] (what a position past the
    // list reads).  An identity list (0, 1, ...) is not uploaded.
    std::vector<uint32_t> plist;
    std::vector<double> elist;
    uint32_t nlist = 0, nlist_epl = 0;  // list length (a multiple of nlist_epl, its points per lane)
    bool plist_identity = true;
    // the forward variant: jit_load's index (0 reading, 1 fused, 2 reading at
    // kJitKblockTall threads)
    bool fused = false, tall = false;
    int variant = 0;
    uint32_t gy = 0;   // e blocks per column of the reading shape
    uint32_t ldv = 0;  // a chunked series: e values per (state, c) of the state scratch
    // c values per k_qrows workgroup, per k_witems launch, per k_fwd_wide launch
    uint32_t qrows_cb = 1, wide_cb_items = 1, wide_cb_fwd = 1;
    // elements of the grow-only buffers (0: not used by this path)
    size_t n_qrow = 0, n_zg = 0, n_pg = 0, n_v = 0, n_vscr = 0, n_zpv = 0, n_r = 0, n_gpart = 0;
    size_t nst[3] = {0, 0, 0};  // diag stamps: workgroups of k_zpv / k_qrows, k_coefs, forward
    bool pg_zero = false;       // Pg is zero-filled (k_fwd_hs reads its rows' zero slot)
    size_t zrows_lds = 0;       // k_zrows' dynamic LDS (bytes)
    // the mdp_fwd_jit launch (mdp_plan_fwd_launch): 64-bit products, so run
    // time can still refuse a grid too large for the launch
    uint64_t fwd_nblk = 0;      // e blocks x column groups (MdpFwdJitArgs::nblk)
    uint64_t fwd_threads = 0;   // the launch's forward threads (x fwd_pro with the fused prologue's)
    uint32_t fwd_pro = 1;
    uint32_t fwd_block = 0, fwd_lds = 0;  // threads per workgroup, dynamic LDS (bytes)
    uint32_t fwd_nlist = 0;     // MdpFwdJitArgs::nlist
    bool fwd_listed = false;    // the kernel reads plist / elist
};

// The options of mdp_engine_create_opts as given, each converted once by
// parse_engine_opts (its table, spom_plan.cpp, defines what a value means).  An
// empty optional: the option was not given, and the default stays where it is
// (MdpEnginePlan's and MdpJitPlan's initialisers, the planner's constants).
// What depends on the plan (nb, the chunk count, vlds) is applied where the
// field is read.
struct MdpOpts {
    bool jit = true;          // MDP_JIT: false for the value "0" alone
    bool wide = false;        // MDP_WIDE
    bool fwd_scalar = false;  // MDP_FWD=scalar (case-sensitive)
    bool qglobal = false, gather = false, jit_check = false, jit_verbose = false;
    // MDP_EPL as written: k_forward takes 1, 2 or 4 of it, the direct paths the number itself
    std::optional<int> epl;
    std::optional<bool> diag, fused, jit_xcd, jit_efast, qrows_xcd, fast_log, jit_split, jit_rot;
    std::optional<int> fused_cols;   // 1 .. 4
    std::optional<int> jit_slots, jit_wpe, jit_window, jit_hack, wide_mma, jit_threads;  // the number itself
    std::optional<int> jit_kblock;   // 256 or 512
    std::optional<uint32_t> jit_chunk;     // >= 1
    std::optional<uint32_t> vlds_maxuses;  // >= 0
    std::optional<int> vlds_epl;     // 1 or 2
    std::optional<int> vsplit;       // 1, 2 or 4
    std::optional<uint32_t> hs_radix;  // 1 .. kHsRadix
    std::optional<uint32_t> hs_waves;  // 8 or 16
    std::optional<uint32_t> hs_probe;  // 0 .. 7
    std::optional<int> wide_cb;      // >= 1
    std::optional<std::string> jit_dump;
};

// Everything the planner writes or reads of an engine.  The engine itself
// (spom_engine.hip) derives from it and adds the device contexts and the
// run-time state: nothing that uploads or launches takes a plan.
struct MdpEnginePlan {
    uint32_t n = 0, tmax = 0, nvar = 0, nstates = 0, nextid = 0;
    uint32_t npairs = 0, nuses = 0, ncoef = 0, npmax = 1, variant = 0;
    uint32_t deg = 0;         // homogeneous transition degree D
    uint32_t maxA = 0;        // max |A| over uses
    int epl = kEPL;           // k_forward points per lane (MDP_EPL overrides: 1, 2, 4)
    bool fwd_lds = false;     // coefficient block staged in LDS (k_forward_lds)
    size_t fwd_lds_bytes = 0;
    bool lds_zpv = true;      // k_coefs stages Z/PV in LDS
    bool lds_part = true;     // k_coefs keeps subset partial sums in LDS
    bool diag = false;        // MDP_DIAG: record phase stamps
    MdpPath path = MdpPath::Generic;  // what the engine runs
    bool qrows_xcd = true;   // k_qrows deals c ranges XCD-aware (MDP_QROWS_XCD=0: blockIdx order)
    double wide_flops_pt = 0; // its FP64 flops per grid point
    int jit_epl = 1;          // its grid points per lane (Q-row reading variant and chunks)
    uint32_t jit_kblock = kBlock;  // its threads per column
    // the fused variant's: 512 threads x 1 point per column by default (the
    // same 512 e rows per block as 256 x 2, so the grid shape is shared): with
    // one point per lane its 1 024-thread blocks fit 4 waves per SIMD, and the
    // per-column prologue runs over twice the threads (config 2: -2 to -3 %)
    int jit_epl_fused = 2;
    uint32_t jit_kblock_fused = kBlock;
    uint32_t jit_pro_fused = 2;
    bool jit_shape_env = false;  // MDP_EPL / MDP_JIT_KBLOCK set: one shape for both variants
    double jit_flops_pt = 0;  // its FP64 flops per grid point (counted by the generator)
    size_t ldQ = 0;           // per-c Q block (doubles, even) read by the JIT kernel
    std::vector<char> jit_code[3];  // forward kernel code objects [variant: jit_load's index], compiled on demand
    std::string jit_src[3];         // their sources (a cached object the runtime refuses is rebuilt)
    std::vector<std::string> chunk_src;
    std::vector<MdpJitPlan> chunks;               // > 1: the series runs as chunks of years
    std::vector<std::vector<char>> chunk_code;    // their code objects
    double cbound = 0.0;         // the per-c tables' |c| bound at least this (mdp_engine_set_cbound)
    int fused_mode = -1;            // MDP_FUSED: -1 auto, 0, 1
    MdpJitPlan jit_plan;
    // direct path: k_qrows computes Pc[j][b] for the needed (j, b)
    // items, the forward kernel assembles Q from them
    uint32_t nj = 0, nitems = 0, ncoef_d = 0;
    size_t ldP = 0;
    std::vector<uint32_t> cj_bits, cj_item0, itemB, qstart, qitem, udesc_d, var_cols;
    std::vector<uint32_t> itemRow;  // row (j slot) of each item
    std::vector<uint2> qslot;       // k_qrows phase-3 lanes (build_direct_plan)
    std::vector<uint32_t> qlane;    // their groups' Pc slots, kQGroup a lane (nvar <= 8)
    std::vector<uint32_t> islot;    // k_qrows: each item's Pc slot (slots 0-15: zeros)
    uint32_t npl_slots = 0;         // k_qrows: Pc slots per c value
    uint32_t slot_conflicts = 0;    // k_qrows: extra gather cycles its slot colouring leaves (per c pair)
    uint32_t slot_store_conflicts = 0;  // and extra store-group conflicts
    // k_fwd_mma (wide years on the matrix cores): per year t its K entries
    // (k | |A_k| << 8 | m << 16 | valid << 31, padded to 4) from kbase[t],
    // and the Q-row slot of each (K entry, new state l) from gbase[t]
    uint32_t mma_npm = 0;
    std::vector<uint2> mma_kt;  // per year its K entries: LDS byte offsets of the W rows, m, k
    std::vector<uint2> mma_wplan;  // per (year, wave) its work item (chunk range, column tile, slice)
    std::vector<uint32_t> mma_kbase, mma_desc, mma_dbase;
    uint32_t mma_ktmax = 16;
    // k_fwd_mmt (round 6, the default matrix-core forward: years of up to
    // 1 024 states): RT point tiles a block, per (year, tile) K lists, per
    // (year, wave) work items (build_mmt_plan)
    uint32_t mmt_rt = 0, mmt_rows = 0;
    std::vector<uint2> mmt_kt, mmt_ktile, mmt_wplan;
    std::vector<uint32_t> mmt_cidx;
    double mmt_flops_pt = 0;  // executed MFMA flops per grid point (padding included)
    // k_fwd_hs (round 6, through the hidden states: build_hs_plan): 2^hs_nb
    // cube positions, RT point tiles; per (year, tile) K lists of hidden
    // states and their item offsets, per year butterfly passes, the new
    // states' cube positions in tile order and free 16-row park blocks
    uint32_t hs_rt = 0, hs_nb = 0, hs_nw = 16;
    uint32_t hs_probe = 0;  // MDP_HS_PROBE (timing probes only, wrong results): 1 skips v Pe, 2 U Pc
    std::vector<uint32_t> hs_kt, hs_cidx, hs_pbase, hs_dpos, hs_dbase, hs_pk;
    std::vector<uint2> hs_ppos, hs_dpk;
    std::vector<uint4> hs_wplan;
    std::vector<uint4> hs_pass;
    double hs_flops_pt = 0, hs_mfma_pt = 0;  // FP64 flops per grid point (padding included), of them MFMA
    std::vector<uint32_t> ystate;  // each year's states (short_state bits), year_off order
    uint32_t qslot_lglmax = 0;      // log2 of the widest lane segment
    std::vector<uint8_t> isvar;
    std::vector<double> Sj;  // [nj][n] colonisation sums of every column for each needed j
    std::string jit_log;
    size_t coef_lds = 0;      // k_coefs dynamic LDS bytes
    size_t lds_max = 160 * 1024;  // the device's LDS per workgroup (mdp_plan_engine's argument; 160 KiB on gfx950)
    double prior0 = 1.0;
    std::vector<uint32_t> np, pairA, pairB, pairOff, use_pair, prog, udesc, pairPart0, partP, partK0;
    MdpOpts opts;             // mdp_engine_create_opts (variant selection; no environment reads)
};

// The forward kernels' output strides: log L of point (ie, ic) at
// out[ie * se + ic * sc] -- [e][c] rows (se = ld, sc = 1) or [c][e] columns
// (se = 1, sc = ld); every forward kernel takes both.  Passed explicitly down
// every launch path: only mdp_engine_run / mdp_engine_time_kernels honour the
// engine's layout (mdp_engine_set_layout); mdp_loglik_grid always fills its
// device slab in [e][c] (its host contract).
struct OutStrides {
    uint32_t se, sc;
};
inline OutStrides layout_strides(int layout, uint32_t ld)
{
    return layout == MDP_LAYOUT_CE ? OutStrides{1u, ld} : OutStrides{ld, 1u};
}

// ---------------------------------------------------------------------------
// LDS and table sizes both sides compute (inline: the run path calls them)
// ---------------------------------------------------------------------------
// per-c coefficient stride: every forward use (deg+1 coefficients padded to
// an even count) plus two zero transitions of prefetch padding
inline size_t rsp_of(const MdpEnginePlan *eng) { return (eng->deg + 2) & ~1u; }
inline size_t ldR_of(const MdpEnginePlan *eng) { return ((size_t)eng->nuses + 2) * rsp_of(eng); }

// k_fwd_mma: two state buffers and the power tables of the block's points,
// and (LDS staging) three years' K entries
inline size_t mma_lds(const MdpEnginePlan *eng)
{
    const uint32_t npm = eng->mma_npm;
    return (2 * (size_t)mma_rows(npm) * mma_pts(npm) + 2 * ((size_t)eng->maxA + 1) * mma_ps(npm)) * sizeof(double) +
           0;
}

// k_fwd_mmt: the state buffer and the power tables of the block's points
// k_fwd_mmt's shapes by the largest year: RT point tiles, state rows, two buffers
struct MmtShape {
    uint32_t rt, rows;
    bool db;
};
// (measured, profiles/r06/wide: years of up to 128 states run 25 % faster on
// <4, 128, 2buf> than on <2, 256, 1buf>; a 256-state problem 6 % faster on
// one buffer than on <2, 256, 2buf>)
inline MmtShape mmt_shape(const MdpEnginePlan *eng)
{
    const uint32_t npmax = eng->npmax;
    if (npmax <= 128) return {4u, 128u, true};
    if (npmax <= 256) return {2u, 256u, false};
    if (npmax <= 512) return {2u, 512u, false};
    return {1u, 1024u, false};
}

inline size_t mmt_lds(const MdpEnginePlan *eng)
{
    const MmtShape sh = mmt_shape(eng);
    return ((sh.db ? 2 : 1) * (size_t)sh.rows * mmt_pts(sh.rt) + 2 * ((size_t)eng->maxA + 1) * mmt_ps(sh.rt)) *
           sizeof(double);
}

// k_fwd_hs: the cube of the block's points (128 KiB for each shape)
inline size_t hs_lds(const MdpEnginePlan *eng)
{
    return (((size_t)1 << eng->hs_nb) + eng->hs_nb + 1) * mmt_pts(eng->hs_rt) * sizeof(double);  // + y^k table
}

// k_qrows LDS for cb c values per workgroup: Z, var-column S, Pc, Q CSR
inline size_t qrows_lds(const MdpEnginePlan *eng, uint32_t cb)
{
    const size_t nv = eng->nvar <= 8 ? 8 : eng->nvar <= 16 ? 16 : 24;  // k_qrows NV
    return ((((size_t)cb * eng->nj + 1) & ~(size_t)1) + (size_t)eng->nj * (cb * nv + 2) + (size_t)cb * eng->npl_slots) *
               sizeof(double) +
           ((size_t)eng->ncoef_d + 1 + eng->qitem.size()) * sizeof(uint32_t);  // (items stay in registers)
}

// The fused forward kernel keeps its column's tables (ct_len doubles,
// dynamic LDS), Z, Pc and Q in LDS.
inline size_t fused_lds(const MdpEnginePlan *eng, size_t ct_len)
{
    const size_t fc = (size_t)eng->jit_plan.fused_cols;
    return (ct_len + 2 + fc * (eng->nj + eng->nitems + 2 * eng->ldQ)) * sizeof(double);  // + staging scratch
}

// k_fwd_wide: per-lane x^r, y^r tables, r <= maxA
inline size_t wide_lds(const MdpEnginePlan *eng) { return 2 * ((size_t)eng->maxA + 1) * kBlock * sizeof(double); }

// ---------------------------------------------------------------------------
// The instantiation set of each templated kernel family, written once: the
// switch from the plan to the one instantiation it runs, as fn(tags...) with
// std::integral_constant tags.  Raising the LDS limit, launching and naming a
// launch (mdp_engine_launched) all go through these, so they cannot name
// different instantiations.  The kFmt strings are note_launch's formats.
// ---------------------------------------------------------------------------
template <int V>
using mdp_int = std::integral_constant<int, V>;
template <bool V>
using mdp_bool = std::integral_constant<bool, V>;

constexpr const char *kFmtQrows = "k_qrows<%d,%d,%d>", *kFmtCoefs = "k_coefs<%d,%d,%d>", *kFmtWitems = "k_witems<%d>",
                     *kFmtHs = "k_fwd_hs<%u,%u>", *kFmtMmt = "k_fwd_mmt<%u,%u,%s>", *kFmtMma = "k_fwd_mma<%u>",
                     *kFmtJit = "mdp_fwd_jit<%s,maxA%u>", *kFmtJitTall = "mdp_fwd_jit<reading,kb%d>",
                     *kFmtJitChunks = "mdp_fwd_jit<reading,maxA%u,chunks%zu%s>";

// k_qrows<NV, EXACT, CB> for cb c values per workgroup: a power of two, at
// most 4, 2, 1 by NV (the register budget at 1 024 threads; else one)
template <typename F>
auto for_qrows(const MdpEnginePlan *eng, uint32_t cb, F &&fn)
{
    const uint32_t nvar = eng->nvar;
    if ((cb != 2 && cb != 4) || cb > (nvar <= 8 ? 4u : nvar <= 16 ? 2u : 1u)) {
        if (nvar == 8) return fn(mdp_int<8>(), mdp_bool<true>(), mdp_int<1>());
        if (nvar < 8) return fn(mdp_int<8>(), mdp_bool<false>(), mdp_int<1>());
        if (nvar <= 16) return fn(mdp_int<16>(), mdp_bool<false>(), mdp_int<1>());
        return fn(mdp_int<24>(), mdp_bool<false>(), mdp_int<1>());
    }
    if (cb == 2) {
        if (nvar == 8) return fn(mdp_int<8>(), mdp_bool<true>(), mdp_int<2>());
        if (nvar < 8) return fn(mdp_int<8>(), mdp_bool<false>(), mdp_int<2>());
        return fn(mdp_int<16>(), mdp_bool<false>(), mdp_int<2>());
    }
    return nvar == 8 ? fn(mdp_int<8>(), mdp_bool<true>(), mdp_int<4>()) : fn(mdp_int<8>(), mdp_bool<false>(), mdp_int<4>());
}

// the padded variable-column count of k_coefs and k_witems
template <typename F>
auto for_nv(const MdpEnginePlan *eng, F &&fn)
{
    if (eng->nvar <= 8) return fn(mdp_int<8>());
    if (eng->nvar <= 16) return fn(mdp_int<16>());
    return fn(mdp_int<24>());
}

// k_coefs<LDS_ZPV, LDS_PART, NV>
template <typename F>
auto for_coefs(const MdpEnginePlan *eng, F &&fn)
{
    if (eng->lds_zpv) return for_nv(eng, [&](auto nv) { return fn(mdp_bool<true>(), mdp_bool<true>(), nv); });
    if (eng->lds_part) return for_nv(eng, [&](auto nv) { return fn(mdp_bool<false>(), mdp_bool<true>(), nv); });
    return for_nv(eng, [&](auto nv) { return fn(mdp_bool<false>(), mdp_bool<false>(), nv); });
}

// k_fwd_hs<RT, NB, NW>
template <typename F>
auto for_hs(const MdpEnginePlan *eng, F &&fn)
{
    if (eng->hs_nb == 8)
        return eng->hs_nw == 8 ? fn(mdp_int<2>(), mdp_int<8>(), mdp_int<8>()) : fn(mdp_int<4>(), mdp_int<8>(), mdp_int<16>());
    if (eng->hs_nb == 9) return fn(mdp_int<2>(), mdp_int<9>(), mdp_int<16>());
    return fn(mdp_int<1>(), mdp_int<10>(), mdp_int<16>());
}

// k_fwd_mmt<RT, ROWS, DB>
template <typename F>
auto for_mmt(const MdpEnginePlan *eng, F &&fn)
{
    if (eng->mmt_rows == 128) return fn(mdp_int<4>(), mdp_int<128>(), mdp_bool<true>());
    if (eng->mmt_rows == 256) return fn(mdp_int<2>(), mdp_int<256>(), mdp_bool<false>());
    if (eng->mmt_rows == 512) return fn(mdp_int<2>(), mdp_int<512>(), mdp_bool<false>());
    return fn(mdp_int<1>(), mdp_int<1024>(), mdp_bool<false>());
}

// k_fwd_mma<NPM>
template <typename F>
auto for_mma(const MdpEnginePlan *eng, F &&fn)
{
    if (eng->mma_npm == 64) return fn(mdp_int<64>());
    if (eng->mma_npm == 128) return fn(mdp_int<128>());
    return fn(mdp_int<256>());
}

// ---------------------------------------------------------------------------
// planner entry points (spom_plan.cpp)
// ---------------------------------------------------------------------------

// The options string into o (reset first), by the one table of names and
// conversions; an unknown name is MDP_EINVAL, a value never is.
// diag_build: the measurement-only names (MDP_DIAG, ...) are accepted
int parse_engine_opts(const char *s, MdpOpts &o, bool diag_build);

// How far mdp_plan_engine goes with hipRTC.
enum class MdpPlanMode {
    Compile,       // compile the forward kernel the first grid most likely runs
    OfflineCheck,  // MDP_JIT_CHECK=1 without a device: compile every kernel, then MDP_ENODEV
    // no hipRTC: the specialised kernel is taken to compile, so the path is
    // a direct one with no code object behind it.  For plan_check, which plans a bare
    // MdpEnginePlan: a plan is not an engine, and nothing that uploads or
    // launches takes one.
    TablesOnly
};
// Plan the engine for problem p (eng->opts parsed): the generic plan, then the
// direct / chunked / vlds / wide one the problem and the options select, with
// lds_max the device's LDS per workgroup (160 KiB on gfx950).  jit_t (may be
// null) receives the steady-clock seconds around the hipRTC step.
int mdp_plan_engine(MdpEnginePlan *eng, const mdp_problem *p, size_t lds_max, MdpPlanMode mode, double *jit_t);

#define MDP_PLAN_GRID 1    // (plan_check.cpp also builds against planners without these: scripts/jit_sources.py --rev)
#define MDP_ENGINE_PLAN 1  // the planner takes an MdpEnginePlan
#define MDP_PLAN_PATH 1    // the plan names its path (MdpPath), the grid plan its steps
// The grid plan of e[ne] x c[nc] on a device of ncu compute units: refuses a
// c the engine does not take (MDP_EINVAL) and Z rows past k_zrows' LDS
// (MDP_EUNSUPPORTED), rebuilds ct when the grid's |c| bound (at least
// eng->cbound) is not the one it holds (g.tables_new), and fills g but for
// the forward launch.  The engine's forward shape must be known (jit_source
// of one variant has run: mdp_plan_engine's compile, or plan_check's digest).
int mdp_plan_grid(const MdpEnginePlan *eng, MdpCTables &ct, const double *e, uint32_t ne, const double *c, uint32_t nc,
                  uint32_t ncu, MdpGridPlan &g);
// The mdp_fwd_jit launch of g, once its variant's shape is known (jit_build or
// jit_source of g.variant has run: the generator settles the fused shape).
void mdp_plan_fwd_launch(const MdpEnginePlan *eng, const MdpCTables &ct, uint32_t ne, uint32_t nc, MdpGridPlan &g);
// Can any grid of this plan run the fused forward kernel?
bool mdp_plan_fused_capable(const MdpEnginePlan *eng);
// The c-independent tables of the direct and wide paths: sv[row][b], the
// colonisation sum of variable column b for row's hidden state (+inf for the
// columns of j: pressure fmin(c inf, 1) = 1.0), and the packed items {B | row
// << 24, j | (row >> 8) << 24}; one spare element each.
void mdp_plan_item_tables(const MdpEnginePlan *eng, std::vector<double> &sv, std::vector<uint2> &items);
// What each slot of a grid runs, from the engine's path and g.fused: the only
// place that knows these rules (a slot with nothing to do is MdpStep::None).
// On a default-constructed g: the steps the path alone implies.
void mdp_plan_steps(const MdpEnginePlan *eng, MdpGridPlan &g);
// The kernel instantiations one run of the grid notes for mdp_engine_launched,
// sorted (the generic path's forward kernel is left to its launcher).
std::vector<std::string> mdp_plan_grid_kernels(const MdpEnginePlan *eng, const MdpGridPlan &g, uint32_t ne, uint32_t nc);

// The arithmetic of mdp_engine_get_info / _work / _work_fact; from the device
// contexts: their count, the |c| bound the first one's c tables hold for
// (< 0: none yet), the current grids' e rows on the s-form (ns of nall).
void mdp_plan_info(const MdpEnginePlan *eng, int n_devices, mdp_engine_info *info);
void mdp_plan_work(const MdpEnginePlan *eng, uint64_t ne, uint64_t nc, double *flop_impl, double *flop_survey,
                   double *bytes_min);
void mdp_plan_work_fact(const MdpEnginePlan *eng, uint64_t ne, uint64_t nc, double cmax, double ns, double nall,
                        mdp_work *w);

void z_split(const MdpEnginePlan *eng, uint32_t js, double cmax, std::vector<double> &large, double *coef,
             std::vector<uint32_t> *cols = nullptr);
std::string jit_source(MdpEnginePlan *eng, int variant);  // the forward kernel's source (no hipRTC)
int jit_build(MdpEnginePlan *eng, int variant);
int jit_build_chunks(MdpEnginePlan *eng);

#endif
