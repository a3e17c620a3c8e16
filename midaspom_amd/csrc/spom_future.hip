// midaspom_amd/csrc/spom_future.hip -- MI355X engine for the reference's
// forward-simulation program MIDASPOM_future:
//   /root/reference/sources/main_MIDASPOM_future.c:343-386  (replicate loop)
//   /root/reference/sources/main_MIDASPOM_future.c:64-110   (simpij: one year)
//
// Every replicate
//   1. samples (e, c) from the trapezoid-weighted posterior by inverse CDF on
//      the (necstep-1)^2 scale with the hard-coded e = ie*0.01, c = ic*0.01
//      (:361-375); a draw above the last cumulative value keeps the previous
//      replicate's (e, c) (the goto is skipped), (0, 0) before the first;
//   2. picks the initial state uniformly among the missing-data completions
//      of the last survey row (:378-379);
//   3. simulates tfut years of extinction (E = e/K_D) then colonisation
//      (pC = min(1, c*(sum_{l occupied, l != k} M[l][k]*K_D + M[n][k]*K_S)))
//      and counts, per year, the replicates with every patch empty (:381-385).
//
// GPU design: one lane per replicate (grid-stride over replicates, >= 8
// waves per CU), the occupancy of all patches as one 64-bit mask in a VGPR,
// the colonisation sums in registers (a template over the padded patch
// count), the M*K_D table read with uniform addresses (scalar loads), and
// the per-year all-extinct counts aggregated by wave ballots into LDS, then
// per workgroup into a partial table reduced by k_future_sum (integer sums,
// deterministic).
// Surveys of more than 64 patches (mdp_future_create_opts, MDP_FUT_WIDE) run
// the patch-parallel k_future_wide<NP> further down: one wave per replicate.
// The ensemble's summaries (mdp_future_summary: per-year histograms of the
// number of occupied patches, per-patch occupancy counts) come from the
// variants k_future_tab<NM> and k_future_wide_tab<NP>, one launch per window
// of years.  The model's year is lane_year / wide_year of spom_sim_year.h,
// shared with the scenario simulators, which k_future_tab and both wide
// kernels call; k_future<NM> holds the lane year inline.
//
// Random numbers: the reference draws rand()/RAND_MAX from one sequential
// stream per process (srand(time(NULL)), :345).  Here every draw is
// addressed -- Philox4x32-10 keyed by the 64-bit seed, counter (replicate,
// year, patch pair) -- so a replicate's trajectory is independent of how
// replicates are split over lanes, workgroups or GPUs.  A draw is the high
// 31 bits of a Philox word r, used exactly as the reference uses rand():
// u = (double)r / (double)RAND_MAX, init = r % npstates.  Word layout of
// philox(key, {rep_lo, rep_hi, t, k >> 1}): [2*(k&1)] extinction draw of
// patch k, [2*(k&1)+1] its colonisation draw; counter {rep_lo, rep_hi,
// 0xffffffff, 0}: word 0 the posterior draw, word 1 the initial state.  The
// CPU restatement (oracle/spom_future_oracle.c) uses the same stream, so the
// counts agree bit for bit; with glibc rand() it reproduces the reference's
// own sequential stream (statistical parity, tests/test_future_oracle.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <type_traits>
#include <vector>

#include "spom_dev.h"
#include "spom_future_plan.h"

#pragma clang fp contract(off)

#include "spom_rng.h"  // u32x4, philox, kRandMax, u_gt, u_lt (shared with spom_scnsim.hip)
#include "spom_sim_year.h"  // kTabN, lane_year<NM>, wide_year<NP>

namespace {

constexpr int kFutBlock = 256;
constexpr int kFutMaxWG = 4096;         // grid-stride cap (>= 16 workgroups per CU)
constexpr uint32_t kFutMaxT = 12288;    // LDS year counters (48 KB; + 16 KB table for n <= 8)
constexpr uint32_t kLookBack = 1u << 16;

struct FutArgs {
    uint32_t n, nmiss, tfut, lvalid;
    uint64_t occ0;          // bit k = patch k occupied in the last survey (:315-316)
    uint64_t rep0, nrep;    // global index of the first replicate, count
    uint32_t key0, key1;    // seed
    uint32_t necstep, pad;
    double pscale;          // (double)((necstep-1)*(necstep-1)) (:361)
    double K;               // K_D (:67, :93)
};

// first i < len with x < pcum[i] (pcum non-decreasing), or len
__device__ __forceinline__ uint32_t upper_bound(const double *__restrict__ pcum, uint32_t len, double x)
{
    uint32_t lo = 0, cnt = len;
    while (cnt > 0) {
        const uint32_t half = cnt >> 1, mid = lo + half;
        if (!(x < pcum[mid])) lo = mid + 1, cnt -= half + 1;
        else cnt = half;
    }
    return lo;
}

// colonisation sums of every survivor set of n <= 8 patches:
// T[surv][k] = (sum_{l in surv, l != k, ascending} M[l][k]*K_D) + M[n][k]*K_S,
// the reference's s1 of simpij :89-95 (its added zeros change nothing).  The
// source term is in the table, so this is not sim_year_table.
__global__ __launch_bounds__(256) void k_future_table(const double *__restrict__ MK, const double *__restrict__ src,
                                                      uint32_t n, double *__restrict__ T)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (1u << kTabN) * kTabN) return;
    const uint32_t surv = i / kTabN, k = i % kTabN;
    double s1 = 0.0;
    for (uint32_t l = 0; l < n; ++l)
        if (l != k && ((surv >> l) & 1u)) s1 += MK[l * kTabN + k];
    T[i] = s1 + src[k];
}

// ---------------------------------------------------------------------------
// The replicate model of the lane kernels as functions: fut_draw and
// fut_rates (also the wide kernels'), fut_init, and fut_year<NM>, which is
// lane_year<NM> of spom_sim_year.h with this engine's pC.  k_future_tab<NM>
// calls them.  k_future<NM> below still holds the same text inline: with the
// year alone replaced by the call its listing changes, and with the prologue
// replaced as well k_future<64> measured 0.2-0.4 % slower than its parent
// build.  So the model's year stands in three places --
// lane_year, wide_year and k_future<NM> -- and a change to the lane year is
// made in lane_year and here; the tests pin the two to each other
// (hist[:, 0] of k_future_tab equals k_future's counts).
// ---------------------------------------------------------------------------
// (e, c) cell of replicate rg from the posterior, with the reference's
// carry-over (:361-377): idx < lvalid is the cell, lvalid "never found";
// init_w the replicate's initial-state draw.  overflow() runs when the
// look-back passes kLookBack replicates.
template <typename F>
__device__ __forceinline__ void fut_draw(uint32_t key0, uint32_t key1, uint32_t lvalid, double pscale,
                                         const double *__restrict__ pcum, uint64_t rg, uint32_t &idx,
                                         uint32_t &init_w, F overflow)
{
    idx = lvalid, init_w = 0;
    uint64_t q = rg;
    for (uint32_t step = 0;; ++step) {
        const u32x4 w = philox(key0, key1, u32x4{(uint32_t)q, (uint32_t)(q >> 32), 0xffffffffu, 0u});
        if (step == 0) init_w = w.y >> 1;
        if (lvalid == 0) break;  // empty / all-NaN posterior: never found
        const double pec = pscale * (double)(w.x >> 1) / kRandMax;
        idx = upper_bound(pcum, lvalid, pec);
        if (idx < lvalid || q == 0) break;
        if (step + 1 >= kLookBack) {  // posterior mass too small for an exact look-back
            overflow();
            break;
        }
        --q;
    }
}

// E = min(1, e/K_D) (simpij :67, :74) and c of posterior cell idx
__device__ __forceinline__ double fut_rates(uint32_t idx, uint32_t lvalid, uint32_t necstep, double K, double &c)
{
    uint32_t ie = 0, ic = 0;
    if (idx < lvalid) ie = idx / necstep, ic = idx - ie * necstep;
    const double e = (double)ie * 0.01;
    c = (double)ic * 0.01;
    double E = e / K;
    if (E > 1) E = 1;
    return E;
}

// initial state of the lane kernels: missing columns filled from init (first
// missing = MSB) (:315-321, :378)
__device__ __forceinline__ uint64_t fut_init(uint64_t occ0, uint32_t nmiss, const uint64_t *__restrict__ missbit,
                                             uint32_t init_w)
{
    const uint32_t init = init_w & ((1u << nmiss) - 1u);
    uint64_t occ = occ0;
    for (uint32_t q = 0; q < nmiss; ++q)
        if ((init >> (nmiss - 1 - q)) & 1u) occ |= missbit[q];
    return occ;
}

// one year of replicate rg (simpij :64-110): the occupancy after year t + 1.
// lane_year on the table scaled by K_D: the source term src_k = M[n][k] K_S
// joins every sum behind the survivors' terms (in T for NM = 8), pC = c s1.
template <int NM>
__device__ __forceinline__ uint64_t fut_year(const FutArgs &a, const double *__restrict__ MK,
                                             const double *__restrict__ src, const double *Ts, uint64_t rg,
                                             uint32_t t, uint32_t npairs, uint64_t occ, double E, double c)
{
    return lane_year<NM>(a, MK, Ts, rg, t, npairs, occ, E, src, [&](double s, int) { return c * s; });
}

template <int NM>
__global__ __launch_bounds__(kFutBlock) void k_future(FutArgs a, const double *__restrict__ MK,
                                                      const double *__restrict__ src,
                                                      const double *__restrict__ pcum,
                                                      const uint64_t *__restrict__ missbit,
                                                      const double *__restrict__ T,
                                                      uint32_t *__restrict__ partial, uint32_t *__restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    // NM == 8: the colonisation table (16 KB) first, then the year counters
    double *Ts = dyn;
    uint32_t *cnt = (uint32_t *)(dyn + (NM == kTabN ? (1 << kTabN) * kTabN : 0));
    if constexpr (NM == kTabN) {
        for (uint32_t i = threadIdx.x; i < (1u << kTabN) * kTabN / 2; i += kFutBlock)
            reinterpret_cast<double2 *>(Ts)[i] = reinterpret_cast<const double2 *>(T)[i];
    }
    for (uint32_t t = threadIdx.x; t < a.tfut; t += kFutBlock) cnt[t] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t npairs = (a.n + 1) >> 1;
    for (uint64_t r = (uint64_t)blockIdx.x * kFutBlock + threadIdx.x; r < a.nrep;
         r += (uint64_t)gridDim.x * kFutBlock) {
        const uint64_t rg = a.rep0 + r;
        // ---- (e, c) from the posterior, with the reference's carry-over (:361-377)
        uint32_t idx = a.lvalid, init_w = 0;
        {
            uint64_t q = rg;
            for (uint32_t step = 0;; ++step) {
                const u32x4 w = philox(a.key0, a.key1, u32x4{(uint32_t)q, (uint32_t)(q >> 32), 0xffffffffu, 0u});
                if (step == 0) init_w = w.y >> 1;
                if (a.lvalid == 0) break;  // empty / all-NaN posterior: never found
                const double pec = a.pscale * (double)(w.x >> 1) / kRandMax;
                idx = upper_bound(pcum, a.lvalid, pec);
                if (idx < a.lvalid || q == 0) break;
                if (step + 1 >= kLookBack) {  // posterior mass too small for an exact look-back
                    atomicOr(err, 1u);
                    break;
                }
                --q;
            }
        }
        uint32_t ie = 0, ic = 0;
        if (idx < a.lvalid) ie = idx / a.necstep, ic = idx - ie * a.necstep;
        const double e = (double)ie * 0.01, c = (double)ic * 0.01;
        double E = e / a.K;  // simpij :67, :74
        if (E > 1) E = 1;
        // ---- initial state: missing columns filled from init (first missing = MSB) (:315-321, :378)
        const uint32_t init = init_w & ((1u << a.nmiss) - 1u);
        uint64_t occ = a.occ0;
        for (uint32_t q = 0; q < a.nmiss; ++q)
            if ((init >> (a.nmiss - 1 - q)) & 1u) occ |= missbit[q];
        // ---- tfut years (:381-385)
        for (uint32_t t = 0; t < a.tfut; ++t) {
            uint64_t surv = 0;
            uint32_t colw[NM];
#pragma unroll
            for (int m = 0; m < NM / 2; ++m) {
                if ((uint32_t)m < npairs) {
                    const u32x4 w = philox(a.key0, a.key1, u32x4{(uint32_t)rg, (uint32_t)(rg >> 32), t, (uint32_t)m});
                    const uint32_t k0 = 2 * m, k1 = 2 * m + 1;
                    colw[k0] = w.y >> 1;
                    colw[k1] = w.w >> 1;
                    // extinction: an occupied patch survives if u > E (:75-82)
                    if (((occ >> k0) & 1u) && u_gt(w.x >> 1, E)) surv |= 1ull << k0;
                    if (((occ >> k1) & 1u) && u_gt(w.z >> 1, E)) surv |= 1ull << k1;
                } else {
                    colw[2 * m] = colw[2 * m + 1] = 0;
                }
            }
            // colonisation sums, ascending l for every k (:89-95)
            double s1[NM];
            if constexpr (NM == kTabN) {
                const double2 *row = reinterpret_cast<const double2 *>(Ts + (uint32_t)surv * kTabN);
#pragma unroll
                for (int k = 0; k < NM; k += 2) {
                    const double2 v = row[k / 2];
                    s1[k] = v.x, s1[k + 1] = v.y;
                }
            } else {
#pragma unroll
                for (int k = 0; k < NM; ++k) s1[k] = 0.0;
                for (uint32_t l = 0; l < a.n; ++l) {
                    const bool on = (surv >> l) & 1u;
#pragma unroll
                    for (int k = 0; k < NM; ++k) s1[k] += on ? MK[l * NM + k] : 0.0;
                }
#pragma unroll
                for (int k = 0; k < NM; ++k) s1[k] += src[k];
            }
            uint64_t nw = surv;
#pragma unroll
            for (int k = 0; k < NM; ++k) {
                if ((uint32_t)k < a.n && !((surv >> k) & 1u)) {
                    double pc = c * s1[k];  // :95-97
                    if (pc > 1) pc = 1;
                    if (u_lt(colw[k], pc)) nw |= 1ull << k;  // :98-101
                }
            }
            occ = nw;
            const uint64_t ext = __ballot(occ == 0);
            if (ext && lane == (uint32_t)(__ffsll((unsigned long long)__ballot(1)) - 1))
                atomicAdd(&cnt[t], (uint32_t)__popcll(ext));
        }
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < a.tfut; t += kFutBlock) partial[(size_t)blockIdx.x * a.tfut + t] = cnt[t];
}

// counts[t] = sum over workgroups of partial[wg][t]  (one workgroup per year)
__global__ __launch_bounds__(256) void k_future_sum(const uint32_t *__restrict__ partial, uint32_t nwg, uint32_t tfut,
                                                    unsigned long long *__restrict__ counts)
{
    __shared__ unsigned long long red[256];
    const uint32_t t = blockIdx.x;
    unsigned long long s = 0;
    for (uint32_t b = threadIdx.x; b < nwg; b += 256) s += partial[(size_t)b * tfut + t];
    red[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[t] = red[0];
}

// ---------------------------------------------------------------------------
// Patch-parallel form for 65..1024 patches (and, by option, any n): one wave
// per replicate, the patches spread over its lanes.  Lane lambda owns the
// patch pairs m = lambda + 64*j, j < NP (patches 2m, 2m+1: one Philox call
// per pair and year gives the four draws), and holds their occupancy in bits
// 2j, 2j+1 of one word.  The survivors of a year are wave ballots, one
// 64-bit mask per (j, parity), walked in ascending patch order; every step
// adds one row of the dispersal table to the lane's 2*NP running sums.  The
// table is Toeplitz, so a row is a window of the two-sided distance image
// (spom_future_plan.h) in LDS: consecutive lanes read consecutive 16-byte
// slots, from the copy whose alignment fits the parity of the survivor.
// Same stream, same sums in the same order as k_future<NM>: the same counts.
// ---------------------------------------------------------------------------
struct FutWideArgs {
    uint32_t n, nmiss, tfut, lvalid;
    uint64_t rep0, nrep;
    uint32_t key0, key1;
    uint32_t necstep, len;  // len: doubles per copy of the distance image
    uint32_t ks0, pad;      // ks0: K_S == 0, an extinct replicate stays extinct
    double pscale;
    double K;
};

constexpr int kWideWaves = kFutBlock / 64;  // replicates in flight per workgroup

// bit 2j+p set where patch 2*(lane + 64*j) + p exists
template <int NP>
__device__ __forceinline__ uint32_t fut_wide_live(uint32_t n, uint32_t lane)
{
    uint32_t live = 0;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const uint32_t k0 = 2 * (lane + 64u * j);
        if (k0 < n) live |= 1u << (2 * j);
        if (k0 + 1 < n) live |= 2u << (2 * j);
    }
    return live;
}

// initial state of a wave's replicate: missing patches filled from init
// (first missing = MSB) (:315-321, :378)
__device__ __forceinline__ uint32_t fut_wide_init(uint32_t occ_init, uint32_t nmiss, const uint32_t *__restrict__ miss,
                                                  uint32_t init_w, uint32_t lane)
{
    const uint32_t init = init_w & ((1u << nmiss) - 1u);
    uint32_t occ = occ_init;
    for (uint32_t q = 0; q < nmiss; ++q) {
        const uint32_t mq = miss[q];
        if (((init >> (nmiss - 1 - q)) & 1u) && lane == (mq >> 8)) occ |= 1u << (mq & 0xffu);
    }
    return occ;
}

template <int NP>
__global__ __launch_bounds__(kFutBlock) void k_future_wide(FutWideArgs a, const double *__restrict__ image,
                                                           const double *__restrict__ src,
                                                           const double *__restrict__ pcum,
                                                           const uint32_t *__restrict__ occ0,
                                                           const uint32_t *__restrict__ miss,
                                                           uint32_t *__restrict__ partial,
                                                           uint32_t *__restrict__ states, uint32_t *__restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    // both copies of the distance image first (2*len doubles), then the year counters
    double2 *G2 = reinterpret_cast<double2 *>(dyn);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(dyn + 2 * a.len);
    for (uint32_t i = threadIdx.x; i < a.len; i += kFutBlock) G2[i] = reinterpret_cast<const double2 *>(image)[i];
    for (uint32_t t = threadIdx.x; t < a.tfut; t += kFutBlock) cnt[t] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t npairs = (a.n + 1) >> 1;
    const uint32_t occ_init = occ0[lane];
    const uint32_t live = fut_wide_live<NP>(a.n, lane);
    for (uint64_t r = (uint64_t)blockIdx.x * kWideWaves + wave; r < a.nrep; r += (uint64_t)gridDim.x * kWideWaves) {
        const uint64_t rg = a.rep0 + r;  // wave-uniform from here to the state
        uint32_t idx, init_w;
        fut_draw(a.key0, a.key1, a.lvalid, a.pscale, pcum, rg, idx, init_w, [&]() {
            if (lane == 0) atomicOr(err, 1u);
        });
        double c;
        const double E = fut_rates(idx, a.lvalid, a.necstep, a.K, c);
        uint32_t occ = fut_wide_init(occ_init, a.nmiss, miss, init_w, lane);
        // ---- tfut years (:381-385)
        for (uint32_t t = 0; t < a.tfut; ++t) {
            occ = wide_year<NP>(a, G2, src, rg, t, lane, npairs, live, occ, E,
                                [&](double s, double sk) { return c * (s + sk); });
            if (__ballot(occ != 0) == 0) {
                if (!a.ks0) {
                    if (lane == 0) atomicAdd(&cnt[t], 1u);
                } else {
                    // no source: every sum is 0, pC = c*0, and no draw is
                    // below 0 -- the replicate is extinct in every later year
                    for (uint32_t tt = t + lane; tt < a.tfut; tt += 64) atomicAdd(&cnt[tt], 1u);
                    break;
                }
            }
        }
        if (states) states[r * 64 + lane] = occ;
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < a.tfut; t += kFutBlock) partial[(size_t)blockIdx.x * a.tfut + t] = cnt[t];
}

// ---------------------------------------------------------------------------
// The summary path (mdp_future_summary): hist[t][m], the replicates with
// exactly m occupied patches after year t + 1, and occ[t][k], those with
// patch k occupied.  k_future_tab<NM> and k_future_wide_tab<NP> run the same
// years on the same draws as k_future<NM> and k_future_wide<NP> (the fut_*
// functions above) over one window [t0, t1) of years per launch, and count
// into a window table in LDS: 32-bit integer atomics and ballots, exact in
// any order.  Between launches a replicate rests in a record (its posterior
// cell and occupancy); the draws are addressed, so resuming is exact.  Every
// workgroup adds its non-zero cells to the global 64-bit table
// tab[t][2n+1] (hist, then occ) with integer atomics.
// ---------------------------------------------------------------------------
struct FutSumWin {
    uint32_t t0, t1;   // the launch's years
    uint32_t cells;    // LDS cells per year (FutSumPlan)
    uint32_t last;     // t1 == tfut: no record is written
};

template <int NM>
__global__ __launch_bounds__(kFutBlock) void k_future_tab(FutArgs a, FutSumWin w, const double *__restrict__ MK,
                                                          const double *__restrict__ src,
                                                          const double *__restrict__ pcum,
                                                          const uint64_t *__restrict__ missbit,
                                                          const double *__restrict__ T,
                                                          uint64_t *__restrict__ rec_occ,
                                                          uint32_t *__restrict__ rec_idx,
                                                          unsigned long long *__restrict__ tab,
                                                          uint32_t *__restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    // NM == 8: the colonisation table (16 KB) first, then the window table
    double *Ts = dyn;
    uint32_t *win = (uint32_t *)(dyn + (NM == kTabN ? (1 << kTabN) * kTabN : 0));
    const uint32_t ncell = (w.t1 - w.t0) * w.cells;
    if constexpr (NM == kTabN) {
        for (uint32_t i = threadIdx.x; i < (1u << kTabN) * kTabN / 2; i += kFutBlock)
            reinterpret_cast<double2 *>(Ts)[i] = reinterpret_cast<const double2 *>(T)[i];
    }
    for (uint32_t i = threadIdx.x; i < ncell; i += kFutBlock) win[i] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t npairs = (a.n + 1) >> 1;
    // wave-uniform trip count: the lanes past the last replicate stay in the
    // ballots (inactive, counted nowhere), so lane k is there to take patch k
    for (uint64_t rb = (uint64_t)blockIdx.x * kFutBlock + (threadIdx.x & ~63u); rb < a.nrep;
         rb += (uint64_t)gridDim.x * kFutBlock) {
        const uint64_t r = rb + lane, rg = a.rep0 + r;
        const bool act = r < a.nrep;
        uint32_t idx = a.lvalid;
        uint64_t occ = 0;
        if (act) {
            if (w.t0 == 0) {
                uint32_t init_w;
                fut_draw(a.key0, a.key1, a.lvalid, a.pscale, pcum, rg, idx, init_w, [&]() { atomicOr(err, 1u); });
                occ = fut_init(a.occ0, a.nmiss, missbit, init_w);
            } else {
                idx = rec_idx[r];
                occ = rec_occ[r];
            }
        }
        double c;
        const double E = fut_rates(idx, a.lvalid, a.necstep, a.K, c);
        for (uint32_t t = w.t0; t < w.t1; ++t) {
            if (act) occ = fut_year<NM>(a, MK, src, Ts, rg, t, npairs, occ, E, c);
            uint32_t *row = win + (t - w.t0) * w.cells;
            // hist: one LDS atomic per distinct occupied count in the wave
            const uint32_t m = (uint32_t)__popcll(occ);
            uint64_t rem = __ballot(act);
            while (rem) {
                const uint32_t lead = (uint32_t)__builtin_ctzll(rem);
                const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)m, (int)lead);
                const uint64_t same = __ballot(act && m == v);
                if (lane == lead) atomicAdd(&row[v], (uint32_t)__popcll(same));
                rem &= ~same;
            }
            // occ: lane k takes the wave's count of patch k
            uint32_t mine = 0;
            for (uint32_t k = 0; k < a.n; ++k) {
                const uint32_t cnt = (uint32_t)__popcll(__ballot(act && ((occ >> k) & 1u)));
                if (lane == k) mine = cnt;
            }
            if (mine) atomicAdd(&row[a.n + 1 + lane], mine);
        }
        if (act && !w.last) {
            rec_idx[r] = idx;
            rec_occ[r] = occ;
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < ncell; i += kFutBlock) {
        const uint32_t v = win[i];
        if (v) atomicAdd(&tab[(size_t)w.t0 * w.cells + i], (unsigned long long)v);
    }
}

template <int NP>
__global__ __launch_bounds__(kFutBlock) void k_future_wide_tab(FutWideArgs a, FutSumWin w,
                                                               const double *__restrict__ image,
                                                               const double *__restrict__ src,
                                                               const double *__restrict__ pcum,
                                                               const uint32_t *__restrict__ occ0,
                                                               const uint32_t *__restrict__ miss,
                                                               uint32_t *__restrict__ rec_occ,
                                                               uint32_t *__restrict__ rec_idx,
                                                               unsigned long long *__restrict__ tab,
                                                               uint32_t *__restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    // both copies of the distance image first (2*len doubles), then the window
    // table: per year hist[n+1], then occ in lane order -- bit b of lane lam
    // (patch 2*(lam + 64*(b/2)) + b%2) in cell 64*b + lam, so that the lanes
    // of a wave hit consecutive banks
    double2 *G2 = reinterpret_cast<double2 *>(dyn);
    uint32_t *win = reinterpret_cast<uint32_t *>(dyn + 2 * a.len);
    const uint32_t ncell = (w.t1 - w.t0) * w.cells;
    for (uint32_t i = threadIdx.x; i < a.len; i += kFutBlock) G2[i] = reinterpret_cast<const double2 *>(image)[i];
    for (uint32_t i = threadIdx.x; i < ncell; i += kFutBlock) win[i] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t npairs = (a.n + 1) >> 1;
    const uint32_t occ_init = occ0[lane];
    const uint32_t live = fut_wide_live<NP>(a.n, lane);
    for (uint64_t r = (uint64_t)blockIdx.x * kWideWaves + wave; r < a.nrep; r += (uint64_t)gridDim.x * kWideWaves) {
        const uint64_t rg = a.rep0 + r;  // wave-uniform
        uint32_t idx, occ;
        if (w.t0 == 0) {
            uint32_t init_w;
            fut_draw(a.key0, a.key1, a.lvalid, a.pscale, pcum, rg, idx, init_w, [&]() {
                if (lane == 0) atomicOr(err, 1u);
            });
            occ = fut_wide_init(occ_init, a.nmiss, miss, init_w, lane);
        } else {
            idx = rec_idx[r];
            occ = rec_occ[r * 64 + lane];
        }
        double c;
        const double E = fut_rates(idx, a.lvalid, a.necstep, a.K, c);
        for (uint32_t t = w.t0; t < w.t1; ++t) {
            if (a.ks0 && __ballot(occ != 0) == 0) {
                // no source and nobody left (at a window's start too): every
                // sum is 0, pC = c*0, and no draw is below 0 -- hist[tt][0]
                // for the rest of the window, nothing to occ
                for (uint32_t tt = t + lane; tt < w.t1; tt += 64) atomicAdd(&win[(tt - w.t0) * w.cells], 1u);
                break;
            }
            occ = wide_year<NP>(a, G2, src, rg, t, lane, npairs, live, occ, E,
                                [&](double s, double sk) { return c * (s + sk); });
            uint32_t *row = win + (t - w.t0) * w.cells;
            uint32_t m = 0;
#pragma unroll
            for (int b = 0; b < 2 * NP; ++b) {
                const bool on = (occ >> b) & 1u;
                m += (uint32_t)__popcll(__ballot(on));
                if (on) atomicAdd(&row[a.n + 1 + 64 * b + lane], 1u);
            }
            if (lane == 0) atomicAdd(&row[m], 1u);
        }
        if (!w.last) {
            if (lane == 0) rec_idx[r] = idx;
            rec_occ[r * 64 + lane] = occ;
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < ncell; i += kFutBlock) {
        const uint32_t v = win[i];
        if (!v) continue;
        const uint32_t y = i / w.cells, cl = i - y * w.cells;
        const int32_t g = fut_sum_wide_cell(a.n, cl);
        if (g >= 0) atomicAdd(&tab[(size_t)(w.t0 + y) * (2 * a.n + 1) + (uint32_t)g], (unsigned long long)v);
    }
}

// tab[t][2n+1] -> hist[t][n+1] and occ[t][n] (either may be null)
__global__ __launch_bounds__(256) void k_future_split(const unsigned long long *__restrict__ tab, uint32_t ncell,
                                                      uint32_t n, unsigned long long *__restrict__ hist,
                                                      unsigned long long *__restrict__ occ)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ncell) return;
    const uint32_t t = i / (2 * n + 1), c = i - t * (2 * n + 1);
    if (c <= n) {
        if (hist) hist[(size_t)t * (n + 1) + c] = tab[i];
    } else if (occ) {
        occ[(size_t)t * n + (c - n - 1)] = tab[i];
    }
}

}  // namespace
// (DevQueue: the device, stream and events, released after the buffers below)
// The stream rule (spom_dev.h): no grid is uploaded here, but the partial
// counts, the summary table, the replicate records and the device forms'
// look-back flag (dpartial, dtab, drec_*, derr[0]) are one set per engine,
// shared by every call.  A device form notes the caller's stream and waits for
// one pending on another stream; the host forms and the timing calls, which
// run on the engine's own stream, wait for whatever is pending.
struct mdp_future : DevQueue {
    uint32_t n = 0, nm = 0, nmiss = 0, necstep = 0, lvalid = 0;
    uint64_t occ0 = 0;
    double K = 1.0, pscale = 0.0;
    DevBuf<double> dMK, dsrc, dpcum, dT;
    DevBuf<uint64_t> dmiss;
    DevBuf<uint32_t> dpartial, derr;
    DevBuf<unsigned long long> dcounts;
    // k_future_wide<np> (np > 0): its tables instead of dMK / dmiss / dT
    uint32_t np = 0, wlen = 0, ks0 = 0;
    DevBuf<double> dimage;
    DevBuf<uint32_t> docc0, dwmiss, dstates;  // dstates: 64 lane words a replicate
    char kname[32] = "";
    // the summary path: its window cap (MDP_FUT_SUM_YEARS), the global table
    // [tfut][2n+1] and the records of a launch's replicates (drec_occ: one
    // 64-bit word a replicate, or k_future_wide_tab's 64 lane words = 32)
    uint32_t sum_years = 0;
    DevBuf<unsigned long long> dtab;
    DevBuf<uint64_t> drec_occ;
    DevBuf<uint32_t> drec_idx;
    ~mdp_future() { drain(); }
};

namespace {

// the refusal of a look-back overflow, from the flag a finished launch left;
// device_path: the text of mdp_future_check
int fut_lookback(uint32_t err, bool device_path)
{
    if (!err) return MDP_OK;
    return mdp_set_error(MDP_EUNSUPPORTED,
                         "a posterior draw needed more than %u look-back replicates (posterior mass far "
                         "below the (necstep-1)^2 scale)%s",
                         kLookBack, device_path ? ": the device counts are not valid" : "");
}

// replicates per workgroup: one per lane, or one per wave (k_future_wide)
uint64_t fut_per_wg(const mdp_future *f) { return f->np ? kWideWaves : kFutBlock; }

int fut_grid(const mdp_future *f, uint64_t nrep)
{
    const uint64_t wg = (nrep + fut_per_wg(f) - 1) / fut_per_wg(f);
    return (int)std::max<uint64_t>(1, std::min<uint64_t>(wg, kFutMaxWG));
}

int fut_reserve(mdp_future *f, int nwg, uint32_t tfut)
{
    if (int rc = f->dpartial.grow((size_t)nwg * tfut)) return rc;
    return f->dcounts.grow(tfut);
}

FutArgs fut_args(const mdp_future *f, uint64_t seed, uint64_t rep0, uint64_t nrep, uint32_t tfut)
{
    FutArgs a{};
    a.n = f->n;
    a.nmiss = f->nmiss;
    a.tfut = tfut;
    a.lvalid = f->lvalid;
    a.occ0 = f->occ0;
    a.rep0 = rep0;
    a.nrep = nrep;
    a.key0 = (uint32_t)seed;
    a.key1 = (uint32_t)(seed >> 32);
    a.necstep = f->necstep;
    a.pscale = f->pscale;
    a.K = f->K;
    return a;
}

FutWideArgs fut_wide_args(const mdp_future *f, uint64_t seed, uint64_t rep0, uint64_t nrep, uint32_t tfut)
{
    FutWideArgs a{};
    a.n = f->n;
    a.nmiss = f->nmiss;
    a.tfut = tfut;
    a.lvalid = f->lvalid;
    a.rep0 = rep0;
    a.nrep = nrep;
    a.key0 = (uint32_t)seed;
    a.key1 = (uint32_t)(seed >> 32);
    a.necstep = f->necstep;
    a.len = f->wlen;
    a.ks0 = f->ks0;
    a.pscale = f->pscale;
    a.K = f->K;
    return a;
}

size_t fut_wide_lds(const mdp_future *f, uint32_t tfut)
{
    return (size_t)2 * f->wlen * sizeof(double) + (size_t)tfut * sizeof(uint32_t);
}

// k_future_wide<np> over replicates [rep0, rep0 + nrep); d_states: the final
// lane words of every replicate ([nrep][64]) or null
int fut_launch_wide(mdp_future *f, uint64_t seed, uint64_t rep0, uint64_t nrep, uint32_t tfut, hipStream_t st,
                    uint32_t *d_states, uint32_t *derr)
{
    const FutWideArgs a = fut_wide_args(f, seed, rep0, nrep, tfut);
    const int nwg = fut_grid(f, nrep);
    const size_t lds = fut_wide_lds(f, tfut);
    if (int rc = dev_for_pairs(f->np, [&](auto NP) {
            hipLaunchKernelGGL(k_future_wide<decltype(NP)::value>, dim3(nwg), dim3(kFutBlock), lds, st, a, f->dimage.get(),
                               f->dsrc.get(), f->dpcum.get(), f->docc0.get(), f->dwmiss.get(), f->dpartial.get(), d_states, derr);
            return MDP_OK;
        }))
        return rc;
    HIP_TRY(hipGetLastError());
    return MDP_OK;
}

// one simulation (k_future or k_future_wide, + k_future_sum) into d_counts on stream st
int fut_launch(mdp_future *f, uint64_t seed, uint64_t rep0, uint64_t nrep, uint32_t tfut,
               unsigned long long *d_counts, hipStream_t st, bool sum, uint32_t *derr)
{
    const int nwg = fut_grid(f, nrep);
    if (f->np) {
        if (int rc = fut_launch_wide(f, seed, rep0, nrep, tfut, st, nullptr, derr)) return rc;
    } else {
        const FutArgs a = fut_args(f, seed, rep0, nrep, tfut);
        const size_t lds = (size_t)tfut * sizeof(uint32_t) + (f->nm == kTabN ? sizeof(double) * (kTabN << kTabN) : 0);
        if (int rc = dev_for_padded(f->nm, [&](auto NM) {
                hipLaunchKernelGGL(k_future<decltype(NM)::value>, dim3(nwg), dim3(kFutBlock), lds, st, a, f->dMK.get(),
                                   f->dsrc.get(), f->dpcum.get(), f->dmiss.get(), f->dT.get(), f->dpartial.get(), derr);
                return MDP_OK;
            }))
            return rc;
        HIP_TRY(hipGetLastError());
    }
    if (sum) {
        hipLaunchKernelGGL(k_future_sum, dim3(tfut), dim3(256), 0, st, f->dpartial.get(), (uint32_t)nwg, tfut, d_counts);
        HIP_TRY(hipGetLastError());
    }
    return MDP_OK;
}

int fut_check_args(mdp_future *f, uint64_t nrep, uint32_t tfut)
{
    if (!f) return mdp_set_error(MDP_EINVAL, "null future engine");
    if (tfut == 0 || tfut > kFutMaxT)
        return mdp_set_error(MDP_EUNSUPPORTED, "duration %u outside 1..%u years", tfut, kFutMaxT);
    if (nrep > (1ull << 62)) return mdp_set_error(MDP_EINVAL, "replicate count too large");
    return MDP_OK;
}

// the whole summary of replicates [rep0, rep0 + nrep) into f->dtab.get() on st:
// the table zeroed, then for every range of p.reps replicates one launch per
// window of years
int fut_summary_run(mdp_future *f, const FutSumPlan &p, uint64_t seed, uint64_t rep0, uint64_t nrep, uint32_t tfut,
                    hipStream_t st, uint32_t *derr)
{
    const size_t ncell = (size_t)tfut * (2 * f->n + 1);
    HIP_TRY(hipMemsetAsync(f->dtab.get(), 0, ncell * sizeof(unsigned long long), st));
    const uint64_t per = fut_per_wg(f);
    const size_t lds = (size_t)p.lds;
    for (uint64_t done = 0; done < nrep; done += p.reps) {
        const uint64_t cnt = std::min<uint64_t>(p.reps, nrep - done);
        const int nwg = (int)std::min<uint64_t>((cnt + per - 1) / per, p.maxwg);
        for (uint32_t t0 = 0; t0 < tfut; t0 += p.years) {
            FutSumWin w{};
            w.t0 = t0;
            w.t1 = std::min(tfut, t0 + p.years);
            w.cells = p.cells;
            w.last = w.t1 == tfut;
            int rc;
            if (f->np) {
                const FutWideArgs a = fut_wide_args(f, seed, rep0 + done, cnt, tfut);
                rc = dev_for_pairs(f->np, [&](auto NP) {
                    hipLaunchKernelGGL(k_future_wide_tab<decltype(NP)::value>, dim3(nwg), dim3(kFutBlock), lds, st, a,
                                       w, f->dimage.get(), f->dsrc.get(), f->dpcum.get(), f->docc0.get(), f->dwmiss.get(),
                                       (uint32_t *)f->drec_occ.get(), f->drec_idx.get(), f->dtab.get(), derr);
                    return MDP_OK;
                });
            } else {
                const FutArgs a = fut_args(f, seed, rep0 + done, cnt, tfut);
                rc = dev_for_padded(f->nm, [&](auto NM) {
                    hipLaunchKernelGGL(k_future_tab<decltype(NM)::value>, dim3(nwg), dim3(kFutBlock), lds, st, a, w,
                                       f->dMK.get(), f->dsrc.get(), f->dpcum.get(), f->dmiss.get(), f->dT.get(), (uint64_t *)f->drec_occ.get(),
                                       f->drec_idx.get(), f->dtab.get(), derr);
                    return MDP_OK;
                });
            }
            if (rc) return rc;
            HIP_TRY(hipGetLastError());
        }
    }
    return MDP_OK;
}

// refusals (no device call), then the table and, for more than one window,
// the records of p.reps replicates at the most
int fut_summary_prepare(mdp_future *f, uint64_t nrep, uint32_t tfut, FutSumPlan *p)
{
    if (!f) return mdp_set_error(MDP_EINVAL, "null future engine");
    if (nrep > (1ull << 62)) return mdp_set_error(MDP_EINVAL, "replicate count too large");
    if (int rc = fut_sum_plan(f->n, f->np, f->wlen, tfut, f->sum_years, p)) return rc;
    HIP_TRY(hipSetDevice(f->device));
    if (int rc = f->dtab.grow((size_t)tfut * (2 * f->n + 1))) return rc;
    const size_t recs = p->windows > 1 ? (size_t)std::min<uint64_t>(nrep, p->reps) : 0;
    if (int rc = f->drec_occ.grow(recs * (f->np ? 32 : 1))) return rc;
    return f->drec_idx.grow(recs);
}

// tables, colonisation table, look-back flags, stream and events of an engine
// whose host fields are set
int fut_device_setup(mdp_future *f, const FutLanePlan &lp, const FutWidePlan &wp, const FutPostPlan &pp)
{
    const int device = f->device;
    if (hipSetDevice(device) != hipSuccess) return mdp_set_error(MDP_EHIP, "hipSetDevice(%d) failed", device);
    f->opened = true;  // (not DevQueue::open(): this engine's own results for a bad device)
    int rc;
    if ((rc = f->dpcum.assign(pp.pcum))) return rc;
    if (f->np) {
        if ((rc = f->dimage.assign(wp.image)) || (rc = f->dsrc.assign(wp.src)) ||
            (rc = f->docc0.assign(wp.occ0)) || (rc = f->dwmiss.assign(wp.miss)))
            return rc;
        // the image and kFutMaxT year counters pass 64 KB of dynamic LDS; the
        // summary kernel: the image and one window's table
        const size_t lds[2] = {fut_wide_lds(f, kFutMaxT), (size_t)2 * f->wlen * sizeof(double) + kFutSumTableBytes};
        const void *fn[2] = {nullptr, nullptr};
        if ((rc = dev_for_pairs(f->np, [&](auto NP) {
                 fn[0] = (const void *)k_future_wide<decltype(NP)::value>;
                 fn[1] = (const void *)k_future_wide_tab<decltype(NP)::value>;
                 return MDP_OK;
             })))
            return rc;
        for (int i = 0; i < 2; ++i)
            if (hipFuncSetAttribute(fn[i], hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds[i]) != hipSuccess)
                return mdp_set_error(MDP_EHIP, "%s: %zu bytes of LDS refused on device %d%s", f->kname, lds[i], device,
                                     i ? " (summary)" : "");
    } else {
        if ((rc = f->dMK.assign(lp.MK)) || (rc = f->dsrc.assign(lp.src)) || (rc = f->dmiss.assign(lp.miss)))
            return rc;
        if (f->nm == kTabN) {
            if ((rc = f->dT.grow((size_t)kTabN << kTabN))) return rc;
            hipLaunchKernelGGL(k_future_table, dim3((kTabN << kTabN) / 256), dim3(256), 0, nullptr, f->dMK.get(), f->dsrc.get(),
                               f->n, f->dT.get());
            if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)
                return mdp_set_error(MDP_EHIP, "colonisation table kernel failed on device %d", device);
        }
    }
    // look-back overflow flags: [0] the device path (read and cleared by
    // mdp_future_check), [1] the host-returning calls (their own)
    if ((rc = f->derr.grow(2))) return rc;
    if (hipMemset(f->derr.get(), 0, 2 * sizeof(uint32_t)) != hipSuccess ||
        hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&f->ev0) != hipSuccess || hipEventCreate(&f->ev1) != hipSuccess)
        return mdp_set_error(MDP_EHIP, "device setup failed on device %d", device);
    return MDP_OK;
}

}  // namespace

extern "C" {

// mdp_future_create (mode kFutWideOff) and mdp_future_create_opts: select the
// kernel, plan, upload, set attributes.  Every refusal of an argument comes
// before the engine exists and before the first HIP call.
static int fut_create(const int32_t *last_row, uint32_t n, const double *post, uint32_t necstep, double m, double d,
                      double KD, double KS, double dS, int device, FutWideMode mode, uint32_t sum_years,
                      mdp_future **out)
{
    if (!last_row || !out || n == 0) return mdp_set_error(MDP_EINVAL, "empty survey row");
    uint32_t np = 0;
    if (int rc = fut_select_kernel(n, mode, &np)) return rc;
    if (necstep > 0 && !post) return mdp_set_error(MDP_EINVAL, "null posterior");
    if (!(KD >= 0) || !std::isfinite(KD) || !(KS >= 0) || !std::isfinite(KS))
        return mdp_set_error(MDP_EINVAL, "-D and -S must be finite and >= 0");
    if (!(m > 0) && !(m < 0)) return mdp_set_error(MDP_EINVAL, "mean dispersal -m must be non-zero");
    FutLanePlan lp;
    FutWidePlan wp;
    FutPostPlan pp;
    if (int rc = np ? fut_wide_plan(last_row, n, np, m, d, KD, KS, dS, &wp)
                    : fut_lane_plan(last_row, n, m, d, KD, KS, dS, &lp))
        return rc;
    if (int rc = fut_post_plan(post, necstep, &pp)) return rc;
    // from here the engine owns what it holds: destroyed on every exit but the last
    std::unique_ptr<mdp_future> f(new (std::nothrow) mdp_future());
    if (!f) return mdp_set_error(MDP_ENOMEM, "out of host memory");
    f->device = device;
    f->n = n;
    f->nm = fut_lane_nm(n);
    f->np = np;
    f->sum_years = sum_years;
    f->K = KD;
    f->necstep = necstep;
    f->lvalid = pp.lvalid;
    f->pscale = pp.pscale;
    if (np) {
        snprintf(f->kname, sizeof f->kname, "k_future_wide<%u>", np);
        f->nmiss = wp.nmiss;
        f->wlen = wp.len;
        f->ks0 = KS == 0;
    } else {
        snprintf(f->kname, sizeof f->kname, "k_future<%u>", f->nm);
        f->nmiss = lp.nmiss;
        f->occ0 = lp.occ0;
    }
    if (int rc = fut_device_setup(f.get(), lp, wp, pp)) return rc;
    *out = f.release();
    return MDP_OK;
}

int mdp_future_create(const int32_t *last_row, uint32_t n, const double *post, uint32_t necstep, double m,
                      double d, double KD, double KS, double dS, int device, mdp_future **out)
{
    return fut_create(last_row, n, post, necstep, m, d, KD, KS, dS, device, kFutWideOff, 0, out);
}

int mdp_future_create_opts(const int32_t *last_row, uint32_t n, const double *post, uint32_t necstep, double m,
                           double d, double KD, double KS, double dS, int device, const char *opts,
                           mdp_future **out)
{
    FutWideMode mode;
    uint32_t sum_years;
    if (int rc = fut_parse_opts(opts, &mode, &sum_years)) return rc;
    return fut_create(last_row, n, post, necstep, m, d, KD, KS, dS, device, mode, sum_years, out);
}

const char *mdp_future_kernel(const mdp_future *f) { return f ? f->kname : ""; }

int mdp_future_states(mdp_future *f, uint64_t seed, uint64_t rep0, uint64_t nrep, uint32_t tfut, uint64_t *words)
{
    if (!f) return mdp_set_error(MDP_EINVAL, "null future engine");
    if (!f->np)
        return mdp_set_error(MDP_EUNSUPPORTED, "%s keeps no replicate states: create the engine with "
                             "MDP_FUT_WIDE=1 (or auto beyond 64 patches)", f->kname);
    if (tfut > kFutMaxT) return mdp_set_error(MDP_EUNSUPPORTED, "duration %u outside 0..%u years", tfut, kFutMaxT);
    const uint32_t W = (f->n + 63) / 64;
    if (nrep > kFutStatesMaxWords / W)
        return mdp_set_error(MDP_EUNSUPPORTED, "%llu replicates x %u words: mdp_future_states returns at most %llu "
                             "words per call", (unsigned long long)nrep, W, (unsigned long long)kFutStatesMaxWords);
    if (nrep == 0) return MDP_OK;
    if (!words) return mdp_set_error(MDP_EINVAL, "null states");
    HIP_TRY(hipSetDevice(f->device));
    int rc;
    if ((rc = f->settle())) return rc;  // (mdp_future: the stream rule)
    if ((rc = fut_reserve(f, fut_grid(f, nrep), tfut))) return rc;
    if ((rc = f->dstates.grow((size_t)nrep * 64))) return rc;
    HIP_TRY(hipMemsetAsync(f->derr.get() + 1, 0, sizeof(uint32_t), f->stream));
    if ((rc = fut_launch_wide(f, seed, rep0, nrep, tfut, f->stream, f->dstates.get(), f->derr.get() + 1))) return rc;
    std::vector<uint32_t> lanes((size_t)nrep * 64);
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(lanes.data(), f->dstates.get(), lanes.size() * sizeof(uint32_t), hipMemcpyDeviceToHost,
                           f->stream));
    HIP_TRY(hipMemcpyAsync(&err, f->derr.get() + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));
    if ((rc = fut_lookback(err, false))) return rc;
    fut_wide_unpack(lanes.data(), nrep, f->n, f->np, words);
    return MDP_OK;
}

void mdp_future_destroy(mdp_future *f)
{
    delete f;  // (its destructor releases the device side)
}

int mdp_future_simulate_device(mdp_future *f, uint64_t seed, uint64_t rep0, uint64_t nrep, uint32_t tfut,
                               uint64_t *d_counts, void *stream)
{
    int rc = fut_check_args(f, nrep, tfut);
    if (rc) return rc;
    if (!d_counts) return mdp_set_error(MDP_EINVAL, "null device counts");
    HIP_TRY(hipSetDevice(f->device));
    hipStream_t st = (hipStream_t)stream;  // as given: NULL is HIP's null stream
    if ((rc = f->settle_unless(st))) return rc;
    if ((rc = fut_reserve(f, fut_grid(f, nrep), tfut))) return rc;
    f->launched_on(st);
    // the look-back overflow flag is sticky: mdp_future_check reads and
    // clears it, so one check covers every launch since the previous check
    return fut_launch(f, seed, rep0, nrep, tfut, (unsigned long long *)d_counts, st, true, f->derr.get());
}

int mdp_future_check(mdp_future *f, void *stream)
{
    if (!f) return mdp_set_error(MDP_EINVAL, "null future engine");
    HIP_TRY(hipSetDevice(f->device));
    hipStream_t st = (hipStream_t)stream;
    // (the launches it covers are those on st; one pending elsewhere is waited
    // for, so that its flag is read too rather than cleared under it)
    if (int rc = f->settle_unless(st)) return rc;
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, f->derr.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemsetAsync(f->derr.get(), 0, sizeof(uint32_t), st));
    HIP_TRY(hipStreamSynchronize(st));
    f->waited_for(st);
    return fut_lookback(err, true);
}

int mdp_future_simulate(mdp_future *f, uint64_t seed, uint64_t rep0, uint64_t nrep, uint32_t tfut,
                        uint64_t *counts)
{
    int rc = fut_check_args(f, nrep, tfut);
    if (rc) return rc;
    if (!counts) return mdp_set_error(MDP_EINVAL, "null counts");
    HIP_TRY(hipSetDevice(f->device));
    if ((rc = f->settle())) return rc;  // (mdp_future: the stream rule)
    if ((rc = fut_reserve(f, fut_grid(f, nrep), tfut))) return rc;
    if (nrep == 0) return MDP_OK;
    HIP_TRY(hipMemsetAsync(f->derr.get() + 1, 0, sizeof(uint32_t), f->stream));
    if ((rc = fut_launch(f, seed, rep0, nrep, tfut, f->dcounts.get(), f->stream, true, f->derr.get() + 1))) return rc;
    std::vector<unsigned long long> h(tfut);
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(h.data(), f->dcounts.get(), tfut * sizeof(unsigned long long), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(hipMemcpyAsync(&err, f->derr.get() + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));
    if ((rc = fut_lookback(err, false))) return rc;
    for (uint32_t t = 0; t < tfut; ++t) counts[t] += h[t];
    return MDP_OK;
}

int mdp_future_time_kernel(mdp_future *f, uint64_t seed, uint64_t nrep, uint32_t tfut, int reps, double *ms)
{
    int rc = fut_check_args(f, nrep, tfut);
    if (rc) return rc;
    if (!ms || reps <= 0 || nrep == 0) return mdp_set_error(MDP_EINVAL, "bad timing request");
    HIP_TRY(hipSetDevice(f->device));
    if ((rc = f->settle())) return rc;  // (mdp_future: the stream rule)
    if ((rc = fut_reserve(f, fut_grid(f, nrep), tfut))) return rc;
    auto launch = [&]() {
        return fut_launch(f, seed, 0, nrep, tfut, f->dcounts.get(), f->stream, false, f->derr.get() + 1);
    };
    if ((rc = launch())) return rc;  // warm-up
    return f->time(f->stream, reps, ms, launch);
}

int mdp_future_summary_device(mdp_future *f, uint64_t seed, uint64_t rep0, uint64_t nrep, uint32_t tfut,
                              uint64_t *d_hist, uint64_t *d_occ, void *stream)
{
    if (!d_hist && !d_occ) return mdp_set_error(MDP_EINVAL, "null hist and occ");
    FutSumPlan p;
    int rc = fut_summary_prepare(f, nrep, tfut, &p);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;  // as given: NULL is HIP's null stream
    if ((rc = f->settle_unless(st))) return rc;
    f->launched_on(st);
    // the sticky look-back flag of the device path (mdp_future_check)
    if ((rc = fut_summary_run(f, p, seed, rep0, nrep, tfut, st, f->derr.get()))) return rc;
    const uint32_t ncell = tfut * (2 * f->n + 1);
    hipLaunchKernelGGL(k_future_split, dim3((ncell + 255) / 256), dim3(256), 0, st, f->dtab.get(), ncell, f->n,
                       (unsigned long long *)d_hist, (unsigned long long *)d_occ);
    HIP_TRY(hipGetLastError());
    return MDP_OK;
}

int mdp_future_summary(mdp_future *f, uint64_t seed, uint64_t rep0, uint64_t nrep, uint32_t tfut, uint64_t *hist,
                       uint64_t *occ)
{
    if (!hist && !occ) return mdp_set_error(MDP_EINVAL, "null hist and occ");
    FutSumPlan p;
    int rc = fut_summary_prepare(f, nrep, tfut, &p);
    if (rc) return rc;
    if (nrep == 0) return MDP_OK;
    if ((rc = f->settle())) return rc;  // (mdp_future: the stream rule)
    HIP_TRY(hipMemsetAsync(f->derr.get() + 1, 0, sizeof(uint32_t), f->stream));
    if ((rc = fut_summary_run(f, p, seed, rep0, nrep, tfut, f->stream, f->derr.get() + 1))) return rc;
    const uint32_t n = f->n, cells = 2 * n + 1;
    std::vector<unsigned long long> h((size_t)tfut * cells);
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(h.data(), f->dtab.get(), h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(hipMemcpyAsync(&err, f->derr.get() + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));
    if ((rc = fut_lookback(err, false))) return rc;
    for (uint32_t t = 0; t < tfut; ++t) {
        const unsigned long long *row = h.data() + (size_t)t * cells;
        for (uint32_t m = 0; hist && m <= n; ++m) hist[(size_t)t * (n + 1) + m] += row[m];
        for (uint32_t k = 0; occ && k < n; ++k) occ[(size_t)t * n + k] += row[n + 1 + k];
    }
    return MDP_OK;
}

int mdp_future_time_summary(mdp_future *f, uint64_t seed, uint64_t nrep, uint32_t tfut, int reps, double *ms)
{
    FutSumPlan p;
    int rc = fut_summary_prepare(f, nrep, tfut, &p);
    if (rc) return rc;
    if (!ms || reps <= 0 || nrep == 0) return mdp_set_error(MDP_EINVAL, "bad timing request");
    if ((rc = f->settle())) return rc;  // (mdp_future: the stream rule)
    auto launch = [&]() { return fut_summary_run(f, p, seed, 0, nrep, tfut, f->stream, f->derr.get() + 1); };
    if ((rc = launch())) return rc;  // warm-up
    return f->time(f->stream, reps, ms, launch);
}

int mdp_future_philox(uint64_t key, const uint32_t *ctr, uint32_t *out)
{
    // host restatement of the device generator, for known-answer tests of the
    // stream definition (the device path is checked through the counts)
    if (!ctr || !out) return mdp_set_error(MDP_EINVAL, "null pointer");
    uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
    uint32_t x = ctr[0], y = ctr[1], z = ctr[2], w = ctr[3];
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * x, p1 = (uint64_t)0xCD9E8D57u * z;
        const uint32_t nx = (uint32_t)(p1 >> 32) ^ y ^ k0, ny = (uint32_t)p1;
        const uint32_t nz = (uint32_t)(p0 >> 32) ^ w ^ k1, nw = (uint32_t)p0;
        x = nx, y = ny, z = nz, w = nw;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = x, out[1] = y, out[2] = z, out[3] = w;
    return MDP_OK;
}

}  // extern "C"