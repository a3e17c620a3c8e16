// midaspom_amd/csrc/spom_sim_year.h -- the model's year, stated once for the
// three simulation units (spom_future.hip, spom_scnsim.hip, spom_scnchain.hip):
//   lane_year<NM>  one replicate per lane, the occupancy a 64-bit mask
//                  (k_future_tab, k_scnsim, k_scnchain);
//   wide_year<NP>  one replicate per wave, the patches over its lanes
//                  (k_future_wide, k_future_wide_tab, k_scnsim_wave).
// Both draw the extinctions, take the colonisation sums in ascending patch
// order and draw the colonisations; the units differ in the expression of pC
// alone, which each call site passes as a callable.  So every kernel takes
// the same draws and adds the same terms in the same order.  The year is
// shared as a whole function only: handing the draws or the sums back to the
// caller changes the kernels' register allocation.
// k_future<NM> of spom_future.hip holds the lane year a second time, inline,
// for a measured reason given there.
// Device code; include after <hip/hip_runtime.h> and spom_rng.h, under
// `#pragma clang fp contract(off)`.  Internal linkage.
#ifndef SPOM_SIM_YEAR_H
#define SPOM_SIM_YEAR_H
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "spom_future_plan.h"  // fut_wide_slot0: the addressing of the distance image

namespace {

constexpr int kTabN = 8;  // NM = 8: survivor-sum table in LDS

// Ts[surv][k] = sum over l in surv, l != k, ascending, of M[l][k]: the table
// the scenario kernels' lane_year<8> reads (the future engine's includes the
// source term: k_future_table), filled by the `block` threads of a workgroup
// (the caller puts the barrier behind it)
__device__ __forceinline__ void sim_year_table(uint32_t n, const double *__restrict__ M, double *Ts, uint32_t block)
{
    for (uint32_t i = threadIdx.x; i < (1u << kTabN) * kTabN; i += block) {
        const uint32_t sv = i / kTabN, k = i % kTabN;
        double s = 0.0;
        for (uint32_t l = 0; l < n; ++l)
            if (l != k && ((sv >> l) & 1u)) s += M[l * kTabN + k];
        Ts[i] = s;
    }
}

// one year of replicate rg (simpij :64-110 of main_MIDASPOM_future.c; the
// scenario programs' dieoff.c:51-83, loss.c:52-105): the occupancy after year
// t + 1.  `a` gives the key (key0, key1) and the patch count n; t is the year
// word of the counter.  s1_k is the sum over the survivors of M[l][k] (NM = 8:
// row surv of Ts), plus bias[k] where bias is a pointer and no table is read
// (nullptr: no such term); pcol(s1_k, k) is pC before the clamp.
template <int NM, typename Args, typename Bias, typename PCol>
__device__ __forceinline__ uint64_t lane_year(const Args &a, const double *__restrict__ M, const double *Ts,
                                              uint64_t rg, uint32_t t, uint32_t npairs, uint64_t occ, double E,
                                              Bias bias, PCol pcol)
{
    uint64_t surv = 0;
    uint32_t colw[NM];
#pragma unroll
    for (int m = 0; m < NM / 2; ++m) {
        if ((uint32_t)m < npairs) {
            const u32x4 w = philox(a.key0, a.key1, u32x4{(uint32_t)rg, (uint32_t)(rg >> 32), t, (uint32_t)m});
            const uint32_t k0 = 2 * m, k1 = 2 * m + 1;
            colw[k0] = w.y >> 1;
            colw[k1] = w.w >> 1;
            // extinction: an occupied patch survives if u > E (:75-82; dieoff.c:56-64)
            if (((occ >> k0) & 1u) && u_gt(w.x >> 1, E)) surv |= 1ull << k0;
            if (((occ >> k1) & 1u) && u_gt(w.z >> 1, E)) surv |= 1ull << k1;
        } else {
            colw[2 * m] = colw[2 * m + 1] = 0;
        }
    }
    // colonisation sums, ascending l for every k (:89-95; dieoff.c:72-77)
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
            for (int k = 0; k < NM; ++k) s1[k] += on ? M[l * NM + k] : 0.0;
        }
        if constexpr (!std::is_same_v<Bias, std::nullptr_t>) {
#pragma unroll
            for (int k = 0; k < NM; ++k) s1[k] += bias[k];
        }
    }
    uint64_t nw = surv;
#pragma unroll
    for (int k = 0; k < NM; ++k) {
        if ((uint32_t)k < a.n && !((surv >> k) & 1u)) {
            double pc = pcol(s1[k], k);  // :95-97
            if (pc > 1) pc = 1;
            if (u_lt(colw[k], pc)) nw |= 1ull << k;  // :98-101
        }
    }
    return nw;
}

// the scenario kernels' lane year on the unscaled table, with the scenario's
// pressure
//   pC = (c (s1 + src_k ks)) km
// where (ks, km) = (0, 1) in a baseline year, (0, K) under die-off and (K, 1)
// under loss: adding 0.0 to s1 >= 0 and multiplying by 1.0 are exact, so each
// case is the reference's own expression and rounding.
template <int NM, typename Args>
__device__ __forceinline__ uint64_t sim_year(const Args &a, const double *__restrict__ M,
                                             const double *__restrict__ src, const double *Ts, uint64_t rg,
                                             uint32_t t, uint32_t npairs, uint64_t occ, double E, double c, double ks,
                                             double km)
{
    return lane_year<NM>(a, M, Ts, rg, t, npairs, occ, E, nullptr, [&](double s, int k) {
        const double sk = src[k] * ks;  // loss.c:95-98: the product is rounded before the add
        return (c * (s + sk)) * km;     // dieoff.c:78 (c s1) K
    });
}

// one year of the wave's replicate rg: the lane's occupancy word after year
// t + 1.  Lane `lane` owns the patch pairs m = lane + 64*j, j < NP, patch
// 2m + p in bit 2j + p of occ and of live (the patches that exist).  G2 is the
// two-sided distance image in LDS (a.len doubles per copy), src the source row
// in lane order; pcol(s_k, src_k) is pC before the clamp.
template <int NP, typename Args, typename PCol>
__device__ __forceinline__ uint32_t wide_year(const Args &a, const double2 *G2, const double *__restrict__ src,
                                              uint64_t rg, uint32_t t, uint32_t lane, uint32_t npairs, uint32_t live,
                                              uint32_t occ, double E, PCol pcol)
{
    uint64_t bal[NP][2];
    uint32_t colw[2 * NP];
    uint32_t surv = 0;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const uint32_t m = lane + 64u * j;
        bool s0 = false, s1 = false;
        colw[2 * j] = colw[2 * j + 1] = 0;
        if (m < npairs) {
            const u32x4 w = philox(a.key0, a.key1, u32x4{(uint32_t)rg, (uint32_t)(rg >> 32), t, m});
            colw[2 * j] = w.y >> 1;
            colw[2 * j + 1] = w.w >> 1;
            // extinction: an occupied patch survives if u > E (:75-82; dieoff.c:56-64)
            s0 = ((occ >> (2 * j)) & 1u) && u_gt(w.x >> 1, E);
            s1 = ((occ >> (2 * j + 1)) & 1u) && u_gt(w.z >> 1, E);
        }
        bal[j][0] = __ballot(s0);
        bal[j][1] = __ballot(s1);
        surv |= ((uint32_t)s0 << (2 * j)) | ((uint32_t)s1 << (2 * j + 1));
    }
    // colonisation sums, ascending l for every k (:89-95; dieoff.c:72-77): patch
    // l = 2*(lam + 64*j) + p ascends with j, then lam, then p
    double s[2 * NP];
#pragma unroll
    for (int k = 0; k < 2 * NP; ++k) s[k] = 0.0;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        uint64_t both = bal[j][0] | bal[j][1];
        while (both) {
            const uint32_t lam = (uint32_t)__builtin_ctzll(both);
            both &= both - 1;
#pragma unroll
            for (uint32_t p = 0; p < 2; ++p) {
                if (!((bal[j][p] >> lam) & 1u)) continue;
                const uint32_t l = 2 * (lam + 64u * j) + p;
                const double2 *row = G2 + fut_wide_slot0(a.n, a.len, l) + lane;
#pragma unroll
                for (int jj = 0; jj < NP; ++jj) {
                    const double2 v = row[64 * jj];
                    s[2 * jj] += v.x;
                    s[2 * jj + 1] += v.y;
                }
            }
        }
    }
    uint32_t nw = surv;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const double2 sv = reinterpret_cast<const double2 *>(src)[lane + 64 * j];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const uint32_t bit = 1u << (2 * j + p);
            if ((live & bit) && !(surv & bit)) {
                double pc = pcol(s[2 * j + p], p ? sv.y : sv.x);  // :95-97
                if (pc > 1) pc = 1;
                if (u_lt(colw[2 * j + p], pc)) nw |= bit;  // :98-101
            }
        }
    }
    return nw;
}

}  // namespace

#endif
