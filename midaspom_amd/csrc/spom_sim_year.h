// midaspom_amd/csrc/spom_sim_year.h -- the model year of the two simulated
// scenario engines (spom_scnsim.hip k_scnsim<NM>, spom_scnchain.hip
// k_scnchain<NM>): one text, so both kernels take the same draws and add the
// same terms in the same order.  Device code; include after
// <hip/hip_runtime.h> and spom_rng.h, under `#pragma clang fp contract(off)`.
// Internal linkage, as when the text stood in spom_scnsim.hip.
#ifndef SPOM_SIM_YEAR_H
#define SPOM_SIM_YEAR_H
#include <cstdint>

namespace {

constexpr int kTabN = 8;  // NM = 8: survivor-sum table of the unscaled M in LDS

// Ts[surv][k] = sum over l in surv, l != k, ascending, of M[l][k]: the table
// sim_year<8> reads, filled by the `block` threads of a workgroup (the caller
// puts the barrier behind it)
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

// one year of replicate rg: fut_year<NM> of spom_future.hip on the unscaled
// table, with the scenario's pressure
//   pC = (c (s1 + src_k ks)) km
// where (ks, km) = (0, 1) in a baseline year, (0, K) under die-off and (K, 1)
// under loss: adding 0.0 to s1 >= 0 and multiplying by 1.0 are exact, so each
// case is the reference's own expression and rounding.  `a` gives the key
// (key0, key1) and the patch count n; t is the year word of the counter.
template <int NM, typename Args>
__device__ __forceinline__ uint64_t sim_year(const Args &a, const double *__restrict__ M,
                                             const double *__restrict__ src, const double *Ts, uint64_t rg,
                                             uint32_t t, uint32_t npairs, uint64_t occ, double E, double c, double ks,
                                             double km)
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
            // extinction: an occupied patch survives if u > E (dieoff.c:56-64)
            if (((occ >> k0) & 1u) && u_gt(w.x >> 1, E)) surv |= 1ull << k0;
            if (((occ >> k1) & 1u) && u_gt(w.z >> 1, E)) surv |= 1ull << k1;
        } else {
            colw[2 * m] = colw[2 * m + 1] = 0;
        }
    }
    // colonisation sums, ascending l for every k (dieoff.c:72-77)
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
    }
    uint64_t nw = surv;
#pragma unroll
    for (int k = 0; k < NM; ++k) {
        if ((uint32_t)k < a.n && !((surv >> k) & 1u)) {
            const double sk = src[k] * ks;       // loss.c:95-98: the product is rounded before the add
            double pc = (c * (s1[k] + sk)) * km;  // dieoff.c:78 (c s1) K
            if (pc > 1) pc = 1;
            if (u_lt(colw[k], pc)) nw |= 1ull << k;
        }
    }
    return nw;
}

}  // namespace

#endif
