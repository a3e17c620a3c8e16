// midaspom_amd/csrc/spom_rng.h -- the addressed random stream of the two
// simulators (spom_future.hip, spom_scnsim.hip): Philox4x32-10 and the exact
// comparison of a 31-bit draw with a double threshold.  Device code; include
// after <hip/hip_runtime.h>.  Internal linkage, as when the text stood in
// spom_future.hip.
#ifndef SPOM_RNG_H
#define SPOM_RNG_H
#include <cstdint>

namespace {

constexpr double kRandMax = 2147483647.0;  // glibc RAND_MAX

// Philox4x32-10 (Salmon et al., SC'11), the Random123 constants.
struct u32x4 {
    uint32_t x, y, z, w;
};

__device__ __forceinline__ u32x4 philox(uint32_t k0, uint32_t k1, u32x4 c)
{
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        // one v_mad_u64_u32 per product (instead of mul_lo + mul_hi)
        const uint64_t p0 = (uint64_t)0xD2511F53u * c.x, p1 = (uint64_t)0xCD9E8D57u * c.z;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        c = u32x4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// The reference compares u = (double)r / (double)RAND_MAX with a threshold
// (u > E, u < pC).  r * fl(1/RAND_MAX) is within 3.4e-16 of fl(r/RAND_MAX)
// (both within ~1.2 ulp of r/RAND_MAX <= 1), so outside a 1e-15 band around
// the threshold the product decides the comparison; inside it the exact
// correctly rounded quotient does.  Bit-identical outcomes, ~never divides.
constexpr double kInvRandMax = 1.0 / 2147483647.0;
constexpr double kBand = 1e-15;

__device__ __forceinline__ bool u_gt(uint32_t r, double x)  // fl(r/R) > x
{
    const double q = (double)r * kInvRandMax;
    if (q > x + kBand) return true;
    if (q < x - kBand) return false;
    return (double)r / kRandMax > x;
}

__device__ __forceinline__ bool u_lt(uint32_t r, double x)  // fl(r/R) < x
{
    const double q = (double)r * kInvRandMax;
    if (q < x - kBand) return true;
    if (q > x + kBand) return false;
    return (double)r / kRandMax < x;
}

}  // namespace

#endif
