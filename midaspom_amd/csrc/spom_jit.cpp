// midaspom_amd/csrc/spom_jit.cpp -- problem-specialised forward kernel: the
// generator of its source.
//
// The forward recursion of the reference (main_MIDASPOM.c:368-392) has a
// control structure fixed by the observation file alone: the number of
// possible states in each year.  At engine creation we emit it as
// straight-line HIP source -- one block per year, every transition's
// coefficient block at a compile-time LDS offset -- and compile it for gfx950
// with hipRTC (spom_jit_rtc.cpp).  With no data-dependent branches left, the
// compiler can issue the LDS reads of later transitions under the arithmetic
// of earlier ones; the runtime-shape kernels in spom_engine.hip serialise on
// every general year instead.
//
// This unit is host code alone (no HIP runtime, no hipRTC): a plan goes in,
// text comes out.  The text is emitted by one Emitter per source, a member
// function per stage of the kernel, in the kernel's own order:
//   defines, REVQ | signature, shared front | staging (Q row, gathered chunk
//   or the fused prologue) | point set-up | forward body | kernel end
#include <algorithm>
#include <cstdint>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "spom_jit.h"

namespace {

const char *kPrelude = R"SRC(
typedef unsigned int u32;
// log x = k ln2 + log m, x = 2^k m with m in [sqrt(1/2), sqrt(2)): log m =
// 2 atanh(s), s = (m - 1) / (m + 1), |s| <= 0.1716, the odd series to s^21
// (remainder below 2^-62 of the sum).  About 20 FP64 operations and no
// table, a fraction of the library log's cost; within 2 ulp of it
// (tests/test_gpu_parity.py::test_engine_log_accuracy).
__device__ __forceinline__ double mdp_log(double x)
{
    if (!(x > 0.0) || x == __builtin_inf()) return x == 0.0 ? -__builtin_inf() : (x > 0.0 ? x : __builtin_nan(""));
    int k = 0;
    if (x < 0x1p-1022) {  // subnormal: scale into the normal range
        x *= 0x1p54;
        k = -54;
    }
    const unsigned long long ix = (unsigned long long)__double_as_longlong(x);
    k += (int)(ix >> 52) - 1023;
    double m = __longlong_as_double((long long)((ix & 0x000fffffffffffffull) | 0x3ff0000000000000ull));
    if (m > 1.4142135623730951) {
        m *= 0.5;
        ++k;
    }
    const double f = m - 1.0, d = m + 1.0;
    double r = __builtin_amdgcn_rcp(d);  // 1 / d: one Newton step, then a corrected quotient
    r = fma(fma(-d, r, 1.0), r, r);
    double s = f * r;
    s = fma(fma(-d, s, f), r, s);
    const double z = s * s;
    double p = 1.0 / 21.0;
    p = fma(p, z, 1.0 / 19.0);
    p = fma(p, z, 1.0 / 17.0);
    p = fma(p, z, 1.0 / 15.0);
    p = fma(p, z, 1.0 / 13.0);
    p = fma(p, z, 1.0 / 11.0);
    p = fma(p, z, 1.0 / 9.0);
    p = fma(p, z, 1.0 / 7.0);
    p = fma(p, z, 1.0 / 5.0);
    p = fma(p, z, 1.0 / 3.0);
    const double lm = fma(2.0 * s, z * p, 2.0 * s);  // 2 s (1 + z p)
    const double kd = (double)k;
    return fma(kd, 0x1.62e42fefa39efp-1, fma(kd, 0x1.abc9e3b39803fp-56, lm));
}
)SRC";

// The transition P[a][b](e, c) = sum_m Q_ab[m](c) x^(|A|-m) y^m (x = min(e, 1),
// y = 1 - x) is evaluated per point without a weight table, in
// one of two ratio forms chosen per lane:
//   t-form (x >= y): P = x^|A| * H_t,              H_t = sum_m Q[m] t^m,      t = y / x <= 1
//   s-form (x <  y): P = y^|A| * s^(|A|-nX) * H_s, H_s = sum_m Q[m] s^(nX-m), s = x / y <  1
// Both are one Horner chain of nX FMAs over the group's coefficients -- the
// s-form reads them in stored order, the t-form reversed (a second, reversed
// copy of the Q row sits in LDS, so the choice is a per-lane base address).
// Writing B = x (t) or y (s) and g = 1 (t) or s (s):  P = B^|A| g^(|A|-nX) H.
// The factor g^d (d = |A| - nX = |A \ B|, the patches forced extinct) is a
// multiply per transition when d > 0; B^|A| depends only on the source state,
// so it is deferred: every state of a year carries the same pending exponent
// E of B (sources of a year with |A| above the year's minimum are scaled by
// B^(|A| - min) first), applied when E passes kFlushExp and at the end.
// The deferred values are bounded: H <= sum_m Q[m] <= 2^nX <= 2^|A| with both
// ratios <= 1 and B >= 1/2 for e in [0, 1] (B > 1 for e < 0, where nothing
// grows), so a state is at most 2^E np0 times its true value and B^E >= 2^-E.
constexpr uint32_t kFlushExp = 192;

// a use descriptor's fields: the Q offset, nX and |A|
constexpr uint32_t kOffM = (1u << 22) - 1u;
inline uint32_t use_off(uint32_t d) { return d & kOffM; }
inline uint32_t use_nx(uint32_t d) { return (d >> 22) & 31u; }
inline uint32_t use_na(uint32_t d) { return d >> 27; }

struct Schedule {
    std::vector<uint32_t> amin;          // per year t >= 1: min |A| over the year's sources
    std::vector<std::vector<uint32_t>> diff;  // per year: |A_k| - amin per source k
    std::vector<uint32_t> flush;         // per year: pending exponent applied after it (0: none)
    uint32_t final_exp = 0;              // pending exponent at the end of the program
    uint32_t dp = 0, dg = 0;             // largest source pre-scale and g exponent used
};

Schedule schedule(const MdpJitPlan &pl)
{
    Schedule sc;
    sc.amin.assign(pl.np.size(), 0);
    sc.diff.assign(pl.np.size(), {});
    sc.flush.assign(pl.np.size(), 0);
    uint32_t E = pl.e0;
    size_t u = 0;
    for (size_t t = 1; t < pl.np.size(); ++t) {
        const uint32_t npp = pl.np[t - 1], npc = pl.np[t];
        std::vector<uint32_t> a(npp, 0);
        for (uint32_t l = 0; l < npc; ++l)
            for (uint32_t k = 0; k < npp; ++k) {
                const uint32_t d = pl.udesc[u + (size_t)l * npp + k];
                const uint32_t nX = use_nx(d), nA = use_na(d);
                a[k] = nA;  // a use's |A| is its source's
                if (nA > nX) sc.dg = std::max(sc.dg, nA - nX);
            }
        u += (size_t)npp * npc;
        const uint32_t am = *std::min_element(a.begin(), a.end());
        sc.amin[t] = am;
        for (uint32_t k = 0; k < npp; ++k) {
            sc.diff[t].push_back(a[k] - am);
            sc.dp = std::max(sc.dp, a[k] - am);
        }
        E += am;
        if (E >= kFlushExp) {
            sc.flush[t] = E;
            E = 0;
        }
    }
    sc.final_exp = E;
    return sc;
}

// B^E (or g^E) for point i as straight-line code: binary powers of `base`
std::string power_expr(const std::string &base, uint32_t E, const std::string &tmp)
{
    if (E == 0) return "1.0";
    std::ostringstream o;
    o << "[&]() { double " << tmp << "_s = " << base << ", " << tmp << "_f = 1.0;";
    bool first = true;
    for (uint32_t b = E; b; b >>= 1) {
        if (!first) o << " " << tmp << "_s *= " << tmp << "_s;";
        if (b & 1u) o << " " << tmp << "_f = " << (first ? tmp + "_s;" : tmp + "_f * " + tmp + "_s;");
        first = false;
    }
    o << " return " << tmp << "_f; }()";
    return o.str();
}

// The fused kernel's Q-entry sum in the canonical order of spom_engine.hip
// (kQGroup = 8: the items in groups of eight summed left to right, the group
// sums as a pairwise tree over the entry's groups: a binary counter folded
// from its lowest occupied level up).  Every gather is unconditional: slots
// past the entry's count read the zero slot pl[NITEMS] (set in the Pc
// phase), so all loads are in flight at once instead of one branch and wait
// per item.  The groups and the tree then run over the compile-time bound
// (groups of zeros past the entry, a tree padded to a power of two); every
// padded addition is x + (+0.0) = x for the non-negative (or NaN / inf) sums
// here, so the bits are those of the canonical order.  Sets `a`.
std::string qsum_flat_code(uint32_t qml, uint32_t qun)
{
    const uint32_t G = 8, ngm = (qml + G - 1) / G;  // = kQGroup (spom_engine.h)
    uint32_t ngp = 1;
    while (ngp < ngm) ngp *= 2;
    std::ostringstream o;
    o << "            const u32 cnt_ = qn[k];\n"
         "            double p_[" << qml << "];\n";
    for (uint32_t u = 0; u < qml; ++u) {
        if (u < qun)
            o << "            p_[" << u << "] = pl[qx[k][" << u << "]];\n";
        else
            o << "            { const u32 t_ = Qil[qb[k] + " << u << "u]; p_[" << u << "] = pl[" << u
              << "u < cnt_ ? t_ : (u32)NITEMS]; }\n";
    }
    o << "            (void)cnt_;\n            double g_[" << ngp << "];\n";
    for (uint32_t g = 0; g < ngp; ++g) {
        if (g >= ngm) {
            o << "            g_[" << g << "] = 0.0;\n";
            continue;
        }
        o << "            g_[" << g << "] = p_[" << G * g << "]";
        for (uint32_t u = 1; u < G && G * g + u < qml; ++u) o << " + p_[" << G * g + u << "]";
        o << ";\n";
    }
    for (uint32_t w = ngp; w > 1; w /= 2)
        for (uint32_t i = 0; i < w / 2; ++i)
            o << "            g_[" << i << "] = g_[" << 2 * i << "] + g_[" << 2 * i + 1 << "];\n";
    o << "            const double a = g_[0];\n";
    return o.str();
}

}  // namespace

MdpRatioWork mdp_jit_ratio_work(const MdpJitPlan &pl)
{
    MdpRatioWork w;
    if (pl.np.empty()) return w;
    const Schedule sch = schedule(pl);
    // B^E by squaring: floor(log2 E) squarings + popcount(E) - 1 products
    auto powcost = [](uint32_t E) -> double {
        if (E <= 1) return 0.0;
        return (double)(31 - __builtin_clz(E)) + (double)__builtin_popcount(E) - 1.0;
    };
    w.setup_t = 2.0 + (sch.dp > 1 ? sch.dp - 1.0 : 0.0);
    w.setup_s = w.setup_t + (sch.dg > 1 ? sch.dg - 1.0 : 0.0);
    std::set<uint32_t> groups, gd;
    for (uint32_t d : pl.udesc) {
        const uint32_t off = use_off(d), nX = use_nx(d), nA = use_na(d);
        if (groups.insert(off).second) {
            w.use_s += 2.0 * nX;
            w.use_t += 2.0 * nX;
        }
        if (nA > nX && gd.insert(off | (nA - nX) << 22).second) w.use_s += 1.0;
    }
    double yr = 0.0;
    for (size_t t = 1; t < pl.np.size(); ++t) {
        const double npp = pl.np[t - 1], npc = pl.np[t];
        yr += npc * (2.0 * npp - 1.0);
        for (uint32_t df : sch.diff[t]) yr += df ? 1.0 : 0.0;
        if (sch.flush[t]) yr += npc + powcost(sch.flush[t]);
    }
    w.use_s += yr;
    w.use_t += yr;
    w.final_pt = (double)pl.np.back() + 1.0 + (sch.final_exp ? powcost(sch.final_exp) + 1.0 : 0.0);
    return w;
}

int mdp_jit_default_epl(const std::vector<uint32_t> &) { return 2; }

// reversed-copy index of every coefficient slot: within each group (offset,
// nX + 1 coefficients) slot off + k holds coefficient off + nX - k; slots of
// no used group map to themselves
std::vector<uint32_t> mdp_jit_reversed_index(const std::vector<uint32_t> &udesc, size_t ldq)
{
    std::vector<uint32_t> rev(ldq);
    for (size_t i = 0; i < ldq; ++i) rev[i] = (uint32_t)i;
    for (uint32_t d : udesc) {
        const uint32_t off = use_off(d), nX = use_nx(d);
        for (uint32_t k = 0; k <= nX && off + k < ldq; ++k) rev[off + k] = off + nX - k;
    }
    return rev;
}

uint32_t mdp_jit_end_exp(const MdpJitPlan &plan) { return schedule(plan).final_exp; }

namespace {

// ---- plan-independent kernel text -----------------------------------------

// The front of the kernel is one dependent chain of memory round trips if it
// is written the obvious way, so its order is fixed: each variant issues the
// loads its first barrier waits for (the staging loads) first, then this
// front, then its stores.  No load ahead of the first barrier sits in an
// exec-masked branch (the compiler drains vmcnt at each one's join): an index
// past the end is clamped and the value selected afterwards.
//
// (1) This lane's points.  One point per lane (kFrontPoint): e row
// by * KBLOCK + tid.  Several (kFrontList): list positions
// pp = by * KBLOCK * EPL + tid * EPL + i, each naming an e row (plist; bit 31:
// a duplicate that computes but does not store), the host's list putting only
// points of one ratio form in a lane (set_grid_dev) so that they share their
// coefficient reads.  No list is the identity, which a sorted grid with an
// even number of s-form rows is.  With a list `evals` holds e by list
// position, then e[0] (what the row 0 of a position past the list reads), so
// the e load never waits for the list's: the rows (needed for the flags and
// the final store) are read beside it in a workgroup-uniform branch.
const char *kFrontDecl = R"HIP(    u32 ie[EPL], pp[EPL];
    bool st[EPL];
    double ev[EPL];
)HIP";
const char *kFrontPoint = R"HIP(    pp[0] = by * KBLOCK + tip;
    ie[0] = pp[0];
    st[0] = ie[0] < ne;
    ev[0] = evals[st[0] ? ie[0] : 0u];
)HIP";
const char *kFrontList = R"HIP(    u32 q_[EPL];
#pragma unroll
    for (int i = 0; i < EPL; ++i) {
        pp[i] = by * (KBLOCK * EPL) + tip * EPL + i;
        q_[i] = pp[i] < nlist ? pp[i] : 0x80000000u;
        const u32 j_ = q_[i] & 0x7fffffffu;
        ev[i] = evals[plist ? (pp[i] < nlist ? pp[i] : nlist) : (j_ < ne ? j_ : 0u)];
    }
    if (plist) {
#pragma unroll
        for (int i = 0; i < EPL; ++i) {
            const u32 l_ = plist[pp[i] < nlist ? pp[i] : 0u];
            q_[i] = pp[i] < nlist ? l_ : 0x80000000u;
        }
    }
#pragma unroll
    for (int i = 0; i < EPL; ++i) {
        ie[i] = q_[i] & 0x7fffffffu;
        st[i] = !(q_[i] >> 31) && ie[i] < ne;
    }
)HIP";
// (2) What only the rest of the kernel reads, held in registers from here on,
// while the staging loads are in flight: an argument first read after a
// barrier is a scalar round trip every wave of the block waits for.  (Inputs
// only: a pointer that came out of an asm statement would lose its address
// space, and its loads and stores would turn flat.)
const char *kFrontLate = R"HIP(#pragma unroll
    for (int i = 0; i < EPL; ++i) ev[i] = ie[i] < ne ? ev[i] : 0.0;
    asm volatile("" :: "s"(kmax), "s"(one), "s"(out), "s"(ld_out), "s"(out_cs), "s"(prior0), "s"(vscr), "s"(ldv));
)HIP";

// Per point: the ratio form (lane-uniform: every point of a lane has one form
// -- the host list -- so point 0 decides), the ratio z, the deferred base B,
// g, and the power tables bp[k] = B^k (source pre-scales, k <= DP) and
// gp[d] = g^d (d <= DG).  The state vector's first values follow, inside the
// second loop (Emitter::point_setup closes it).
const char *kPointSetup = R"HIP(#pragma unroll
    for (int i = 0; i < EPL; ++i) {
        const double e = ev[i];
        xx[i] = e > 1.0 ? 1.0 : e;
        yy[i] = 1.0 - xx[i];
    }
    const bool tf = xx[0] >= yy[0];
    const double *Qp = Qh + (tf ? FC * LDQ : 0);
#pragma unroll
    for (int i = 0; i < EPL; ++i) {
        const double num = tf ? yy[i] : xx[i], den = tf ? xx[i] : yy[i];
        zz[i] = num / den;
        bb[i] = den;
        const double g = tf ? 1.0 : zz[i];
        bp[i][0] = 1.0;
        gp[i][0] = 1.0;
#pragma unroll
        for (int r = 1; r <= DP; ++r) bp[i][r] = bp[i][r - 1] * den;
#pragma unroll
        for (int r = 1; r <= DG; ++r) gp[i][r] = gp[i][r - 1] * g;
)HIP";

// The fused prologue: the k_qrows phases for one c value per column
// (spom_engine.hip k_qrows) -- Z per hidden-state row, Pc per item, Q per
// entry -- all in LDS.  The column tables (host-built, 1 KiB-padded:
// var-column S, items, CSR, then zs as [k/2][row][k%2]) are copied to LDS
// through registers, all in flight, one barrier.
//
// c goes ahead of the points (the Z and item phases want it first); its value
// is selected after the front (kFusedTables), so that the scalar loads of c
// and of the late arguments wait once, together.
const char *kFusedColumns = R"HIP(    double cc[FC];
#pragma unroll
    for (int f = 0; f < FC; ++f) cc[f] = cvals[ic0 + f < nc ? ic0 + f : 0u];
)HIP";
// Pl: a column's items, then its zero slot (the flat Q sums' padding).  Rql:
// the reversed-copy slots, staged with the tables (REVQ is a global load,
// issued where used: after the Pc barrier).
const char *kFusedTables = R"HIP(#pragma unroll
    for (int f = 0; f < FC; ++f) cc[f] = ic0 + f < nc ? cc[f] : 0.0;
    __shared__ double Zl[FC * NJ];
#define PLS (NITEMS + 1)
    __shared__ double Pl[FC * PLS];
    const uint2 *Itl = (const uint2 *)(ct + OFF_IT);
    const u32 *Qsl = (const u32 *)(ct + OFF_QS);
    const u32 *Qil = (const u32 *)(ct + OFF_QI);
    const u32 *Rql = (const u32 *)(ct + OFF_RQ);
    const double *zcl = ct + OFF_ZC;
    const double *Svl = ct;
    const double *zl = ct + OFF_ZS;
)HIP";
// Operands of the Pc and Q phases that do not depend on Z, read and combined
// before the Z phase.  This pass: per item its Z slot and the product F of
// its var-column factors (a fixed pairwise tree).
// Item w of pass k (ITEM_W): even passes run from the last thread down, so a
// single pass (config 2: 588 items on 1 024 threads) lands on the waves
// without Z rows, which then run beside them (round 6: kernel 8.27 -> 8.16 us
// in the A/B, profiles/r06/cfg2); a wave with no item in a pass skips it
// (exec-empty branch).
// The factors: f_b = j_b ? 1 : B_b ? p_b : 1 - p_b with p_b = min(1, c S): one
// v_min_f64 for the clamp and j (round 6: the image marks j's columns +inf,
// so c S is +inf -- or NaN at c = 0, which minNum drops -- and p_b = 1.0;
// j <= B, so B_b is set there; the compare-and-select form cost 4 more
// instructions a factor, config 2 8.49 -> 8.32 us, profiles/r06/cfg2), then
// |n_b - p_b| with n_b = 1.0 where B_b is clear -- the same bits as
// fma(s, p, n), (s, n) = (1, 0) or (-1, 1) (1 - p rounded once, |0 - p| = p),
// with the abs moved to the product (k_qrows uses the same fold).
const char *kFusedItemPass = R"HIP(    constexpr int KPC = (FC * NITEMS + NT - 1) / NT;
    constexpr int KQ = (FC * LDQ + NT - 1) / NT;
    double Fp[KPC];
    u32 zi[KPC];
#define ITEM_W(k) ((k) * NT + (((k) & 1) ? threadIdx.x : NT - 1 - threadIdx.x))
#define ZW(k) ((k) * NT + threadIdx.x)
#define QW(k) ((k) * NT + threadIdx.x)
#pragma unroll
    for (int k = 0; k < KPC; ++k) {
        const u32 w = ITEM_W(k);
        Fp[k] = 0.0;
        zi[k] = 0u;
        if (w >= FC * NITEMS) continue;
        const u32 col = w % FC, it = w / FC;
        const double c = cc[col];
        const uint2 t = Itl[it];
        const u32 r = (t.x >> 24) | ((t.y >> 24) << 8), B = t.x & 0xffffffu, j = t.y & 0xffffffu;
        double f[NVAR];
        const u32 nB = ~B;
        (void)j;
#pragma unroll
        for (int b = 0; b < NVAR; ++b) {
            const u32 bit = NVAR - 1 - b;
            const double p = fmin(c * Svl[r * NVAR + b], 1.0);
            f[b] = (double)((nB >> bit) & 1u) - p;
        }
#pragma unroll
        for (int b = 0; b < NVAR; b += 2) f[b] = b + 1 < NVAR ? fabs(f[b]) * fabs(f[b + 1]) : fabs(f[b]);
#pragma unroll
        for (int s = 2; s < NVAR; s *= 2)
#pragma unroll
            for (int b = 0; b + s < NVAR; b += 2 * s) f[b] *= f[b + s];
        Fp[k] = f[0];
        zi[k] = col * NJ + r;
    }
)HIP";
// ... and per Q entry its item count and first QUN item indices: every index
// load in flight, reading past the entry within the image; slots past the
// count name the zero slot.
const char *kFusedQIndexPass = R"HIP(    u32 qb[KQ], qn[KQ], qx[KQ][QUN];
#pragma unroll
    for (int k = 0; k < KQ; ++k) {
        const u32 w = QW(k), q = w % LDQ;
        const bool live = w < FC * LDQ && q < NCOEF;
        const u32 q0 = live ? Qsl[q] : 0u, q1 = live ? Qsl[q + 1] : 0u;
        qb[k] = q0;
        qn[k] = q1 - q0;
#pragma unroll
        for (int u = 0; u < QUN; ++u) { const u32 t_ = Qil[q0 + u]; qx[k][u] = (u32)u < qn[k] ? t_ : (u32)NITEMS; }
    }
)HIP";
// Z per (column, row): the row's KZ (compile-time bound) values all in
// flight; rows past kmax contribute fma(-c, 0, 1) = 1 (with ZPAD the image
// holds those zero rows, so no per-value select).  Then the row's small
// columns: exp(-c (P1 + c (P2/2 + ...))), the expression k_zrows evaluates
// (spom_engine.hip zseries).
const char *kFusedZRows = R"HIP(#pragma unroll
    for (int k = 0; k < (FC * NJ + NT - 1) / NT; ++k) {
        const u32 w = ZW(k);
        if (w < FC * NJ) {
            const u32 col = w % FC, r = w / FC;
            const double c = cc[col];
            double sk[KZ];
#pragma unroll
            for (u32 kk = 0; kk < KZ; kk += 2) {
                const double2 t2 = ((const double2 *)zl)[(ZPAD || kk < kmax ? kk : kk % 8u) / 2 * NJ + r];
                sk[kk] = t2.x;
                sk[kk + 1] = t2.y;
            }
            double za = 1.0, zb = 1.0, zc = 1.0, zd = 1.0;
#pragma unroll
            for (u32 kk = 0; kk < KZ; kk += 8) {
                const bool in = ZPAD || kk < kmax;
#pragma unroll
                for (int u = 0; u < 8; ++u) sk[kk + u] = in ? sk[kk + u] : 0.0;
                za *= fma(-c, sk[kk + 0], 1.0) * fma(-c, sk[kk + 4], 1.0);
                zb *= fma(-c, sk[kk + 1], 1.0) * fma(-c, sk[kk + 5], 1.0);
                zc *= fma(-c, sk[kk + 2], 1.0) * fma(-c, sk[kk + 6], 1.0);
                zd *= fma(-c, sk[kk + 3], 1.0) * fma(-c, sk[kk + 7], 1.0);
            }
            double z = (za * zb) * (zc * zd);
            if (kmax && !(fma(-c, sk[0], 1.0) > 0.0)) z = 0.0;
            {
                const double2 *zq = (const double2 *)(zcl + r * 8);
                const double2 p01 = zq[0], p23 = zq[1], p45 = zq[2], p67 = zq[3];
                double q = p67.y;
                q = fma(q, c, p67.x);
                q = fma(q, c, p45.y);
                q = fma(q, c, p45.x);
                q = fma(q, c, p23.y);
                q = fma(q, c, p23.x);
                q = fma(q, c, p01.y);
                q = fma(q, c, p01.x);
                z *= exp(-(q * c));
            }
            Zl[col * NJ + r] = z;
        }
    }
    __syncthreads();
)HIP";
// Pc per item: its row's Z times the factors' product; then each column's
// zero slot.
const char *kFusedPcPass = R"HIP(#pragma unroll
    for (int k = 0; k < KPC; ++k) {
        const u32 w = ITEM_W(k);
        if (w < FC * NITEMS) Pl[(w % FC) * PLS + w / FC] = Zl[zi[k]] * Fp[k];
    }
    if (threadIdx.x < FC) Pl[threadIdx.x * PLS + NITEMS] = 0.0;
    __syncthreads();
)HIP";
// Q entries: the items in CSR (ascending j) order, summed by qsum_flat_code
// between these two, stored in both copies of the row.
const char *kFusedQSumsOpen = R"HIP(#pragma unroll
    for (int k = 0; k < KQ; ++k) {
        const u32 w = QW(k);
        if (w < FC * LDQ) {
            const double *pl = Pl + (w / LDQ) * PLS;
)HIP";
const char *kFusedQSumsClose = R"HIP(            Ql[w] = a;
            Ql[FC * LDQ + (w / LDQ) * LDQ + Rql[w % LDQ]] = a;
        }
    }
)HIP";

// ---- the plan's shape ------------------------------------------------------

// Every size the text depends on, resolved once: the #defines print these and
// the C++ loops below count with them.
struct Shape {
    int EPL;          // grid points per lane
    int KB;           // threads per column (KBLOCK)
    // columns per workgroup (KBLOCK threads each; the fused variant).  Two
    // columns per reading workgroup (both Q rows staged, the pair's results
    // stored as one 16-byte store per row through LDS) was measured slower on
    // configs 2 and 3, so the reading variant takes one.
    int FC;
    // target split (vlds): SPL waves per 64 points, wave group `half`
    // accumulating the new states l with l % SPL == half
    int SPL;
    int PRO;          // fused: the prologue's threads over the forward's
    uint32_t NT;      // threads of the workgroup: KB * FC * SPL * PRO
    uint32_t npmax;   // most states of a year
    bool gather;      // Ql gathered through plan.qidx
    size_t ldq;       // doubles of one staged Q row (LDQ)
    uint32_t qml = 1, qun = 1;  // fused: most items of a Q entry; of them index-preloaded
    // fused: 16-byte staging loads per thread of the table image, counted over
    // the KB * FC * PRO threads of a workgroup that is not split
    uint32_t nstg = 0;

    explicit Shape(const MdpJitPlan &pl)
        : EPL(pl.vlds ? (pl.epl == 2 ? 2 : 1) : pl.epl > 0 ? pl.epl : 2),
          KB(pl.kblock > 0 ? pl.kblock : 256),
          FC(pl.fused ? (pl.fused_cols > 0 ? pl.fused_cols : 1) : 1),
          SPL(pl.vlds && (pl.vsplit == 2 || pl.vsplit == 4) ? pl.vsplit : 1),
          PRO(pl.fused && pl.pro > 1 ? pl.pro : 1),
          NT((uint32_t)(KB * FC * SPL * PRO)),
          npmax(std::max<uint32_t>(1u, *std::max_element(pl.np.begin(), pl.np.end()))),
          gather(!pl.qidx.empty()),
          ldq(gather ? ((pl.qidx.size() + 1) & ~(size_t)1) : pl.ldQ)
    {
        if (!pl.fused) return;
        qml = std::max<uint32_t>(1u, pl.qmaxlen);
        qun = std::min<uint32_t>(qml, 16u);
        const uint32_t nt = (uint32_t)(KB * FC * PRO);
        nstg = std::max<uint32_t>(1u, (pl.ct_max / 2 + nt - 1) / nt);
    }
};

// ---- the transition cache --------------------------------------------------

// A use whose Q group (same offset = same H) recurs within kHorizon of its
// wave group's uses keeps its H in one of `nslot` registers; later uses read
// it.  Slots are evicted farthest-next-use first.  H is computed exactly as
// inline, so results do not change.  Positions count within the use's wave
// group, in the order that group emits its uses: the register kernel in use
// order (per new state l, ascending k); with the states in LDS, per year
// source-major (for k: for the group's l), so a region reads each state once
// and its accumulations are independent chains.  Each n[l] still sums
// ascending k, so the order changes no bits.
class TransitionCache {
public:
    TransitionCache(const MdpJitPlan &pl, int spl, int nslot)
        : nslot_(nslot), key_(pl.udesc.size()), grp_(pl.udesc.size(), 0), pos_(pl.udesc.size(), 0),
          next_(pl.udesc.size(), SIZE_MAX), slot_key_(spl), slot_next_(spl)
    {
        std::vector<std::vector<size_t>> seq(spl);
        size_t ub = 0;
        for (size_t t = 1; t < pl.np.size(); ++t) {
            const uint32_t npp = pl.np[t - 1], npc = pl.np[t];
            if (!pl.vlds)
                for (size_t j = 0; j < (size_t)npp * npc; ++j) seq[0].push_back(ub + j);
            else
                for (int h = 0; h < spl; ++h)
                    for (uint32_t k = 0; k < npp; ++k)
                        for (uint32_t l = h; l < npc; l += spl) seq[h].push_back(ub + (size_t)l * npp + k);
            ub += (size_t)npp * npc;
        }
        for (int h = 0; h < spl; ++h) {
            std::map<uint32_t, size_t> last;
            for (size_t p = seq[h].size(); p-- > 0;) {
                const size_t u = seq[h][p];
                key_[u] = use_off(pl.udesc[u]);
                grp_[u] = h;
                pos_[u] = p;
                auto it = last.find(key_[u]);
                if (it != last.end()) next_[u] = it->second;
                last[key_[u]] = p;
            }
        }
        reset();
    }

    // every slot free: the start of a copy of the forward
    void reset()
    {
        for (auto &k : slot_key_) k.assign(nslot_, 0u);
        for (auto &n : slot_next_) n.assign(nslot_, SIZE_MAX);  // SIZE_MAX: free / dead
    }

    // What use u does: read its H from `slot` (hit), compute H into `slot`
    // for later uses, or (slot < 0) compute it in place.
    struct Ref {
        int slot;
        bool hit;
    };
    Ref use(size_t u)
    {
        const size_t p = pos_[u], np = next_[u];
        std::vector<uint32_t> &skey = slot_key_[grp_[u]];
        std::vector<size_t> &snext = slot_next_[grp_[u]];
        for (int sl = 0; sl < nslot_; ++sl)
            if (snext[sl] == p && skey[sl] == key_[u]) {
                snext[sl] = np;
                return {sl, true};
            }
        if (nslot_ == 0 || np == SIZE_MAX || np - p > kHorizon) return {-1, false};
        int best = 0;
        for (int sl = 1; sl < nslot_; ++sl)
            if (snext[sl] > snext[best]) best = sl;
        if (snext[best] != SIZE_MAX && snext[best] <= np) return {-1, false};
        skey[best] = key_[u];
        snext[best] = np;
        return {best, false};
    }

private:
    static constexpr size_t kHorizon = 64;
    const int nslot_;
    std::vector<uint32_t> key_;       // per use: its Q group
    std::vector<int> grp_;            // per use: its wave group
    std::vector<size_t> pos_, next_;  // per use: its position, and that of the group's next use (SIZE_MAX: none)
    std::vector<std::vector<uint32_t>> slot_key_;  // per wave group and slot
    std::vector<std::vector<size_t>> slot_next_;   // ... the position of the held H's next use
};

// ---- the emitter -----------------------------------------------------------

class Emitter {
public:
    explicit Emitter(const MdpJitPlan &plan)
        : pl(plan), sch(schedule(plan)), sh(plan), window(plan.window > 0 ? plan.window : 8),
          nslot(plan.slots > 0 ? plan.slots : 0), cache(plan, sh.SPL, nslot)
    {
    }

    std::string source();

    const MdpJitPlan &pl;
    const Schedule sch;
    const Shape sh;
    double flops = 0.0;  // FP64 flops per grid point of the emitted code (the s-form copy's, an upper bound)

private:
    void defines();
    void revq();
    void signature();
    void shared_front();
    std::string points_front() const;
    std::string point_setup() const;
    void stage_qrow(const std::string &front, const std::string &early_setup);
    void stage_gather(const std::string &front, const std::string &early_setup);
    void fused_prologue(const std::string &front);
    void forward();
    void body(const char *coefs, bool with_g);
    void year_chain(size_t t, size_t &u);
    void year_lds(size_t t, size_t &u);
    void year_general(size_t t, size_t &u);
    void kernel_end();

    std::string stamp(int slot) const;
    std::string vref(uint32_t k) const;
    std::string src(size_t t, uint32_t k) const;
    std::string hexpr(uint32_t d) const;
    std::string gfac(uint32_t d) const;
    std::string use_expr(size_t u, std::string &pre);
    std::string flush_factor(size_t t) const { return power_expr("bb[i]", sch.flush[t], "fl"); }
    const char *guard() const;
    void fence();

    std::ostringstream o;
    const int window;  // transitions per scheduling region
    const int nslot;   // transition-cache registers
    TransitionCache cache;
    // the copy of the forward being emitted
    const char *qbase = "Qp";  // its coefficients: "Qp", "Qs_" or "Qt_"
    bool gmul = true;          // it multiplies by g^d
    int since = 0;             // transitions since the last region boundary
};

// diagnostic phase stamps: s_memtime (slots 0-5) and s_memrealtime (6, 7)
std::string Emitter::stamp(int slot) const
{
    if (!pl.diag) return std::string();
    return std::string("    if (stamps && threadIdx.x == 0) stamps[(size_t)blockIdx.x * 8 + ") + std::to_string(slot) +
           "] = " + (slot >= 6 ? "__builtin_amdgcn_s_memrealtime();\n" : "__builtin_amdgcn_s_memtime();\n");
}

void Emitter::defines()
{
    o << "#define LOGF(x) " << (pl.fast_log ? "mdp_log(x)" : "log(x)") << "\n";
    o << "#define KBLOCK " << sh.KB << "\n";
    o << "#define EPL " << sh.EPL << "\n#define LDQ " << sh.ldq << "\n#define LDQG " << (sh.gather ? pl.ldq_row : pl.ldQ)
      << "\n#define NQG " << pl.qidx.size() << "\n#define NPMAX " << sh.npmax << "\n#define DP " << sch.dp
      << "\n#define DG " << sch.dg << "\n";
    if (pl.fused)
        o << "#define NJ " << pl.nj << "\n#define NVAR " << pl.nvar << "\n#define NITEMS " << pl.nitems
          << "\n#define NCOEF " << pl.ncoef << "\n#define NQI " << (pl.nqi ? pl.nqi : 1) << "\n#define OFF_IT "
          << pl.off_it << "\n#define OFF_QS " << pl.off_qs << "\n#define OFF_QI " << pl.off_qi << "\n#define OFF_RQ "
          << pl.off_rq << "\n#define OFF_ZC " << pl.off_zc << "\n#define OFF_ZS " << pl.off_zs << "\n#define KZ "
          << std::max<uint32_t>(8u, pl.kzmax) << "\n#define ZPAD " << (pl.zpad ? 1 : 0) << "\n#define QML " << sh.qml
          << "\n#define QUN " << sh.qun << "\n#define NSTG " << sh.nstg << "\n";
    o << "#define FC " << sh.FC << "\n#define SPL " << sh.SPL << "\n#define NTF (KBLOCK * FC * SPL)\n#define NT (NTF * "
      << sh.PRO << ")\n";
}

// slot of each coefficient in the reversed copy (see the ratio forms), then
// the two scratch slots the staging stores past the row
void Emitter::revq()
{
    std::vector<uint32_t> all = mdp_jit_reversed_index(pl.udesc, sh.ldq);
    all.push_back((uint32_t)sh.ldq);
    all.push_back((uint32_t)sh.ldq + 1);
    o << "__constant__ const " << (sh.ldq <= 65536 ? "unsigned short" : "unsigned int") << " REVQ[" << sh.ldq + 2
      << "] = {";
    for (size_t q = 0; q < all.size(); ++q) o << (q ? (q % 32 ? "," : ",\n") : "") << all[q];
    o << "};\n";
}

// The parameter list of spom_jit.h.  Every pointer the kernel only reads stays
// const __restrict__: the code object then marks the argument read-only, and
// the runtime launches a kernel with a writable table argument measurably
// slower (config 2: 8.4 -> 11.0 us a step, the first phase 2 250 -> 6 130
// cycles with the same instructions; profiles/r07).  The workgroup count is an
// argument because the hidden gridDim.x is one more scalar round trip.
void Emitter::signature()
{
    o << "extern \"C\" __global__ __launch_bounds__(NT) "
      << (pl.wpe > 0 ? "__attribute__((amdgpu_waves_per_eu(" + std::to_string(pl.wpe) + "))) " : std::string())
      << "void mdp_fwd_jit(\n";
    const char *sep = "    ";
    const std::string tab = pl.fused ? "coltab" : "Qrow";
    auto name = [&](const char *n) { return std::string(n) == "tab" ? tab : std::string(n); };
#define MDP_JIT_IN_(t, n) o << sep << "const " #t " *__restrict__ " << name(#n), sep = ", ";
#define MDP_JIT_VAL_(t, n) o << sep << #t " " << name(#n), sep = ", ";
#define MDP_JIT_OUT_(t, n) o << sep << #t " *__restrict__ " << name(#n), sep = ", ";
#define MDP_JIT_NL_ sep = ",\n    ";
    MDP_FWD_JIT_PARAMS(MDP_JIT_IN_, MDP_JIT_VAL_, MDP_JIT_OUT_, MDP_JIT_NL_)
#undef MDP_JIT_IN_
#undef MDP_JIT_VAL_
#undef MDP_JIT_OUT_
#undef MDP_JIT_NL_
    o << ")\n{\n";
}

// What every variant starts with: the Q rows' LDS (stored order, then the
// same rows with every group reversed, read by t-form lanes), the fused
// kernel's table-image loads, the block's place in the grid and the lane's in
// its block.
void Emitter::shared_front()
{
    o << "    __shared__ __attribute__((aligned(16))) double Ql[2 * FC * LDQ + 2];\n" << stamp(6) << stamp(0);
    // The fused kernel's table image: the kernel's first loads, all in flight,
    // ahead even of the block's place in the grid.
    if (pl.fused) {
        o << "    extern __shared__ __attribute__((aligned(16))) double ct[];\n"
             "    const u32 n2 = ct_len / 2;\n";
        for (uint32_t k = 0; k < sh.nstg; ++k)
            o << "    const u32 si" << k << "_ = threadIdx.x + " << k << " * NT;\n"
              << "    const double2 stg" << k << "_ = ((const double2 *)coltab)[si" << k << "_ < n2 ? si" << k << "_ : 0];\n";
    }
    // XCD-aware order: the dispatcher deals blocks round-robin over the 8
    // XCDs, so consecutive logical blocks (adjacent c columns of the output
    // rows) are given to one XCD and its L2 assembles whole lines
    o << "    const u32 nb = nblk, full = nb & ~7u;\n"
      << (pl.xcd ? "    const u32 lb = blockIdx.x < full ? (blockIdx.x & 7u) * (full >> 3) + (blockIdx.x >> 3) : blockIdx.x;\n"
                 : "    const u32 lb = blockIdx.x + 0 * full;\n")
      // FC columns per workgroup (fused variant): KBLOCK threads each
      << "    const u32 half = threadIdx.x / KBLOCK, tid = threadIdx.x % KBLOCK;\n"
      // the lane's place in its column's e block: with several columns per
      // workgroup each column's lanes are rotated by half a block, so the
      // waves a SIMD holds (wave w on SIMD w mod 4) take e rows from both
      // halves -- on a grid with ratio forms split at the block's middle
      // every SIMD then runs one s-form and one t-form wave, not two of one
      << (sh.FC > 1 && sh.SPL == 1 && pl.rot ? "    const u32 tip = (tid + half * (KBLOCK / 2)) % KBLOCK;\n"
                                             : "    const u32 tip = tid;\n")
      // (column group, e block): FC columns x KBLOCK*EPL e values per workgroup
      << (pl.efast ? "    const u32 gy = (nlist + KBLOCK * EPL - 1) / (KBLOCK * EPL), ic0 = lb / gy * FC, by = lb % gy;\n"
                   : "    const u32 ncb = (nc + FC - 1) / FC, ic0 = lb % ncb * FC, by = lb / ncb;\n")
      << (sh.SPL > 1 || sh.FC == 1 ? "    const u32 ic = ic0;\n" : "    const u32 ic = ic0 + half;\n")
      << (sh.SPL > 1 ? "    const double *Qh = Ql;\n" : "    const double *Qh = Ql + half * LDQ;\n");
}

std::string Emitter::points_front() const
{
    return std::string(kFrontDecl) + (sh.EPL == 1 ? kFrontPoint : kFrontList) + kFrontLate;
}

// kPointSetup, then the state vector's first values: 1 for the first year's
// states (the prior is applied at the end), or the previous chunk's end vector
// (ldv covers every lane's list position)
std::string Emitter::point_setup() const
{
    std::ostringstream w;
    w << kPointSetup;
    const char *vdst = pl.vlds ? "Vl[(k * EPL + i) * KBLOCK + tid]" : "v[i][k]";
    // (split: the state k set by wave group k % SPL)
    w << (sh.SPL > 1 ? "#pragma unroll\n        for (int k = half; k < NPMAX; k += SPL) "
                     : "#pragma unroll\n        for (int k = 0; k < NPMAX; ++k) ")
      << vdst << " = k < " << pl.np[0]
      << (pl.first ? " ? 1.0 : 0.0;\n" : " ? vscr[((size_t)k * nc + ic) * ldv + pp[i]] : 0.0;\n") << "    }\n";
    return w.str();
}

// This column's Q row (k_qrows), in stored order and, through REVQ, with every
// group reversed: every load in flight before the (unconditional, past the
// end into a scratch slot) stores, one named register per staging load,
// emitted unrolled, as the fused kernel's.
void Emitter::stage_qrow(const std::string &front, const std::string &early_setup)
{
    const uint32_t nk = (uint32_t)((sh.ldq / 2 + sh.NT - 1) / sh.NT);
    o << "    const double2 *src_ = (const double2 *)(Qrow + (size_t)ic * LDQ);\n"
         "    constexpr u32 N2 = LDQ / 2;\n";
    for (uint32_t k = 0; k < nk; ++k) {
        const std::string K = std::to_string(k);
        o << "    const u32 qi" << K << "_ = threadIdx.x + " << K << " * NT;\n"
          << "    const double2 qt" << K << "_ = src_[qi" << K << "_ < N2 ? qi" << K << "_ : 0];\n"
          << "    const u32 ra" << K << "_ = REVQ[qi" << K << "_ < N2 ? 2 * qi" << K << "_ : 0], rb" << K
          << "_ = REVQ[qi" << K << "_ < N2 ? 2 * qi" << K << "_ + 1 : 0];\n";
    }
    o << front << early_setup << "    {\n        double2 *dst_ = (double2 *)Ql;\n";
    for (uint32_t k = 0; k < nk; ++k) {
        const std::string K = std::to_string(k);
        o << "        dst_[qi" << K << "_ < N2 ? qi" << K << "_ : LDQ] = qt" << K << "_;\n"
          << "        Ql[qi" << K << "_ < N2 ? LDQ + ra" << K << "_ : 2 * LDQ] = qt" << K << "_.x;\n"
          << "        Ql[qi" << K << "_ < N2 ? LDQ + rb" << K << "_ : 2 * LDQ] = qt" << K << "_.y;\n";
    }
    o << "    }\n" << stamp(1);
}

// This chunk's coefficients gathered from the column's Q row: every load in
// flight before the (unconditional) stores (the list's loads first; the
// coefficient loads depend on them).
void Emitter::stage_gather(const std::string &front, const std::string &early_setup)
{
    const uint32_t nk = (uint32_t)((pl.qidx.size() + sh.NT - 1) / sh.NT);
    o << "    const double *src_ = Qrow + (size_t)ic * LDQG;\n";
    for (uint32_t k = 0; k < nk; ++k) {
        const std::string K = std::to_string(k);
        o << "    const u32 qi" << K << "_ = threadIdx.x + " << K << " * NT;\n"
          << "    const u32 qx" << K << "_ = qidx[qi" << K << "_ < NQG ? qi" << K << "_ : 0];\n"
          << "    const u32 qr" << K << "_ = REVQ[qi" << K << "_ < NQG ? qi" << K << "_ : 0];\n";
    }
    o << front;
    for (uint32_t k = 0; k < nk; ++k) o << "    const double qt" << k << "_ = src_[qx" << k << "_];\n";
    o << early_setup;
    for (uint32_t k = 0; k < nk; ++k) {
        const std::string K = std::to_string(k);
        o << "    Ql[qi" << K << "_ < NQG ? qi" << K << "_ : 2 * LDQ] = qt" << K << "_;\n"
          << "    Ql[qi" << K << "_ < NQG ? LDQ + qr" << K << "_ : 2 * LDQ] = qt" << K << "_;\n";
    }
    o << stamp(1);
}

// The fused variant computes its columns' Q rows itself (the raw literals
// above, in order).  The image's stores are unconditional: lanes past the
// image write a scratch slot, so the loads are not sunk into per-load
// branches (load, wait, store x NSTG).
void Emitter::fused_prologue(const std::string &front)
{
    o << kFusedColumns << front << kFusedTables;
    for (uint32_t k = 0; k < sh.nstg; ++k)
        o << "    ((double2 *)ct)[si" << k << "_ < n2 ? si" << k << "_ : n2] = stg" << k << "_;\n";
    o << "    __syncthreads();\n"
      << stamp(4) << kFusedItemPass << kFusedQIndexPass << kFusedZRows << stamp(5) << kFusedPcPass << stamp(1)
      << kFusedQSumsOpen << qsum_flat_code(sh.qml, sh.qun) << kFusedQSumsClose;
}

// the state k of point i, as an expression
std::string Emitter::vref(uint32_t k) const
{
    return pl.vlds ? "Vl[(" + std::to_string(k) + " * EPL + i) * KBLOCK + tid]" : "v[i][" + std::to_string(k) + "]";
}

// source k of year t, scaled by B^(|A_k| - the year's minimum) where that is
// not 0 (the register kernel scales in place before the year instead)
std::string Emitter::src(size_t t, uint32_t k) const
{
    const uint32_t df = sch.diff[t][k];
    return pl.vlds && df ? "(" + vref(k) + " * bp[i][" + std::to_string(df) + "])" : vref(k);
}

// H for point i: the Horner chain of a Q group (offset, nX) over the lane's
// copy of the coefficients (stored order for s-form lanes, reversed for
// t-form ones).  Transitions of one group (same A & B and B) from sources of
// different |A| share H and differ only in g^d.
std::string Emitter::hexpr(uint32_t d) const
{
    const uint32_t off = use_off(d), nX = use_nx(d);
    std::string e = std::string(qbase) + "[" + std::to_string(off) + "]";
    for (uint32_t m = 1; m <= nX; ++m) e = "fma(" + e + ", zz[i], " + qbase + "[" + std::to_string(off + m) + "])";
    return e;
}

std::string Emitter::gfac(uint32_t d) const
{
    const uint32_t nX = use_nx(d), nA = use_na(d);
    return gmul && nA > nX ? " * gp[i][" + std::to_string(nA - nX) + "]" : std::string();
}

// The expression for use u (H times its g^d); `pre` gets "pc[i][s] = H; "
// when the use fills a cache slot (inside the caller's per-point loop).
std::string Emitter::use_expr(size_t u, std::string &pre)
{
    const uint32_t d = pl.udesc[u];
    const std::string g = gfac(d);
    if (!g.empty()) flops += 1.0;
    const TransitionCache::Ref r = cache.use(u);
    const std::string held = r.slot < 0 ? std::string() : "pc[i][" + std::to_string(r.slot) + "]";
    if (r.hit) return "(" + held + g + ")";
    flops += 2.0 * use_nx(d);  // nX FMAs
    const std::string e = hexpr(d);
    if (held.empty()) return "((" + e + ")" + g + ")";
    pre = held + " = " + e + "; ";
    return "(" + held + g + ")";
}

// Regions are separate basic blocks: each guard value passes through an
// opaque scalar move, so instruction selection can neither merge regions nor
// hoist every transition's reads to the top (which spills).  (With the states
// in LDS the guard also clobbers memory, so a state loaded in one region is
// reloaded in the next rather than held in a register across the year.)
const char *Emitter::guard() const
{
    return pl.vlds ? "    { u32 g_; asm volatile(\"s_mov_b32 %0, %1\" : \"=s\"(g_) : \"s\"(one) : \"memory\"); if (g_) {\n"
                   : "    { u32 g_; asm volatile(\"s_mov_b32 %0, %1\" : \"=s\"(g_) : \"s\"(one)); if (g_) {\n";
}

void Emitter::fence()
{
    if (++since >= window) {
        o << "    }}\n" << guard();
        since = 0;
    }
}

// a 1 x 1 year of the register kernel: the state times the transition
void Emitter::year_chain(size_t t, size_t &u)
{
    std::string pre;
    const std::string e = use_expr(u++, pre);
    o << "    for (int i = 0; i < EPL; ++i) { " << pre << "v[i][0] = v[i][0] * " << e << "; }\n";
    flops += 1.0;
    if (sch.flush[t]) {
        o << "    for (int i = 0; i < EPL; ++i) v[i][0] *= " << flush_factor(t) << ";\n";
        flops += 1.0;
    }
    fence();
}

// A year with the states in LDS: wave group h accumulates the new states
// l = h, h + SPL, ... (a wave-uniform branch when split), source-major; with
// the split a barrier either side of the write-back (each lane otherwise
// touches only its own column of Vl).
void Emitter::year_lds(size_t t, size_t &u)
{
    const uint32_t npp = pl.np[t - 1], npc = pl.np[t];
    const int SPL = sh.SPL;
    const bool split = SPL > 1;
    auto branch = [&](int h, const char *ind) {
        return h == 0      ? std::string(ind) + "if (half == 0) {\n"
             : h + 1 < SPL ? std::string(ind) + "} else if (half == " + std::to_string(h) + ") {\n"
                           : std::string(ind) + "} else {\n";
    };
    if (split) o << "    }}\n";
    for (int h = 0; h < SPL; ++h) {
        if (split) {
            o << branch(h, "    ") << guard();
            since = 0;
        }
        for (uint32_t k = 0; k < npp; ++k)
            for (uint32_t l = h; l < npc; l += SPL) {
                std::string pre;
                const std::string e = use_expr(u + (size_t)l * npp + k, pre);
                const std::string acc = "n[i][" + std::to_string(l / SPL) + "]";
                o << "    for (int i = 0; i < EPL; ++i) { " << pre << acc << " = fma(" << src(t, k) << ", " << e << ", "
                  << (k ? acc : std::string("0.0")) << "); }\n";
                flops += sch.diff[t][k] ? 1.0 : 0.0;
                flops += k ? 2.0 : 1.0;
                fence();
            }
        if (split) o << "    }}\n";
    }
    if (split) o << "    }\n    __syncthreads();\n";
    o << "    for (int i = 0; i < EPL; ++i) {\n";
    if (sch.flush[t]) {
        o << "        const double fl_ = " << flush_factor(t) << ";\n";
        flops += 1.0 + npc;
    }
    for (int h = 0; h < SPL; ++h) {
        if (split) o << branch(h, "        ");
        for (uint32_t l = h; l < npc; l += SPL)
            o << "            " << vref(l) << " = n[i][" << l / SPL << "]" << (sch.flush[t] ? " * fl_" : "") << ";\n";
    }
    o << (split ? "        }\n    }\n    __syncthreads();\n" : "    }\n");
    if (split) {
        o << guard();
        since = 0;
    }
    u += (size_t)npp * npc;
}

// A general year of the register kernel: the sources above the year's
// minimum |A| scaled in place, then n[.][l] = sum_k v[.][k] P[k][l] in
// ascending k.  States past npc are never read again (a year reads k < npp,
// and the final sum runs over the last year's states), so they are not
// zeroed: that was ~5 % of the forward's VALU issue on config 3.
void Emitter::year_general(size_t t, size_t &u)
{
    const uint32_t npp = pl.np[t - 1], npc = pl.np[t];
    for (uint32_t k = 0; k < npp; ++k)
        if (sch.diff[t][k]) {
            o << "    for (int i = 0; i < EPL; ++i) v[i][" << k << "] *= bp[i][" << sch.diff[t][k] << "];\n";
            flops += 1.0;
        }
    for (uint32_t l = 0; l < npc; ++l)
        for (uint32_t k = 0; k < npp; ++k) {
            std::string pre;
            const std::string e = use_expr(u++, pre);
            o << "    for (int i = 0; i < EPL; ++i) { " << pre << "n[i][" << l << "] = fma(" << vref(k) << ", " << e
              << ", " << (k ? "n[i][" + std::to_string(l) + "]" : std::string("0.0")) << "); }\n";
            flops += k ? 2.0 : 1.0;
            fence();
        }
    o << "    for (int i = 0; i < EPL; ++i) {\n";
    if (sch.flush[t]) {  // the pending exponent is applied: the new states times B^E (one factor per point)
        o << "        const double fl_ = " << flush_factor(t) << ";\n";
        flops += 1.0 + npc;
    }
    for (uint32_t l = 0; l < npc; ++l)
        o << "        " << vref(l) << " = n[i][" << l << "]" << (sch.flush[t] ? " * fl_" : "") << ";\n";
    o << "    }\n";
}

// one copy of the forward recursion, with its own transition-cache state
void Emitter::body(const char *coefs, bool with_g)
{
    qbase = coefs;
    gmul = with_g;
    cache.reset();
    since = 0;
    o << guard();
    size_t u = 0;
    for (size_t t = 1; t < pl.np.size(); ++t) {
        if (pl.vlds) year_lds(t, u);
        else if (pl.np[t - 1] == 1 && pl.np[t] == 1) year_chain(t, u);
        else year_general(t, u);
    }
    o << "    }}\n";
}

// Register kernels emit the forward twice (split_forms), once per ratio form
// behind a lane-uniform branch on tf: the t-form copy reads the reversed
// coefficients at a fixed base and drops every g^d factor (g = 1 there, so
// the products it leaves out are exact: the same bits), 55 % of config 2's
// uses; waves of one form run only their copy.  The LDS-state kernels keep
// one copy (their wave groups already branch per year).  The flop count is
// the first copy's: the s-form's, an upper bound.
void Emitter::forward()
{
    if (nslot > 0) o << "    double pc[EPL][" << nslot << "];\n";
    if (!pl.vlds && pl.split_forms) {
        // (s-form lanes: the stored coefficients; t-form: the reversed copy)
        o << "    if (!tf) {\n    const double *Qs_ = Qh;\n";
        body("Qs_", true);
        const double counted = flops;
        o << "    } else {\n    const double *Qt_ = Qh + FC * LDQ;\n";
        body("Qt_", false);
        flops = counted;
        o << "    }\n";
    } else {
        body("Qp", true);
    }
}

// The pending exponent at the end is applied to L (last chunk); a chunk that
// is not the last hands its states over unscaled (the next one starts from
// this exponent, plan.e0).  MDP_JIT_HACK (measurement only): the result is
// never stored.
void Emitter::kernel_end()
{
    const std::string fin = power_expr("bb[i]", sch.final_exp, "fe");
    if (sch.final_exp && pl.last) flops += 1.0;
    o << stamp(3) << "#define NPLAST " << pl.np.back() << "\n"
      << (pl.vlds ? "#define VREF(l) Vl[((l) * EPL + i) * KBLOCK + tid]\n" : "#define VREF(l) v[i][l]\n");
    if (pl.last && (pl.hack == 1 || pl.hack == 2))
        o << "#pragma unroll\n"
             "    for (int i = 0; i < EPL; ++i) {\n"
             "        double L = 0.0;\n"
             "#pragma unroll\n"
             "        for (int l = 0; l < NPLAST; ++l) L += VREF(l) * prior0;\n"
          << (pl.hack == 1 ? "        if (L == 1234.5678 && st[i] && ic < nc) out[(size_t)ie[i] * ld_out + (size_t)ic * out_cs] = log(L);\n"
                           : "        const double lg_ = LOGF(L * " + fin + ");\n"
                             "        if (lg_ == 1234.5678 && st[i] && ic < nc) out[(size_t)ie[i] * ld_out + (size_t)ic * out_cs] = lg_;\n")
          << "    }\n";
    else if (pl.last)
        o << "    if (SPL == 1 || half == 0) {\n"
             "#pragma unroll\n"
             "    for (int i = 0; i < EPL; ++i) {\n"
             "        double L = 0.0;\n"
             "#pragma unroll\n"
             "        for (int l = 0; l < NPLAST; ++l) L += VREF(l) * prior0;\n"
          << (sch.final_exp ? "        L *= " + fin + ";\n" : std::string()) <<
             "        if (st[i] && ic < nc) out[(size_t)ie[i] * ld_out + (size_t)ic * out_cs] = LOGF(L);\n"
             "    }\n"
             "    }\n";
    else  // hand the end vector to the next chunk
        o << "    if (ic < nc) {\n"
             "#pragma unroll\n"
             "        for (int i = 0; i < EPL; ++i) {\n"
             "#pragma unroll\n"
             "            for (int l = 0; l < NPLAST; ++l)\n"
             "                if (SPL == 1 || l % SPL == (int)half) vscr[((size_t)l * nc + ic) * ldv + pp[i]] = VREF(l);\n"
             "        }\n"
             "    }\n";
    o << stamp(7) << "}\n";
}

std::string Emitter::source()
{
    // flops per point: the ratio and its power tables, the transitions and
    // scalings (counted where they are emitted), the prior sum
    flops = 2.0 + (double)sch.dp + (double)sch.dg + (pl.last ? 2.0 * sh.npmax : 0.0);
    o << kPrelude;
    defines();
    revq();
    signature();
    shared_front();
    const std::string front = points_front(), setup = point_setup();
    // a later chunk's hand-over loads (vscr) go out ahead of the staging
    // stores, so they share the staging loads' round trip
    const bool early = !pl.fused && !pl.first;
    o << "    double xx[EPL], yy[EPL], zz[EPL], bb[EPL], bp[EPL][DP + 1], gp[EPL][DG + 1];\n"
         "    double v[EPL][NPMAX];\n    double n[EPL][(NPMAX + SPL - 1) / SPL];\n";
    if (pl.vlds)  // wide years: state k of point i of lane tid at Vl[k][i][tid]
        o << "    __shared__ double Vl[NPMAX * EPL * KBLOCK];\n";
    if (pl.fused) fused_prologue(front);
    else if (sh.gather) stage_gather(front, early ? setup : std::string());
    else stage_qrow(front, early ? setup : std::string());
    if (!early) o << setup;
    o << "    __syncthreads();\n"
      << stamp(2)
      // the prologue's extra threads (PRO > 1) are done: the forward runs on NTF
      << (sh.PRO > 1 ? "    if (threadIdx.x >= NTF) return;\n" : "");
    forward();
    kernel_end();
    o << "// EPL_CHOSEN " << sh.EPL << "\n";
    return o.str();
}

}  // namespace

std::string mdp_jit_forward_source(MdpJitPlan &plan)
{
    Emitter em(plan);
    plan.epl = em.sh.EPL;
    const std::string src = em.source();
    plan.flops_pt = em.flops;
    return src;
}

std::string mdp_jit_log_source()
{
    return std::string(kPrelude) +
           "extern \"C\" __global__ void mdp_log_apply(const double *__restrict__ x, double *__restrict__ y, "
           "unsigned long long n)\n{\n"
           "    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;\n"
           "    if (i < n) y[i] = mdp_log(x[i]);\n}\n";
}
