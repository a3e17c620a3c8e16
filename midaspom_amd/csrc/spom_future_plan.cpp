// midaspom_amd/csrc/spom_future_plan.cpp -- host planning of the future
// engine (spom_future_plan.h): option parsing, kernel selection, the
// cumulative posterior, the lane kernels' mask and table, the two-sided
// distance image, the lane-owned layout and its inverse.  Host only.
#include "spom_future_plan.h"

#include <cmath>
#include <string>

#include "spom_opts.h"

int fut_parse_opts(const char *s, FutWideMode *mode, uint32_t *sum_years)
{
    *mode = kFutWideOff;
    if (sum_years) *sum_years = 0;
    if (!s) return MDP_OK;
    return mdp_for_each_opt(s, [&](const std::string &k, const std::string &val, bool has) -> int {
        const std::string v = has ? val : std::string("1");
        if (k == "MDP_FUT_SUM_YEARS") {
            // 1 to 5 decimal digits, at most kFutSumMaxT
            uint32_t y = 0;
            bool ok = !v.empty() && v.size() <= 5;
            for (size_t i = 0; ok && i < v.size(); ++i) {
                ok = v[i] >= '0' && v[i] <= '9';
                y = y * 10 + (uint32_t)(v[i] - '0');
            }
            if (!ok || y > kFutSumMaxT)
                return mdp_set_error(MDP_EINVAL, "MDP_FUT_SUM_YEARS=%s (expected 0..%u)", v.c_str(), kFutSumMaxT);
            if (sum_years) *sum_years = y;
            return MDP_OK;
        }
        if (k != "MDP_FUT_WIDE") return mdp_set_error(MDP_EINVAL, "unknown future option '%s'", k.c_str());
        if (v == "0") *mode = kFutWideOff;
        else if (v == "auto") *mode = kFutWideAuto;
        else if (v == "1") *mode = kFutWideOn;
        else return mdp_set_error(MDP_EINVAL, "MDP_FUT_WIDE=%s (expected 0, auto or 1)", v.c_str());
        return MDP_OK;
    });
}

int fut_select_kernel(uint32_t n, FutWideMode mode, uint32_t *np)
{
    *np = 0;
    if (n > kFutWideMaxN)
        return mdp_set_error(MDP_EUNSUPPORTED, "%u patches: the future engine holds <= %u", n, kFutWideMaxN);
    if (mode == kFutWideOff || (mode == kFutWideAuto && n <= kFutLaneMaxN)) {
        if (n > kFutLaneMaxN)
            return mdp_set_error(MDP_EUNSUPPORTED, "%u patches: the future engine holds <= 64", n);
        return MDP_OK;
    }
    *np = n <= 128 ? 1 : n <= 256 ? 2 : n <= 512 ? 4 : 8;
    return MDP_OK;
}

int fut_lane_plan(const int32_t *last_row, uint32_t n, double m, double d, double KD, double KS, double dS,
                  FutLanePlan *plan)
{
    if (!last_row || !plan || n == 0 || n > kFutLaneMaxN)
        return mdp_set_error(MDP_EINVAL, "internal: lane plan of %u patches", n);
    FutLanePlan &p = *plan;
    p = FutLanePlan();
    p.n = n;
    p.nm = fut_lane_nm(n);
    // last survey row -> occupied bits and missing columns (:292-323)
    for (uint32_t j = 0; j < n; ++j) {
        if (last_row[j] == 1) p.occ0 |= 1ull << j;
        else if (last_row[j] == -1) p.miss.push_back(1ull << j);
        else if (last_row[j] != 0)
            return mdp_set_error(MDP_EINVAL, "survey value %d in column %u (expected -1, 0 or 1)", last_row[j], j);
    }
    if (p.miss.size() > kFutMaxMissing)
        return mdp_set_error(MDP_EUNSUPPORTED, "%zu missing patches (npstates = 2^%zu overflows int)", p.miss.size(),
                             p.miss.size());
    p.nmiss = (uint32_t)p.miss.size();
    // dispersal (:266-277), a = 1/m; M*K_D and the source term M[n][k]*K_S
    const double a = 1.0 / m;
    p.MK.assign((size_t)p.nm * p.nm, 0.0);
    p.src.assign(p.nm, 0.0);
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = i + 1; j < n; ++j) {
            const double v = exp(-a * (j - i) * d);
            p.MK[(size_t)i * p.nm + j] = v * KD;
            p.MK[(size_t)j * p.nm + i] = v * KD;
        }
    for (uint32_t j = 0; j < n; ++j) p.src[j] = exp(-a * (j + 1) * dS) * KS;
    return MDP_OK;
}

int fut_post_plan(const double *post, uint32_t necstep, FutPostPlan *plan)
{
    if (!plan || (necstep > 0 && !post)) return mdp_set_error(MDP_EINVAL, "null posterior");
    FutPostPlan &p = *plan;
    p = FutPostPlan();
    // the scan stops matching at the first NaN
    p.pcum.resize((size_t)necstep * necstep);
    double acc = 0;
    size_t lv = p.pcum.size();
    for (uint32_t ie = 0; ie < necstep; ++ie)
        for (uint32_t ic = 0; ic < necstep; ++ic) {
            double w = 1.0;
            if (ie == 0 || ie == necstep - 1) w *= 0.5;
            if (ic == 0 || ic == necstep - 1) w *= 0.5;
            acc += w * post[(size_t)ie * necstep + ic];
            const size_t i = (size_t)ie * necstep + ic;
            p.pcum[i] = acc;
            if (std::isnan(acc) && lv == p.pcum.size()) lv = i;
        }
    for (size_t i = 0; i < lv; ++i)
        if (p.pcum[i] < (i ? p.pcum[i - 1] : 0.0))
            return mdp_set_error(MDP_EUNSUPPORTED, "posterior with negative entries (cell %zu): the sampler "
                                 "needs a non-decreasing cumulative sum", i);
    if (lv > 0 && !(p.pcum[lv - 1] > 0)) lv = 0;  // no draw is ever below the mass: (0, 0) for all
    p.lvalid = (uint32_t)lv;
    p.pscale = (double)((int)(necstep - 1) * (int)(necstep - 1));
    return MDP_OK;
}

int fut_wide_plan(const int32_t *last_row, uint32_t n, uint32_t np, double m, double d, double KD, double KS,
                  double dS, FutWidePlan *plan)
{
    if (!last_row || !plan || n == 0 || np == 0 || n > 128 * np)
        return mdp_set_error(MDP_EINVAL, "internal: wide plan of %u patches with %u pairs per lane", n, np);
    FutWidePlan &p = *plan;
    p = FutWidePlan();
    p.n = n;
    p.np = np;
    p.occ0.assign(64, 0u);
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t pair = k >> 1, lane = pair & 63u, bit = 2 * (pair >> 6) + (k & 1u);
        if (last_row[k] == 1) p.occ0[lane] |= 1u << bit;
        else if (last_row[k] == -1) p.miss.push_back((lane << 8) | bit);
        else if (last_row[k] != 0)
            return mdp_set_error(MDP_EINVAL, "survey value %d in column %u (expected -1, 0 or 1)", last_row[k], k);
    }
    if (p.miss.size() > kFutMaxMissing)
        return mdp_set_error(MDP_EUNSUPPORTED, "%zu missing patches (npstates = 2^%zu overflows int)", p.miss.size(),
                             p.miss.size());
    p.nmiss = (uint32_t)p.miss.size();
    // dispersal (future.c:266-277), a = 1/m: the same expressions, so the
    // same bits, as the n x n table of the lane kernels
    const double a = 1.0 / m;
    p.len = (n + 128 * np + 1) & ~1u;
    std::vector<double> G((size_t)p.len + 1, 0.0);
    for (uint32_t dist = 1; dist < n; ++dist) {
        const double v = exp(-a * dist * d) * KD;
        G[n - 1 - dist] = v;
        G[n - 1 + dist] = v;
    }
    p.image.assign((size_t)2 * p.len, 0.0);
    for (uint32_t i = 0; i < p.len; ++i) {
        p.image[i] = G[i];
        p.image[(size_t)p.len + i] = G[i + 1];
    }
    p.src.assign((size_t)128 * np, 0.0);
    for (uint32_t j = 0; j < n; ++j) p.src[j] = exp(-a * (j + 1) * dS) * KS;
    return MDP_OK;
}

void fut_wide_unpack(const uint32_t *lanes, uint64_t nrep, uint32_t n, uint32_t np, uint64_t *words)
{
    const uint32_t W = (n + 63) / 64;
    (void)np;
    for (uint64_t r = 0; r < nrep; ++r) {
        uint64_t *w = words + r * W;
        for (uint32_t i = 0; i < W; ++i) w[i] = 0;
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t pair = k >> 1, lane = pair & 63u, bit = 2 * (pair >> 6) + (k & 1u);
            if ((lanes[r * 64 + lane] >> bit) & 1u) w[k >> 6] |= 1ull << (k & 63u);
        }
    }
}

int fut_sum_plan(uint32_t n, uint32_t np, uint32_t wlen, uint32_t tfut, uint32_t cap, FutSumPlan *plan)
{
    if (!plan || n == 0 || n > (np ? 128 * np : kFutLaneMaxN))
        return mdp_set_error(MDP_EINVAL, "internal: summary plan of %u patches with %u pairs per lane", n, np);
    if (tfut == 0 || tfut > kFutSumMaxT)
        return mdp_set_error(MDP_EUNSUPPORTED, "duration %u outside 1..%u years", tfut, kFutSumMaxT);
    if ((uint64_t)tfut * (2 * n + 1) > kFutSumMaxCells)
        return mdp_set_error(MDP_EUNSUPPORTED, "%u years x %u cells: the summary tables hold at most %llu cells", tfut,
                             2 * n + 1, (unsigned long long)kFutSumMaxCells);
    FutSumPlan &p = *plan;
    p = FutSumPlan();
    p.cells = np ? n + 1 + 128 * np : 2 * n + 1;
    p.years = kFutSumTableBytes / (4 * p.cells);  // >= 1: a year is at most 2049 cells
    if (p.years > tfut) p.years = tfut;
    if (cap && p.years > cap) p.years = cap;
    p.windows = (tfut + p.years - 1) / p.years;
    const uint32_t fixed = np ? 2 * wlen * (uint32_t)sizeof(double) : n <= 8 ? 16384u : 0u;
    p.lds = fixed + p.years * p.cells * 4;
    // waves per SIMD of k_future_wide_tab<1|2|4|8>: 7, 7, 5, 3; of k_future_tab<8|16|32|64>: 7, 3, 2, 1
    p.maxwg = np ? (np <= 2 ? 2048u : np == 4 ? 1280u : 768u) : n <= 8 ? 2048u : n <= 16 ? 1024u : 512u;
    p.reps = p.windows == 1 ? kFutSumOneWindowReps : np ? kFutSumWideReps : kFutSumLaneReps;
    return MDP_OK;
}
