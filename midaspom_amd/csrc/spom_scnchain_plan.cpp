// midaspom_amd/csrc/spom_scnchain_plan.cpp -- host planning of the
// count-class chain likelihoods (spom_scnchain_plan.h): option parsing, the
// refusals, the dispersal and source tables, the default target, the launches
// of a counting call and the host form of the chain evaluation.  Host only.
#include "spom_scnchain_plan.h"

#include <algorithm>
#include <cmath>
#include <string>

#include "spom_opts.h"
#include "spom_scn_row.h"

namespace {

// 1 to 19 decimal digits
bool chain_decimal(const std::string &v, uint64_t *out)
{
    if (v.empty() || v.size() > 19) return false;
    uint64_t x = 0;
    for (char ch : v) {
        if (ch < '0' || ch > '9') return false;
        x = x * 10 + (uint64_t)(ch - '0');
    }
    *out = x;
    return true;
}

// ne*nc (*nK*nd) with every partial product below 2^52 before it is compared
int chain_points(bool baseline, uint32_t ne, uint32_t nc, uint32_t nK, uint32_t nd, uint64_t *G)
{
    if (ne == 0 || nc == 0 || (!baseline && (nK == 0 || nd == 0))) return mdp_set_error(MDP_EINVAL, "empty grid axis");
    uint64_t g = (uint64_t)ne * nc;
    if (!baseline) {
        if (g <= kChainMaxPoints) g *= nK;
        if (g <= kChainMaxPoints) g *= nd;
    }
    if (g > kChainMaxPoints)
        return mdp_set_error(MDP_EUNSUPPORTED, "grid of more than %llu points", (unsigned long long)kChainMaxPoints);
    *G = g;
    return MDP_OK;
}

int chain_check_weights(const char *name, const double *w, uint32_t n)
{
    for (uint32_t k = 0; w && k <= n; ++k)
        if (!(w[k] >= 0) || !std::isfinite(w[k]))
            return mdp_set_error(MDP_EINVAL, "%s[%u] must be finite and >= 0", name, k);
    return MDP_OK;
}

}  // namespace

int chain_parse_opts(const char *s, ChainOpts *o)
{
    *o = ChainOpts();
    return mdp_for_each_opt(s, [&](const std::string &k, const std::string &v, bool) -> int {
        uint64_t x = 0;
        if (k == "MDP_CHAIN_NM") {
            if (!chain_decimal(v, &x) || (x != 8 && x != 16 && x != 32 && x != 64))
                return mdp_set_error(MDP_EINVAL, "MDP_CHAIN_NM=%s (expected 8, 16, 32 or 64)", v.c_str());
            o->nm = (uint32_t)x;
            return MDP_OK;
        }
        if (k == "MDP_CHAIN_LAUNCH_PTS") {
            if (!chain_decimal(v, &x))
                return mdp_set_error(MDP_EINVAL, "MDP_CHAIN_LAUNCH_PTS=%s (expected a decimal count)", v.c_str());
            o->launch_pts = x;
            return MDP_OK;
        }
        if (k == "MDP_CHAIN_PARTS") {
            if (!chain_decimal(v, &x))
                return mdp_set_error(MDP_EINVAL, "MDP_CHAIN_PARTS=%s (expected a decimal count)", v.c_str());
            o->parts = x;
            return MDP_OK;
        }
        return mdp_set_error(MDP_EINVAL, "unknown scenario chain option '%s'", k.c_str());
    });
}

int chain_plan(const int32_t *row, uint32_t n, double m, float p, double d, int kind, const ChainOpts &opts,
               ChainPlan *plan)
{
    if (!row || !plan || n == 0) return mdp_set_error(MDP_EINVAL, "empty survey row");
    if (kind != 0 && kind != 1) return mdp_set_error(MDP_EINVAL, "scenario kind %d (expected 0 or 1)", kind);
    if (n > kChainMaxN)
        return mdp_set_error(MDP_EUNSUPPORTED, "%u patches: the scenario chain holds <= %u", n, kChainMaxN);
    if (int rc = scn_check_row(row, n)) return rc;
    if (!(m > 0) && !(m < 0)) return mdp_set_error(MDP_EINVAL, "mean dispersal -m must be non-zero");
    if (opts.nm && opts.nm < chain_nm(n))
        return mdp_set_error(MDP_EINVAL, "MDP_CHAIN_NM=%u is smaller than the k_scnchain<%u> that %u patches need",
                             opts.nm, chain_nm(n), n);
    ChainPlan &s = *plan;
    s = ChainPlan();
    s.n = n;
    s.kind = kind;
    s.m = m;
    s.p = (double)p;
    s.opts = opts;
    s.nm = opts.nm ? opts.nm : chain_nm(n);
    for (uint32_t j = 0; j < n; ++j) {
        s.n1 += row[j] == 1;
        s.nmiss += row[j] == -1;
    }
    s.M.assign((size_t)s.nm * s.nm, 0.0);
    scn_dispersal(n, m, d, s.nm, s.M.data());
    // target[n1 + j] = (C(nmiss, j) p^j) (1 - p)^(nmiss - j): the number of
    // occupied patches of the row, its missing ones independent with prior p
    std::vector<uint64_t> binom(s.nmiss + 1, 0);  // Pascal's rule: C(64, 32) < 2^61
    binom[0] = 1;
    for (uint32_t i = 1; i <= s.nmiss; ++i)
        for (uint32_t j = i; j >= 1; --j) binom[j] += binom[j - 1];
    s.target.assign(n + 1, 0.0);
    for (uint32_t j = 0; j <= s.nmiss; ++j)
        s.target[s.n1 + j] = ((double)binom[j] * pow(s.p, (double)j)) * pow(1.0 - s.p, (double)(s.nmiss - j));
    return MDP_OK;
}

void chain_src(const ChainPlan &plan, bool baseline, const double *dsrc, uint32_t nd, std::vector<double> *src)
{
    if (baseline || plan.kind != 1) nd = 1;
    src->assign((size_t)nd * plan.nm, 0.0);
    if (!baseline && plan.kind == 1) scn_source_rows(plan.n, plan.m, dsrc, nd, plan.nm, src->data());
}

int chain_call(const ChainPlan &plan, bool baseline, const double *e, uint32_t ne, const double *c, uint32_t nc,
               const double *K, uint32_t nK, const double *dsrc, uint32_t nd, uint64_t nrep, bool host_table,
               ChainCall *call)
{
    if (!call) return mdp_set_error(MDP_EINVAL, "null argument");
    *call = ChainCall();
    if (!e || !c || ne == 0 || nc == 0) return mdp_set_error(MDP_EINVAL, "empty grid axis");
    if (!baseline && (!K || nK == 0 || nd == 0 || (plan.kind == 1 && !dsrc)))
        return mdp_set_error(MDP_EINVAL, "empty grid axis");
    for (uint32_t i = 0; i < ne; ++i)
        if (!(e[i] >= 0) || !std::isfinite(e[i])) return mdp_set_error(MDP_EINVAL, "e[%u] must be finite and >= 0", i);
    for (uint32_t i = 0; i < nc; ++i)
        if (!(c[i] >= 0) || !std::isfinite(c[i])) return mdp_set_error(MDP_EINVAL, "c[%u] must be finite and >= 0", i);
    for (uint32_t i = 0; !baseline && i < nK; ++i)
        if (!(K[i] > 0) || !std::isfinite(K[i])) return mdp_set_error(MDP_EINVAL, "K[%u] must be finite and > 0", i);
    for (uint32_t i = 0; !baseline && dsrc && i < nd; ++i)
        if (!(dsrc[i] >= 0) || !std::isfinite(dsrc[i]))
            return mdp_set_error(MDP_EINVAL, "dsrc[%u] must be finite and >= 0", i);
    uint64_t G = 0;
    if (int rc = chain_points(baseline, ne, nc, nK, nd, &G)) return rc;
    const uint64_t per_point = (uint64_t)(plan.n + 1) * (plan.n + 1);
    if (host_table && G * per_point > kChainMaxCells)
        return mdp_set_error(MDP_EUNSUPPORTED, "table of more than %llu cells", (unsigned long long)kChainMaxCells);
    if (nrep > kChainMaxReps)
        return mdp_set_error(MDP_EUNSUPPORTED, "%llu replicates: <= %llu per call", (unsigned long long)nrep,
                             (unsigned long long)kChainMaxReps);
    ChainCall &s = *call;
    s.G = G;
    s.tiles_per_class = (nrep + kChainBlock - 1) / kChainBlock;
    s.tiles_per_point = s.tiles_per_class * (plan.n + 1);
    s.cells = G * per_point;
    if (nrep == 0) return MDP_OK;
    const uint64_t fit = std::max<uint64_t>(1, kChainTableBytes / (per_point * sizeof(uint32_t)));
    const uint64_t per = std::min(G, plan.opts.launch_pts ? plan.opts.launch_pts : fit);
    for (uint64_t p0 = 0; p0 < G; p0 += per) {
        ChainLaunch l;
        l.p0 = p0;
        l.npts = std::min(per, G - p0);
        // few points (a baseline table has ne*nc, often 1): many workgroups
        // share each; thousands of points: one workgroup per point
        const uint64_t want = plan.opts.parts ? plan.opts.parts : (kChainFillWG + l.npts - 1) / l.npts;
        l.parts = std::max<uint64_t>(1, std::min(want, s.tiles_per_point));
        l.units = l.npts * l.parts;
        l.nwg = (uint32_t)std::min<uint64_t>(l.units, kChainMaxWG);
        s.launches.push_back(l);
    }
    return MDP_OK;
}

int chain_eval_check(const ChainPlan &plan, int ts, int tdis, uint64_t nrep, uint64_t nbase, const double *start,
                     const double *target)
{
    if (ts < 0 || tdis < 0) return mdp_set_error(MDP_EINVAL, "negative duration (ts %d, tdis %d)", ts, tdis);
    if (nrep == 0 || nbase == 0) return mdp_set_error(MDP_EINVAL, "no replicates");
    if (int rc = chain_check_weights("start", start, plan.n)) return rc;
    if (int rc = chain_check_weights("target", target, plan.n)) return rc;
    if ((uint64_t)ts + (uint64_t)tdis > kChainMaxYears)
        return mdp_set_error(MDP_EUNSUPPORTED, "%llu years: the scenario chain runs <= %u",
                             (unsigned long long)ts + (unsigned long long)tdis, kChainMaxYears);
    if (nrep > kChainMaxReps || nbase > kChainMaxReps)
        return mdp_set_error(MDP_EUNSUPPORTED, "%llu replicates: <= %llu per call",
                             (unsigned long long)std::max(nrep, nbase), (unsigned long long)kChainMaxReps);
    return MDP_OK;
}

void chain_weights(const ChainPlan &plan, const double *start, const double *target, std::vector<double> *w_start,
                   std::vector<double> *w_target)
{
    const uint32_t nc = plan.n + 1;
    if (start) w_start->assign(start, start + nc);
    else w_start->assign(nc, 1.0 / (double)nc);
    if (target) w_target->assign(target, target + nc);
    else *w_target = plan.target;
}

int chain_eval(const ChainPlan &plan, int ts, int tdis, uint32_t ne, uint32_t nc, uint32_t nK, uint32_t nd,
               const uint64_t *cnt_scn, uint64_t nrep, const uint64_t *cnt_base, uint64_t nbase, const double *start,
               const double *target, double *out, double *by_class)
{
    if (!cnt_scn || !cnt_base || !out) return mdp_set_error(MDP_EINVAL, "null argument");
    if (int rc = chain_eval_check(plan, ts, tdis, nrep, nbase, start, target)) return rc;
    uint64_t G = 0;
    if (int rc = chain_points(false, ne, nc, nK, nd, &G)) return rc;
    const uint32_t ncl = plan.n + 1;
    std::vector<double> ws, wt;
    chain_weights(plan, start, target, &ws, &wt);
    std::vector<double> mat((size_t)ncl * ncl), v(ncl), nv(ncl), vb(ncl);
    // v <- mat v, `steps` times; mat = cnt / den
    auto power = [&](const uint64_t *cnt, uint64_t den, int steps) {
        if (steps == 0) return;
        for (size_t i = 0; i < mat.size(); ++i) mat[i] = (double)cnt[i] / (double)den;
        for (int t = 0; t < steps; ++t) {
            for (uint32_t k = 0; k < ncl; ++k) {
                double s = 0.0;
                for (uint32_t l = 0; l < ncl; ++l) s += mat[(size_t)k * ncl + l] * v[l];
                nv[k] = s;
            }
            v.swap(nv);
        }
    };
    const uint64_t inner = (uint64_t)nK * nd;
    for (uint64_t b = 0; b < (uint64_t)ne * nc; ++b) {
        v = wt;
        power(cnt_base + b * ncl * ncl, nbase, tdis);
        vb = v;
        for (uint64_t g = b * inner; g < (b + 1) * inner; ++g) {
            v = vb;
            power(cnt_scn + g * ncl * ncl, nrep, ts);
            double s = 0.0;
            for (uint32_t k = 0; k < ncl; ++k) {
                if (by_class) by_class[g * ncl + k] = v[k];
                s += ws[k] * v[k];
            }
            out[g] = s;
        }
    }
    return MDP_OK;
}
