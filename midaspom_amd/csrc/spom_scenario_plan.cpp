// midaspom_amd/csrc/spom_scenario_plan.cpp -- host planning of the exact
// scenario engine (spom_scenario_plan.h).  Host only.
#include "spom_scenario_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "spom_opts.h"
#include "spom_scn_row.h"

int scn_parse_opts(const char *s, ScnOpts *o)
{
    *o = ScnOpts();
    return mdp_for_each_opt(s, [&](const std::string &k, const std::string &v, bool has) -> int {
        const bool on = !has || atoi(v.c_str()) != 0;
        if (k == "MDP_SCN_BIG") o->big = on;
        else if (k == "MDP_SCN_ROW") o->row = on;
        else if (k == "MDP_SCN_LAUNCH_PTS") {
            const long pts = has ? atol(v.c_str()) : 0;
            o->launch_pts = pts > 0 ? std::min<uint64_t>((uint64_t)pts, 1ull << 32) : 0;
        } else return mdp_set_error(MDP_EINVAL, "unknown scenario option '%s'", k.c_str());
        return MDP_OK;
    });
}

namespace {

// hi factor table offsets (rows jh ascending, 2^(NH-|jh|) supersets x 2^NL lo
// rows each) and the hi-row schedule: rows dealt to the waves by
// longest-processing-time-first (row jh costs its 2^(f-1) superset pairs,
// f = NH - |jh|, plus one for its loads and epilogue)
void scn_lds_tables(ScnPlan &s)
{
    const uint32_t nl = scn_nl(s.n), nh = s.n - nl, nhi = 1u << nh;
    s.boff.assign(nhi, 0);
    uint32_t off = 0;
    for (uint32_t jh = 0; jh < nhi; ++jh) {
        s.boff[jh] = off;
        off += (1u << (nh - __builtin_popcount(jh))) << nl;
    }
    s.btot = off;
    std::vector<uint32_t> rows(nhi);
    for (uint32_t jh = 0; jh < nhi; ++jh) rows[jh] = jh;
    auto cost = [&](uint32_t jh) {
        const uint32_t f = nh - __builtin_popcount(jh);
        return (f ? 1u << (f - 1) : 1u) + 1u;
    };
    std::stable_sort(rows.begin(), rows.end(), [&](uint32_t x, uint32_t y) { return cost(x) > cost(y); });
    std::vector<std::vector<uint32_t>> grp(kWaves);
    std::vector<uint64_t> load(kWaves, 0);
    for (uint32_t jh : rows) {
        const size_t g = (size_t)(std::min_element(load.begin(), load.end()) - load.begin());
        grp[g].push_back(jh);
        load[g] += cost(jh);
    }
    size_t mx = 0;
    for (auto &v : grp) mx = std::max(mx, v.size());
    s.nsched = (uint32_t)mx;
    s.jsched.assign(mx * kWaves, 0xffffffffu);
    for (uint32_t g = 0; g < (uint32_t)kWaves; ++g)
        for (size_t i = 0; i < grp[g].size(); ++i) s.jsched[g * mx + i] = grp[g][i];
    const size_t na = (size_t)((pow3((int)nl) + 1) & ~1) << nh;
    s.lds = (2 * ((size_t)s.ns * kE + (2u << nl)) + na + s.btot + (1u << nl)) * sizeof(double);
    snprintf(s.kname, sizeof s.kname, "k_scn<%u,%u>", nl, nh);
}

}  // namespace

int scn_plan(const int32_t *row, uint32_t n, double m, float p, double d, int kind, const ScnOpts &opts,
             ScnPlan *plan)
{
    if (!row || !plan || n == 0) return mdp_set_error(MDP_EINVAL, "null argument");
    if (n > kBigMaxN)
        return mdp_set_error(MDP_EUNSUPPORTED, "%u patches: the scenario engine takes n <= %u (2^n states)", n,
                             kBigMaxN);
    if (int rc = scn_check_row(row, n)) return rc;
    ScnPlan &s = *plan;
    s = ScnPlan();
    s.n = n;
    const uint32_t ns = s.ns = 1u << n;
    s.kind = kind;
    s.m = m;
    s.d = d;
    s.launch_pts = opts.launch_pts;
    // n > 8: the LDS-resident k_scn does not fit; 8 < n <= 12: k_scn_row
    // (MDP_SCN_ROW=1 forces it for any n <= 12); n > 12: k_scn_big
    // (MDP_SCN_BIG=1 forces it for any n)
    if (!opts.big && n <= kRowMaxN && (n > kMaxN || opts.row)) s.path = kScnRow;
    else if (n > kMaxN || opts.big) s.path = kScnBig;
    // colonisation sums S[j][k] = sum over l != k, ascending, of M[l][k] * j_l (dieoff.c:72-77)
    std::vector<double> M((size_t)n * n, 0.0);
    scn_dispersal(n, m, d, n, M.data());
    s.S.assign((size_t)ns * n, 0.0);
    for (uint32_t j = 0; j < ns; ++j)
        for (uint32_t k = 0; k < n; ++k) {
            double s1 = 0;
            for (uint32_t l = 0; l < n; ++l)
                if (l != k) s1 += M[l * n + k] * (double)((j >> (n - 1 - l)) & 1u);
            s.S[(size_t)j * n + k] = s1;
        }
    // w[state] = float prior of the completion with that state (dieoff.c:198-232):
    // patch j is bit n-1-j, the q-th missing patch bit nmiss-1-q of the completion
    uint32_t fixed = 0, nmiss = 0;
    std::vector<uint32_t> missbit;
    for (uint32_t j = 0; j < n; ++j) {
        if (row[j] == 1) fixed |= 1u << (n - 1 - j);
        else if (row[j] == -1) missbit.push_back(n - 1 - j), ++nmiss;
    }
    std::vector<float> pr;
    scn_priors(nmiss, p, &pr);
    s.w.assign(ns, 0.0);
    for (uint32_t k = 0; k < pr.size(); ++k) {
        uint32_t st = fixed;
        for (uint32_t q = 0; q < nmiss; ++q) st |= ((k >> (nmiss - 1 - q)) & 1u) << missbit[q];
        s.w[st] += (double)pr[k];
    }
    if (s.path == kScnRow) {  // rows by decreasing free-patch count (stable: ascending j within a count)
        s.jord.resize(ns);
        for (uint32_t j = 0; j < ns; ++j) s.jord[j] = j;
        std::stable_sort(s.jord.begin(), s.jord.end(),
                         [](uint32_t x, uint32_t y) { return __builtin_popcount(x) < __builtin_popcount(y); });
        s.lds = (2 * (size_t)ns + 3 * (size_t)n * kRowBlock) * sizeof(double);
        snprintf(s.kname, sizeof s.kname, "k_scn_row");
    } else if (s.path == kScnBig) {
        snprintf(s.kname, sizeof s.kname, "k_scn_big");
    } else {
        scn_lds_tables(s);
    }
    return MDP_OK;
}

int scn_grid_plan(const ScnPlan &plan, int ts, int tdis, const double *e, uint32_t ne, const double *c, uint32_t nc,
                  const double *K, uint32_t nK, const double *dsrc, uint32_t nd, ScnGrid *grid)
{
    if (!grid || (ne && !e) || (nc && !c) || (nK && !K)) return mdp_set_error(MDP_EINVAL, "null argument");
    if (ts < 0 || tdis < 0) return mdp_set_error(MDP_EINVAL, "negative number of years");
    if (plan.kind == 1) {
        if (nd && !dsrc) return mdp_set_error(MDP_EINVAL, "null source distances");
    } else {
        nd = 1;
    }
    ScnGrid &g = *grid;
    g = ScnGrid();
    g.ts = ts, g.tdis = tdis;
    if (!ne || !nc || !nK || !nd) return MDP_OK;
    // workgroups of k_scn's second pass; every partial product is below 2^63
    const uint64_t lim = 0x7fffffffull;
    const uint64_t nwg0 = (ne + (uint64_t)kE - 1) / kE * nc;  // and of its first
    uint64_t nwg = nwg0;
    if (nwg <= lim) nwg *= nK;
    if (nwg <= lim) nwg *= nd;
    if (nwg > lim)
        return mdp_set_error(MDP_EUNSUPPORTED, "grid of %.0Lf points too large", (long double)ne * nc * nK * nd);
    g.ne = ne, g.nc = nc, g.nK = nK, g.nd = nd;
    const uint32_t n = plan.n, ns = plan.ns;
    g.src.assign((size_t)nd * n, 0.0);
    if (plan.kind == 1) scn_source_rows(n, plan.m, dsrc, nd, n, g.src.data());
    g.nV = (size_t)nc * ns * ne;
    const uint64_t tot[2] = {(uint64_t)nc * ne, (uint64_t)ne * nc * nK * nd};
    uint64_t per = 0;  // points per launch (k_scn: one launch per pass)
    if (plan.path == kScnRow) {
        per = plan.launch_pts ? std::min<uint64_t>(plan.launch_pts, kRowPer) : kRowPer;
    } else if (plan.path == kScnBig) {  // two state vectors per point within kBigScratch
        size_t pts = kBigScratch / (2 * (size_t)ns * sizeof(double));
        pts = std::max<size_t>(kBigBlock, std::min<size_t>(pts, std::max(tot[0], tot[1]) + kBigBlock - 1) / kBigBlock * kBigBlock);
        if (plan.launch_pts)  // the cap, rounded up to whole blocks
            pts = std::min<size_t>(pts, (plan.launch_pts + kBigBlock - 1) / kBigBlock * kBigBlock);
        per = g.big_pts = (uint32_t)std::min<size_t>(pts, (size_t)65535 * kBigBlock);
        g.nY = 2 * (size_t)ns * g.big_pts;
    }
    for (int mode = 0; mode < 2; ++mode) {
        if (plan.path == kScnLds) {
            g.launches[mode].push_back({0, tot[mode], (uint32_t)(mode ? nwg : nwg0)});
            continue;
        }
        for (uint64_t p0 = 0; p0 < tot[mode]; p0 += per) {
            const uint64_t pts = std::min(per, tot[mode] - p0);
            g.launches[mode].push_back({p0, pts, plan.path == kScnRow ? (uint32_t)pts : g.big_pts / kBigBlock});
        }
    }
    return MDP_OK;
}

extern "C" {

double mdp_kgrid(uint32_t s, double lo, double hi, double *K)
{
    // dieoff.c:284-286 / loss.c:315-317
    for (uint32_t i = 0; i < s; ++i)
        K[i] = pow(10.0, ((double)i) / (s - 1) * (log10(hi) - log10(lo)) + log10(lo));
    return s ? K[0] : 0.0;
}

double mdp_dgrid(uint32_t s, double lo, double hi, double *dv)
{
    // loss.c:319-322
    for (uint32_t i = 0; i < s; ++i) dv[i] = i * (hi - lo) / (s - 1) + lo;
    return s ? dv[0] : 0.0;
}

}  // extern "C"
