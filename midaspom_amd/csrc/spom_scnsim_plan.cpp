// midaspom_amd/csrc/spom_scnsim_plan.cpp -- host planning of the simulated
// scenario likelihoods (spom_scnsim_plan.h): option parsing, the refusals,
// the dispersal and source tables, the row's masks, completions and float
// priors, the launches of a call and the likelihood estimate.  Host only.
#include "spom_scnsim_plan.h"

#include <algorithm>
#include <cmath>
#include <string>

#include "spom_opts.h"
#include "spom_scn_row.h"

namespace {

// 1 to 19 decimal digits
bool sim_decimal(const std::string &v, uint64_t *out)
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

}  // namespace

int sim_parse_opts(const char *s, SimOpts *o)
{
    *o = SimOpts();
    return mdp_for_each_opt(s, [&](const std::string &k, const std::string &v, bool) -> int {
        uint64_t x = 0;
        if (k == "MDP_SIM_NM") {
            if (!sim_decimal(v, &x) || (x != 8 && x != 16 && x != 32 && x != 64))
                return mdp_set_error(MDP_EINVAL, "MDP_SIM_NM=%s (expected 8, 16, 32 or 64)", v.c_str());
            o->nm = (uint32_t)x;
            return MDP_OK;
        }
        if (k == "MDP_SIM_NP") {
            if (!sim_decimal(v, &x) || (x != 1 && x != 2 && x != 4 && x != 8))
                return mdp_set_error(MDP_EINVAL, "MDP_SIM_NP=%s (expected 1, 2, 4 or 8)", v.c_str());
            o->np = (uint32_t)x;
            return MDP_OK;
        }
        if (k == "MDP_SIM_WAVE") {
            if (v == "0") o->wave = kSimWaveOff;
            else if (v == "auto") o->wave = kSimWaveAuto;
            else if (v == "1") o->wave = kSimWaveOn;
            else return mdp_set_error(MDP_EINVAL, "MDP_SIM_WAVE=%s (expected 0, auto or 1)", v.c_str());
            return MDP_OK;
        }
        if (k == "MDP_SIM_LAUNCH_PTS") {
            if (!sim_decimal(v, &x))
                return mdp_set_error(MDP_EINVAL, "MDP_SIM_LAUNCH_PTS=%s (expected a decimal count)", v.c_str());
            o->launch_pts = x;
            return MDP_OK;
        }
        return mdp_set_error(MDP_EINVAL, "unknown scenario simulation option '%s'", k.c_str());
    });
}

int sim_plan(const int32_t *row, uint32_t n, double m, float p, double d, int kind, const SimOpts &opts,
             SimPlan *plan)
{
    if (!row || !plan || n == 0) return mdp_set_error(MDP_EINVAL, "empty survey row");
    if (kind != 0 && kind != 1) return mdp_set_error(MDP_EINVAL, "scenario kind %d (expected 0 or 1)", kind);
    const uint32_t maxn = opts.wave == kSimWaveOff ? kSimMaxN : kSimWaveMaxN;
    if (n > maxn)
        return mdp_set_error(MDP_EUNSUPPORTED, "%u patches: the scenario simulator holds <= %u", n, maxn);
    if (int rc = scn_check_row(row, n)) return rc;
    if (!(m > 0) && !(m < 0)) return mdp_set_error(MDP_EINVAL, "mean dispersal -m must be non-zero");
    // the kernel family: k_scnsim<NM>, or k_scnsim_wave<NP>
    const bool wave = opts.wave == kSimWaveOn || (opts.wave == kSimWaveAuto && n > kSimMaxN);
    if (wave && opts.nm)
        return mdp_set_error(MDP_EINVAL, "MDP_SIM_NM=%u with k_scnsim_wave selected for %u patches", opts.nm, n);
    if (!wave && opts.np)
        return mdp_set_error(MDP_EINVAL, "MDP_SIM_NP=%u with k_scnsim selected for %u patches", opts.np, n);
    if (!wave && opts.nm && opts.nm < sim_nm(n))
        return mdp_set_error(MDP_EINVAL, "MDP_SIM_NM=%u is smaller than the k_scnsim<%u> that %u patches need", opts.nm,
                             sim_nm(n), n);
    if (wave && opts.np && opts.np < sim_np(n))
        return mdp_set_error(MDP_EINVAL, "MDP_SIM_NP=%u is smaller than the k_scnsim_wave<%u> that %u patches need",
                             opts.np, sim_np(n), n);
    SimPlan &s = *plan;
    s = SimPlan();
    s.n = n;
    s.kind = kind;
    s.m = m;
    s.opts = opts;
    for (uint32_t j = 0; j < n; ++j)
        if (row[j] == -1) s.miss.push_back(j);
    s.nmiss = (uint32_t)s.miss.size();
    // the float priors of the completions: the scenario engine's own (spom_scn_row.h)
    if (s.nmiss <= kSimMaxMatchMissing) scn_priors(s.nmiss, p, &s.prior);
    if (!wave) {
        s.nm = opts.nm ? opts.nm : sim_nm(n);
        s.live = n == 64 ? ~0ull : (1ull << n) - 1;
        for (uint32_t j = 0; j < n; ++j) {
            if (row[j] == 1) s.fixed |= 1ull << j;
            else if (row[j] == -1) s.missmask |= 1ull << j;
        }
        // dispersal, unscaled: the scenario engine's own (spom_scn_row.h)
        s.M.assign((size_t)s.nm * s.nm, 0.0);
        scn_dispersal(n, m, d, s.nm, s.M.data());
        return MDP_OK;
    }
    s.np = opts.np ? opts.np : sim_np(n);
    s.wfixed.assign(64, 0u);
    s.wmissmask.assign(64, 0u);
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t pair = k >> 1, lane = pair & 63u, bit = 2 * (pair >> 6) + (k & 1u);
        if (row[k] == 1) s.wfixed[lane] |= 1u << bit;
        else if (row[k] == -1) s.wmissmask[lane] |= 1u << bit, s.wmiss.push_back((lane << 8) | bit);
    }
    // the distance image: scn_dispersal's expression, so M's bits
    const double a = 1.0 / m;
    s.wlen = (n + 128 * s.np + 1) & ~1u;
    std::vector<double> G((size_t)s.wlen + 1, 0.0);
    for (uint32_t dist = 1; dist < n; ++dist) G[n - 1 - dist] = G[n - 1 + dist] = exp(-a * (double)dist * d);
    s.image.assign((size_t)2 * s.wlen, 0.0);
    for (uint32_t i = 0; i < s.wlen; ++i) {
        s.image[i] = G[i];
        s.image[(size_t)s.wlen + i] = G[i + 1];
    }
    return MDP_OK;
}

void sim_src(const SimPlan &plan, const double *dsrc, uint32_t nd, std::vector<double> *src)
{
    const uint32_t ld = sim_src_ld(plan);
    src->assign((size_t)nd * ld, 0.0);
    if (plan.kind == 1) scn_source_rows(plan.n, plan.m, dsrc, nd, ld, src->data());
}

int sim_call(const SimPlan &plan, int ts, int tdis, const double *e, uint32_t ne, const double *c, uint32_t nc,
             const double *K, uint32_t nK, const double *dsrc, uint32_t nd, uint64_t nrep, bool want_hist,
             bool want_match, SimCall *call)
{
    if (!call) return mdp_set_error(MDP_EINVAL, "null argument");
    *call = SimCall();
    if (!want_hist && !want_match) return mdp_set_error(MDP_EINVAL, "null hist and match");
    if (ts < 0 || tdis < 0) return mdp_set_error(MDP_EINVAL, "negative duration (ts %d, tdis %d)", ts, tdis);
    if (!e || !c || !K || ne == 0 || nc == 0 || nK == 0 || nd == 0 || (plan.kind == 1 && !dsrc))
        return mdp_set_error(MDP_EINVAL, "empty grid axis");
    for (uint32_t i = 0; i < ne; ++i)
        if (!(e[i] >= 0) || !std::isfinite(e[i])) return mdp_set_error(MDP_EINVAL, "e[%u] must be finite and >= 0", i);
    for (uint32_t i = 0; i < nc; ++i)
        if (!(c[i] >= 0) || !std::isfinite(c[i])) return mdp_set_error(MDP_EINVAL, "c[%u] must be finite and >= 0", i);
    for (uint32_t i = 0; i < nK; ++i)
        if (!(K[i] > 0) || !std::isfinite(K[i])) return mdp_set_error(MDP_EINVAL, "K[%u] must be finite and > 0", i);
    for (uint32_t i = 0; dsrc && i < nd; ++i)
        if (!(dsrc[i] >= 0) || !std::isfinite(dsrc[i]))
            return mdp_set_error(MDP_EINVAL, "dsrc[%u] must be finite and >= 0", i);
    if (want_match && plan.nmiss > kSimMaxMatchMissing)
        return mdp_set_error(MDP_EUNSUPPORTED, "%u missing patches: the match table holds <= 2^%u completions "
                             "(the histogram alone takes any number)", plan.nmiss, kSimMaxMatchMissing);
    if ((uint64_t)ts + (uint64_t)tdis > kSimMaxYears)
        return mdp_set_error(MDP_EUNSUPPORTED, "%llu years: the scenario simulator runs <= %u",
                             (unsigned long long)ts + (unsigned long long)tdis, kSimMaxYears);
    // every partial product stays below 2^52 before it is compared
    uint64_t G = (uint64_t)ne * nc;
    if (G <= kSimMaxPoints) G *= nK;
    if (G <= kSimMaxPoints) G *= nd;
    if (G > kSimMaxPoints)
        return mdp_set_error(MDP_EUNSUPPORTED, "grid of more than %llu points", (unsigned long long)kSimMaxPoints);
    const uint64_t hc = G * (plan.n + 1), mc = want_match ? G << plan.nmiss : 0;
    if ((want_hist && hc > kSimMaxCells) || mc > kSimMaxCells)
        return mdp_set_error(MDP_EUNSUPPORTED, "table of more than %llu cells", (unsigned long long)kSimMaxCells);
    if (nrep > kSimMaxReps)
        return mdp_set_error(MDP_EUNSUPPORTED, "%llu replicates: <= %llu per call", (unsigned long long)nrep,
                             (unsigned long long)kSimMaxReps);
    SimCall &s = *call;
    s.G = G;
    const uint64_t per_tile = plan.np ? kSimWaveReps : kSimBlock;
    s.tiles_per_point = (nrep + per_tile - 1) / per_tile;
    s.hist_cells = hc;
    s.match_cells = G << std::min(plan.nmiss, kSimMaxMatchMissing);
    if (nrep == 0) return MDP_OK;
    const uint64_t per = plan.opts.launch_pts ? std::min(plan.opts.launch_pts, G) : G;
    for (uint64_t p0 = 0; p0 < G; p0 += per) {
        SimLaunch l;
        l.p0 = p0;
        l.npts = std::min(per, G - p0);
        l.tiles = l.npts * s.tiles_per_point;
        l.nwg = (uint32_t)std::min<uint64_t>(l.tiles, kSimMaxWG);
        s.launches.push_back(l);
    }
    return MDP_OK;
}

int sim_lik(const SimPlan &plan, const uint64_t *match, size_t npoints, uint64_t nrep, double *out)
{
    if (!match || !out) return mdp_set_error(MDP_EINVAL, "null argument");
    if (nrep == 0) return mdp_set_error(MDP_EINVAL, "no replicates");
    if (plan.nmiss > kSimMaxMatchMissing)
        return mdp_set_error(MDP_EUNSUPPORTED, "%u missing patches: no match table", plan.nmiss);
    const size_t np = (size_t)1 << plan.nmiss;
    const double scale = ldexp(1.0, (int)std::min(plan.n, kSimMaxN));
    for (size_t g = 0; g < npoints; ++g) {
        double s = 0.0;
        for (size_t j = 0; j < np; ++j) s += (double)plan.prior[j] * (double)match[g * np + j];
        // beyond 64 patches 2^n may not be a double (inf at n = 1024, and inf * 0 is NaN):
        // scale the mean instead, the same value wherever (s 2^n) / nrep is finite
        out[g] = plan.n <= kSimMaxN ? s * scale / (double)nrep : ldexp(s / (double)nrep, (int)plan.n);
    }
    return MDP_OK;
}
