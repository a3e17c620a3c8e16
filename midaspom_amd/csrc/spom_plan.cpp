// midaspom_amd/csrc/spom_plan.cpp -- host planning of the posterior engine:
// option parsing (one table, kEngineOpts, converts every value once into a
// field of MdpOpts; nothing after it reads option text), the engine plan as a
// sequence of steps (mdp_plan_engine), the generic / direct / chunked / wide
// plan tables the kernels index (spom_engine.h holds the shared constants), the hipRTC
// forward sources, per grid the c tables and the grid plan (mdp_plan_grid:
// the forward variant, the point list, the chunk widths, every buffer size
// and the forward launch's shape) and the host-only part of the C ABI (work
// counts, engine info).  No HIP runtime call: the device's LDS limit and its
// CU count arrive as arguments, so this unit links into a stand-alone program
// (plan_check.cpp) as it links into libmidaspom.so.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <set>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "spom_engine.h"
#include "spom_opts.h"

// Engine options (ABI 7, mdp_engine_create_opts): "NAME=VALUE" pairs
// separated by ';', ',' or white space.  They select among the engine's
// parity-tested kernel variants; the defaults are the
// measured best.  The library reads no tuning knob from the environment:
// mdp_engine_create is mdp_engine_create_opts with no options.  Names
// marked measurement-only exist in the diag build alone (-DMDP_DIAG_BUILD,
// libmidaspom_diag.so, used by scripts/): MDP_JIT_HACK's kernels do not
// store correct results, and phase stamps / occupancy hints are profiling
// aids.  An unknown name, or a measurement-only name in the default
// build, is MDP_EINVAL.  A value is never refused: each row below converts
// its text leniently (atoi: text that is no number is 0), a name without '='
// has the value "1", and a repeated name takes its last value.
namespace {
struct OptDef {
    const char *name;
    bool diag;  // measurement-only
    void (*set)(MdpOpts &o, const char *v);
};
inline bool on(const char *v) { return atoi(v) != 0; }
inline int clampi(int lo, int v, int hi) { return std::max(lo, std::min(hi, v)); }
// The one list of the accepted names, with what each value means.
const OptDef kEngineOpts[] = {
    {"MDP_JIT", false, [](MdpOpts &o, const char *v) { o.jit = strcmp(v, "0") != 0; }},
    {"MDP_WIDE", false, [](MdpOpts &o, const char *v) { o.wide = on(v); }},
    {"MDP_FWD", false, [](MdpOpts &o, const char *v) { o.fwd_scalar = !strcmp(v, "scalar"); }},
    {"MDP_EPL", false, [](MdpOpts &o, const char *v) { o.epl = atoi(v); }},
    {"MDP_QGLOBAL", false, [](MdpOpts &o, const char *v) { o.qglobal = on(v); }},
    {"MDP_JIT_GATHER", false, [](MdpOpts &o, const char *v) { o.gather = on(v); }},
    {"MDP_JIT_CHECK", false, [](MdpOpts &o, const char *v) { o.jit_check = on(v); }},
    {"MDP_JIT_VERBOSE", false, [](MdpOpts &o, const char *) { o.jit_verbose = true; }},
    {"MDP_FUSED", false, [](MdpOpts &o, const char *v) { o.fused = on(v); }},
    {"MDP_JIT_XCD", false, [](MdpOpts &o, const char *v) { o.jit_xcd = on(v); }},
    {"MDP_JIT_EFAST", false, [](MdpOpts &o, const char *v) { o.jit_efast = on(v); }},
    {"MDP_QROWS_XCD", false, [](MdpOpts &o, const char *v) { o.qrows_xcd = on(v); }},
    {"MDP_FAST_LOG", false, [](MdpOpts &o, const char *v) { o.fast_log = on(v); }},
    {"MDP_JIT_SPLIT", false, [](MdpOpts &o, const char *v) { o.jit_split = on(v); }},
    {"MDP_JIT_ROT", false, [](MdpOpts &o, const char *v) { o.jit_rot = on(v); }},
    {"MDP_FUSED_COLS", false, [](MdpOpts &o, const char *v) { o.fused_cols = clampi(1, atoi(v), 4); }},
    {"MDP_JIT_SLOTS", false, [](MdpOpts &o, const char *v) { o.jit_slots = atoi(v); }},
    {"MDP_JIT_WINDOW", false, [](MdpOpts &o, const char *v) { o.jit_window = atoi(v); }},
    {"MDP_WIDE_MMA", false, [](MdpOpts &o, const char *v) { o.wide_mma = atoi(v); }},
    {"MDP_JIT_THREADS", false, [](MdpOpts &o, const char *v) { o.jit_threads = atoi(v); }},
    {"MDP_JIT_KBLOCK", false, [](MdpOpts &o, const char *v) { o.jit_kblock = atoi(v) == 512 ? 512 : 256; }},
    {"MDP_JIT_CHUNK", false, [](MdpOpts &o, const char *v) { o.jit_chunk = (uint32_t)std::max(1, atoi(v)); }},
    {"MDP_VLDS_MAXUSES", false, [](MdpOpts &o, const char *v) { o.vlds_maxuses = (uint32_t)std::max(0, atoi(v)); }},
    {"MDP_VLDS_EPL", false, [](MdpOpts &o, const char *v) { o.vlds_epl = atoi(v) == 2 ? 2 : 1; }},
    {"MDP_VSPLIT", false, [](MdpOpts &o, const char *v) { o.vsplit = atoi(v) == 1 ? 1 : atoi(v) == 2 ? 2 : 4; }},
    {"MDP_HS_RADIX", false, [](MdpOpts &o, const char *v) { o.hs_radix = (uint32_t)clampi(1, atoi(v), (int)kHsRadix); }},
    {"MDP_HS_WAVES", false, [](MdpOpts &o, const char *v) { o.hs_waves = atoi(v) == 8 ? 8u : 16u; }},
    {"MDP_WIDE_CB", false, [](MdpOpts &o, const char *v) { o.wide_cb = std::max(1, atoi(v)); }},
    {"MDP_JIT_DUMP", false, [](MdpOpts &o, const char *v) { o.jit_dump = v; }},
    {"MDP_DIAG", true, [](MdpOpts &o, const char *v) { o.diag = on(v); }},
    {"MDP_JIT_HACK", true, [](MdpOpts &o, const char *v) { o.jit_hack = atoi(v); }},
    {"MDP_JIT_WPE", true, [](MdpOpts &o, const char *v) { o.jit_wpe = atoi(v); }},
    {"MDP_HS_PROBE", true, [](MdpOpts &o, const char *v) { o.hs_probe = (uint32_t)atoi(v) & 7u; }},
};
}  // namespace

int parse_engine_opts(const char *s, MdpOpts &o, bool diag_build)
{
    o = MdpOpts();
    return mdp_for_each_opt(s, [&](const std::string &k, const std::string &val, bool has) -> int {
        for (const OptDef &d : kEngineOpts) {
            if (k != d.name) continue;
            if (d.diag && !diag_build)
                return mdp_set_error(MDP_EINVAL, "option %s is measurement-only (libmidaspom_diag.so, -DMDP_DIAG_BUILD)",
                                     k.c_str());
            d.set(o, has ? val.c_str() : "1");
            return MDP_OK;
        }
        return mdp_set_error(MDP_EINVAL, "unknown engine option '%s'", k.c_str());
    });
}

namespace {

// limits only the planner applies
constexpr size_t kLdsBudget = 120 * 1024;  // dynamic LDS of k_coefs
constexpr uint32_t kJitMaxUses = 2048;     // uses of one forward kernel; longer series run in chunks
constexpr uint32_t kJitChunkUses = 1024;   // target uses per chunk (hipRTC time grows faster than the code)
constexpr uint32_t kVldsMaxStates = 64;     // wide years the specialised kernel takes (states in LDS;
                                            // 128-state years compile to MB-sized programs)
constexpr uint32_t kVldsMaxUses = 16384;    // ... up to this many uses (hipRTC time)
constexpr size_t kJitMaxLds = 64 * 1024;   // Pc row + Q block of the direct path
constexpr size_t kJitChunkQ = kJitMaxLds / sizeof(double) - 2;  // gathered coefficients per chunk

constexpr int kDegBuckets[] = {4, 8, 16, 24};

int select_variant(MdpEnginePlan *eng, bool &wide)
{
    uint32_t np = 0;
    for (uint32_t b : {1u, 2u, 4u, 8u, 16u})
        if (eng->npmax <= b) { np = b; break; }
    // a year with more than 16 states (over 4 missing patches) exceeds the
    // register-resident forward kernels: the wide path takes the problem
    if (!np) wide = true;
    uint32_t deg = 0;
    for (int b : kDegBuckets)
        if (eng->maxA <= (uint32_t)b) { deg = (uint32_t)b; break; }
    if (!deg) return mdp_set_error(MDP_EUNSUPPORTED, "%u occupied patches in one state (max %d)", eng->maxA, kMaxDeg);
    eng->deg = deg;
    eng->variant = wide ? 20000u + deg : np * 100 + deg;
    return MDP_OK;
}

// Host plan: distinct transition pairs (sorted by |A&B| descending for load
// balance in k_coefs), Q offsets, the per-use pair index in forward order, and
// the step program (runs of 1x1 transitions / general years).  wide: the
// problem is the wide kernels' (MDP_WIDE=1, or a year of more than 16 states),
// which take neither.
int build_plan(MdpEnginePlan *eng, const mdp_problem *p, bool &wide)
{
    eng->n = p->n;
    eng->tmax = p->tmax;
    eng->nvar = p->nvar;
    eng->nextid = p->nextid;
    if (p->nvar > 24)
        return mdp_set_error(MDP_EUNSUPPORTED, "%u variable columns (engine limit 24)", p->nvar);
    eng->nstates = 1u << p->nvar;
    eng->prior0 = (double)p->prior[0];
    wide = eng->opts.wide;
    eng->np.resize(p->tmax);
    eng->npmax = 1;
    for (uint32_t t = 0; t < p->tmax; ++t) {
        eng->np[t] = p->year_off[t + 1] - p->year_off[t];
        eng->npmax = std::max(eng->npmax, eng->np[t]);
    }
    eng->ystate.clear();
    for (uint32_t i = 0; i < p->year_off[p->tmax]; ++i)
        eng->ystate.push_back(p->year_ids[i] < p->nextid ? p->short_state[p->year_ids[i]] : ~0u);
    std::map<uint64_t, uint32_t> pair_index;
    std::vector<uint32_t> A0, B0, use0;
    for (uint32_t t = 1; t < p->tmax; ++t) {
        const uint32_t *prev = p->year_ids + p->year_off[t - 1];
        const uint32_t *cur = p->year_ids + p->year_off[t];
        for (uint32_t l = 0; l < eng->np[t]; ++l)
            for (uint32_t k = 0; k < eng->np[t - 1]; ++k) {
                const uint32_t a = prev[k], b = cur[l];
                if (a >= p->nextid || b >= p->nextid)
                    return mdp_set_error(MDP_EINVAL, "short id out of range in year %u", t);
                const uint64_t key = ((uint64_t)a << 32) | b;
                auto it = pair_index.find(key);
                uint32_t pi;
                if (it == pair_index.end()) {
                    pi = (uint32_t)A0.size();
                    pair_index.emplace(key, pi);
                    A0.push_back(p->short_state[a]);
                    B0.push_back(p->short_state[b]);
                } else {
                    pi = it->second;
                }
                use0.push_back(pi);
                eng->maxA = std::max(eng->maxA, (uint32_t)__builtin_popcount(p->short_state[a]));
            }
    }
    // sort pairs by subset count (heaviest first), stable
    std::vector<uint32_t> order(A0.size());
    for (uint32_t i = 0; i < order.size(); ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        return __builtin_popcount(A0[x] & B0[x]) > __builtin_popcount(A0[y] & B0[y]);
    });
    std::vector<uint32_t> rank(order.size());
    uint32_t off = 0;
    for (uint32_t r = 0; r < order.size(); ++r) {
        const uint32_t i = order[r];
        rank[i] = r;
        eng->pairA.push_back(A0[i]);
        eng->pairB.push_back(B0[i]);
        eng->pairOff.push_back(off);
        off += (uint32_t)__builtin_popcount(A0[i] & B0[i]) + 1u;
    }
    for (uint32_t u : use0) eng->use_pair.push_back(rank[u]);
    // k_coefs subset parts (pair, first subset index), and per-use descriptors
    for (uint32_t pi = 0; pi < eng->pairA.size(); ++pi) {
        const uint32_t nX = (uint32_t)__builtin_popcount(eng->pairA[pi] & eng->pairB[pi]);
        eng->pairPart0.push_back((uint32_t)eng->partP.size());
        for (uint32_t k0 = 0; k0 < (1u << nX); k0 += kSubPart) {
            eng->partP.push_back(pi);
            eng->partK0.push_back(k0);
        }
    }
    eng->pairPart0.push_back((uint32_t)eng->partP.size());
    if (off > kOffMask) return mdp_set_error(MDP_EUNSUPPORTED, "too many transition coefficients");
    for (uint32_t pi : eng->use_pair) {
        const uint32_t A = eng->pairA[pi], B = eng->pairB[pi];
        const uint32_t nA = (uint32_t)__builtin_popcount(A), nX = (uint32_t)__builtin_popcount(A & B);
        eng->udesc.push_back(eng->pairOff[pi] | (nX << kOffBits) | (nA << 27));
    }
    eng->npairs = (uint32_t)eng->pairA.size();
    eng->nuses = (uint32_t)eng->use_pair.size();
    eng->ncoef = off;
    int rc = select_variant(eng, wide);
    if (rc) return rc;
    if (wide) return MDP_OK;  // no step program / k_coefs plan: build_wide_plan
    // step program
    for (uint32_t t = 1; t < p->tmax;) {
        if (eng->np[t - 1] == 1 && eng->np[t] == 1) {
            uint32_t cnt = 0;
            while (t < p->tmax && eng->np[t - 1] == 1 && eng->np[t] == 1) {
                ++cnt;
                ++t;
            }
            eng->prog.push_back(cnt << 1);
        } else {
            eng->prog.push_back(1u | (eng->np[t - 1] << 8) | (eng->np[t] << 16));
            ++t;
        }
    }
    eng->prog.push_back(0u);  // pad: the forward kernel reads one word ahead
    // k_coefs LDS plan: [Z/PV block] [part partials] [Q] [binomials]; the
    // partials spill to a global scratch when they do not fit
    const size_t zbytes = (size_t)(eng->nvar + 1) * eng->nstates * sizeof(double);
    const size_t pbytes = (size_t)eng->partP.size() * (eng->nvar + 1) * sizeof(double);
    const size_t qbytes = ((size_t)eng->ncoef + (size_t)(kMaxDeg + 1) * (kMaxDeg + 1)) * sizeof(double);
    if (zbytes + pbytes + qbytes <= kLdsBudget) {
        eng->lds_zpv = eng->lds_part = true;
        eng->coef_lds = zbytes + pbytes + qbytes;
    } else if (pbytes + qbytes <= kLdsBudget) {
        eng->lds_zpv = false;
        eng->lds_part = true;
        eng->coef_lds = pbytes + qbytes;
    } else if (qbytes <= kLdsBudget) {
        eng->lds_zpv = eng->lds_part = false;
        eng->coef_lds = qbytes;
    } else {
        return mdp_set_error(MDP_EUNSUPPORTED, "%u transition coefficients exceed the LDS budget",
                             eng->ncoef);
    }
    return MDP_OK;
}

// Direct-path plan.  Transitions that share X = A & B and the target state B
// share Q; each (X, B) group needs Pc[j][B] for every j <= X.  Items are the
// distinct (j, B), numbered by j ascending then B ascending; qstart / qitem
// list, for every Q entry (group, m), its items with |j| = m in ascending j.
int build_direct_plan(MdpEnginePlan *eng, const mdp_problem *p)
{
    std::map<uint64_t, uint32_t> group;  // (X, B) -> Q offset
    std::vector<std::pair<uint32_t, uint32_t>> groups;
    std::vector<uint32_t> pair_group(eng->pairA.size());
    uint32_t off = 0;
    std::vector<uint32_t> goff;
    for (size_t pi = 0; pi < eng->pairA.size(); ++pi) {
        const uint32_t B = eng->pairB[pi], X = eng->pairA[pi] & B;
        const uint64_t key = ((uint64_t)X << 32) | B;
        auto it = group.find(key);
        if (it == group.end()) {
            it = group.emplace(key, (uint32_t)groups.size()).first;
            groups.push_back({X, B});
            // even start: the forward kernels read a group's coefficients
            // pairwise as 16-byte aligned ds_read_b128 (an unaligned pair
            // becomes a ds_read2_b64, twice the LDS cycles per byte)
            off = (off + 1u) & ~1u;
            goff.push_back(off);
            off += (uint32_t)__builtin_popcount(X) + 1u;
        }
        pair_group[pi] = it->second;
    }
    if (off > kOffMask) return mdp_set_error(MDP_EUNSUPPORTED, "too many transition coefficients");
    eng->ncoef_d = off;
    std::map<uint32_t, std::vector<uint32_t>> jb;  // j -> states B (sorted, unique)
    auto for_subsets = [](uint32_t X, auto &&fn) {  // ascending j <= X
        const uint32_t nX = (uint32_t)__builtin_popcount(X);
        for (uint32_t k = 0; k < (1u << nX); ++k) {
            uint32_t j = 0, xs = X;
            for (uint32_t i = 0; i < nX; ++i) {
                const uint32_t low = xs & (0u - xs);
                if ((k >> i) & 1u) j |= low;
                xs ^= low;
            }
            fn(j);
        }
    };
    for (auto &g : groups) for_subsets(g.first, [&](uint32_t j) { jb[j].push_back(g.second); });
    std::map<uint64_t, uint32_t> item;  // (j, B) -> item
    eng->cj_bits.clear();
    eng->cj_item0.clear();
    eng->itemB.clear();
    for (auto &kv : jb) {
        auto &v = kv.second;
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        eng->cj_bits.push_back(kv.first);
        eng->cj_item0.push_back((uint32_t)eng->itemB.size());
        for (uint32_t B : v) {
            item.emplace(((uint64_t)kv.first << 32) | B, (uint32_t)eng->itemB.size());
            eng->itemB.push_back(B);
        }
    }
    eng->cj_item0.push_back((uint32_t)eng->itemB.size());
    eng->nj = (uint32_t)eng->cj_bits.size();
    if (eng->nj > 0xffffu) return mdp_set_error(MDP_EUNSUPPORTED, "%u hidden-state rows (direct path max 65535)", eng->nj);
    eng->itemRow.assign(eng->itemB.size(), 0u);
    for (uint32_t js = 0; js < eng->nj; ++js)
        for (uint32_t i = eng->cj_item0[js]; i < eng->cj_item0[js + 1]; ++i) eng->itemRow[i] = js;
    eng->nitems = (uint32_t)eng->itemB.size();
    eng->ldP = ((size_t)eng->nitems + 1) & ~(size_t)1;
    eng->qstart.assign(1, 0u);
    eng->qitem.clear();
    for (auto &g : groups) {
        const uint32_t nX = (uint32_t)__builtin_popcount(g.first);
        if ((eng->qstart.size() - 1) & 1u) eng->qstart.push_back((uint32_t)eng->qitem.size());  // pad slot
        for (uint32_t m = 0; m <= nX; ++m) {
            for_subsets(g.first, [&](uint32_t j) {
                if ((uint32_t)__builtin_popcount(j) == m)
                    eng->qitem.push_back(item.at(((uint64_t)j << 32) | g.second));
            });
            eng->qstart.push_back((uint32_t)eng->qitem.size());
        }
    }
    // k_qrows' phase-3 lane table (the canonical Q-sum order, kQGroup): per
    // entry q < ldQ an aligned segment of L = min(P, kQLanesMax) lanes, P =
    // its group count rounded up to a power of two, each lane 2^G = P / L
    // groups; segments packed largest first, so each is aligned and lies in
    // one wave; padded to whole waves
    {
        const size_t ldq = ((size_t)off + 1) & ~(size_t)1;
        struct Ent { uint32_t lgL, lgG, q; };
        std::vector<Ent> ents;
        for (uint32_t q = 0; q < ldq; ++q) {
            const uint32_t n = q + 1 < eng->qstart.size() ? eng->qstart[q + 1] - eng->qstart[q] : 0u;
            const uint32_t ng = std::max<uint32_t>(1u, (n + kQGroup - 1) / kQGroup);
            uint32_t lgP = 0;
            while ((1u << lgP) < ng) ++lgP;
            uint32_t lgL = 0;
            while ((1u << lgL) < kQLanesMax && lgL < lgP) ++lgL;
            if (lgP - lgL >= (uint32_t)kQLevelsRows)
                return mdp_set_error(MDP_EUNSUPPORTED, "a Q entry of %u items (k_qrows' lane table)", n);
            ents.push_back({lgL, lgP - lgL, q});
        }
        std::stable_sort(ents.begin(), ents.end(), [](const Ent &x, const Ent &y) { return x.lgL > y.lgL; });
        eng->qslot.clear();
        eng->qslot_lglmax = ents.empty() ? 0u : ents[0].lgL;
        for (const Ent &en : ents)
            for (uint32_t le = 0; le < (1u << en.lgL); ++le)
                eng->qslot.push_back(make_uint2(en.q, le | (en.lgL << 8) | (en.lgG << 12)));
        while (eng->qslot.size() % 64) eng->qslot.push_back(make_uint2(0xffffffffu, 0u));
        // nvar <= 8 (one group per lane): each lane's kQGroup items, nitems
        // past its entry; at least 64 lanes
        const uint32_t ni = eng->nitems;
        eng->qlane.assign(std::max<size_t>(eng->qslot.size(), 64) * kQGroup, ni);
        if (eng->nvar <= 8)
            for (size_t sl = 0; sl < eng->qslot.size(); ++sl) {
                const uint32_t q = eng->qslot[sl].x, le = eng->qslot[sl].y & 0xffu;
                if ((size_t)q + 1 >= eng->qstart.size()) continue;  // padding lanes: q = ~0
                const uint32_t j0 = eng->qstart[q] + le * kQGroup, i1 = eng->qstart[q + 1];
                for (uint32_t u = 0; u < kQGroup && j0 + u < i1; ++u) eng->qlane[sl * kQGroup + u] = eng->qitem[j0 + u];
            }
        // Pc slots (16 bytes per slot and c pair in LDS).  Phase 3 gathers
        // item u of every lane in one ds_read_b128, serviced in four 16-lane
        // groups, conflict-free when a group's slots differ mod 16; phase 2
        // stores eight consecutive items per 8-lane group of a
        // ds_write_b128, conflict-free when they differ mod 8.  The items are
        // coloured (colour = slot mod 16) greedily under both rules, the
        // least-used allowed colour first; slots 0-15 hold zeros, and each
        // group's padding takes the zero slot of a colour none of its items
        // has.  nvar > 8 (CSR path): slot = item + 16.
        eng->islot.resize(ni);
        for (uint32_t it = 0; it < ni; ++it) eng->islot[it] = it + 16;
        eng->npl_slots = ni + 16;
        if (eng->nvar <= 8) {
            auto lgroup = [](uint32_t l) -> uint32_t {  // ds_read_b128 lane groups
                const uint32_t h = l & 31u;
                const uint32_t g = (h < 4 || (h >= 12 && h < 16) || (h >= 20 && h < 28)) ? 0u : 1u;
                return g + (l >= 32 ? 2u : 0u);
            };
            const size_t nl = eng->qslot.size();
            std::vector<std::vector<uint32_t>> grp;  // per (wave, u, lane group): its items
            for (size_t w0 = 0; w0 < nl; w0 += 64)
                for (uint32_t u = 0; u < kQGroup; ++u) {
                    std::vector<uint32_t> g4[4];
                    for (uint32_t l = 0; l < 64 && w0 + l < nl; ++l) {
                        const uint32_t it = eng->qlane[(w0 + l) * kQGroup + u];
                        if (it < ni) g4[lgroup(l)].push_back(it);
                    }
                    for (auto &g : g4) {
                        std::sort(g.begin(), g.end());
                        g.erase(std::unique(g.begin(), g.end()), g.end());
                        grp.push_back(std::move(g));
                    }
                }
            std::vector<std::vector<uint32_t>> ig(ni);
            for (uint32_t gi = 0; gi < grp.size(); ++gi)
                for (uint32_t it : grp[gi]) ig[it].push_back(gi);
            std::vector<int> col(ni, -1);
            uint32_t cnt[16] = {};
            for (uint32_t it = 0; it < ni; ++it) {
                uint32_t forb = 0;
                for (uint32_t gi : ig[it])
                    for (uint32_t o : grp[gi])
                        if (col[o] >= 0) forb |= 1u << col[o];
                for (uint32_t o = it & ~7u; o < (it | 7u) + 1 && o < ni; ++o)  // phase 2's store group
                    if (o != it && col[o] >= 0) forb |= 0x101u << (col[o] & 7);
                int best = -1;
                for (int pass = 0; pass < 2 && best < 0; ++pass)
                    for (int cc = 0; cc < 16; ++cc)
                        if ((pass || !((forb >> cc) & 1u)) && (best < 0 || cnt[cc] < cnt[best])) best = cc;
                col[it] = best;
                ++cnt[best];
            }
            // min-conflicts repair: move an item to the colour its groups use
            // least while that lowers its own conflicts (each move lowers the
            // total, which is symmetric in the pairs), a few sweeps.  A gather
            // conflict costs a cycle per group; a store conflict only about a
            // quarter of one (a ds_write_b128's transfer, 13 cycles, hides all
            // but 3 of the 16 array cycles of a 2-way conflict): weights 4 : 1
            for (int sweep = 0; sweep < 16; ++sweep) {
                bool moved = false;
                for (uint32_t it = 0; it < ni; ++it) {
                    uint32_t cost[16] = {};
                    for (uint32_t gi : ig[it])
                        for (uint32_t o : grp[gi])
                            if (o != it) cost[col[o]] += 4;
                    for (uint32_t o = it & ~7u; o < (it | 7u) + 1 && o < ni; ++o)
                        if (o != it) {
                            ++cost[col[o] & 7];
                            ++cost[(col[o] & 7) + 8];
                        }
                    int best = col[it];
                    for (int cc = 0; cc < 16; ++cc)
                        if (cost[cc] < cost[best] || (cost[cc] == cost[best] && cnt[cc] + 1 < cnt[best])) best = cc;
                    if (best != col[it]) {
                        --cnt[col[it]];
                        ++cnt[best];
                        col[it] = best;
                        moved = true;
                    }
                }
                if (!moved) break;
            }
            uint32_t next[16];
            for (uint32_t cc = 0; cc < 16; ++cc) next[cc] = 16 + cc;
            uint32_t top = 16;
            for (uint32_t it = 0; it < ni; ++it) {
                eng->islot[it] = next[col[it]];
                next[col[it]] += 16;
                top = std::max(top, eng->islot[it] + 1);
            }
            eng->npl_slots = top;
            // what the colouring leaves: per phase-3 group the extra cycles of
            // its busiest residue, per phase-2 store group those mod 8
            uint32_t extra = 0, sextra = 0;
            for (const auto &g : grp) {
                uint32_t m[16] = {};
                for (uint32_t it : g) ++m[eng->islot[it] & 15u];
                extra += *std::max_element(m, m + 16) - (g.empty() ? 0u : 1u);
            }
            for (uint32_t g0 = 0; g0 < ni; g0 += 8) {
                uint32_t m[8] = {};
                for (uint32_t it = g0; it < std::min(ni, g0 + 8); ++it) ++m[eng->islot[it] & 7u];
                sextra += *std::max_element(m, m + 8) - 1u;
            }
            eng->slot_conflicts = extra;
            eng->slot_store_conflicts = sextra;
            // the lanes' slots; each (wave, u, lane group)'s padding on a free colour
            for (size_t w0 = 0; w0 < std::max<size_t>(nl, 64); w0 += 64)
                for (uint32_t u = 0; u < kQGroup; ++u) {
                    uint32_t used[4] = {};
                    for (uint32_t l = 0; l < 64; ++l) {
                        const uint32_t it = eng->qlane[(w0 + l) * kQGroup + u];
                        if (it < ni) used[lgroup(l)] |= 1u << (eng->islot[it] & 15u);
                    }
                    for (uint32_t l = 0; l < 64; ++l) {
                        uint32_t &x = eng->qlane[(w0 + l) * kQGroup + u];
                        if (x < ni) {
                            x = eng->islot[x];
                        } else {
                            const uint32_t fr = ~used[lgroup(l)] & 0xffffu;
                            x = fr ? (uint32_t)__builtin_ctz(fr) : 0u;
                        }
                    }
                }
        }
    }
    eng->udesc_d.clear();
    for (uint32_t pi : eng->use_pair) {
        const uint32_t A = eng->pairA[pi], B = eng->pairB[pi];
        const uint32_t nA = (uint32_t)__builtin_popcount(A), nX = (uint32_t)__builtin_popcount(A & B);
        eng->udesc_d.push_back(goff[pair_group[pi]] | (nX << kOffBits) | (nA << 27));
    }
    // colonisation sums S[j][k] = sum over var columns l in j (ascending),
    // l != k, of M[l][k] -- the reference's per-point sum (:350-357) with its
    // zero terms dropped, in its order
    const uint32_t n = p->n, nvar = p->nvar;
    eng->var_cols.assign(p->var_cols, p->var_cols + nvar);
    eng->isvar.assign(n, 0);
    for (uint32_t b = 0; b < nvar; ++b) eng->isvar[p->var_cols[b]] = 1;
    eng->Sj.assign((size_t)eng->nj * n, 0.0);
    for (uint32_t js = 0; js < eng->nj; ++js) {
        const uint32_t j = eng->cj_bits[js];
        for (uint32_t k = 0; k < n; ++k) {
            double acc = 0.0;
            for (uint32_t b = 0; b < nvar; ++b) {
                const uint32_t col = p->var_cols[b];
                if (((j >> (nvar - 1 - b)) & 1u) && col != k) acc += p->M[(size_t)col * n + k];
            }
            eng->Sj[(size_t)js * n + k] = acc;
        }
    }
    return MDP_OK;
}

// per (year, wave) work items over a year's column tiles of nch[tile]
// pipeline chunks each (k_fwd_mmt, k_fwd_hs): more than 16 tiles are dealt
// longest list first to the least-loaded wave (up to tmaxit each); up to 16
// give every tile a wave and the spare waves to the tiles whose slices are
// longest (at least two chunks each; slices past the first `inplace` of a
// tile park their partials, `room` 16-row blocks at most)
void plan_waves(const std::vector<uint32_t> &nch, uint32_t tmaxit, uint32_t inplace, uint32_t room, uint2 *wp,
                uint32_t nw = 16)
{
    const uint32_t ncol = (uint32_t)nch.size();
    if (ncol <= nw) {
        // waves per tile: one each, the rest to the tile whose slices
        // are longest (each slice at least two chunks; the parked
        // partials -- every slice past the first `inplace` of a tile --
        // within the buffer's rows past the year's tiles)
        std::vector<uint32_t> w(ncol, 1);
        uint32_t parked = 0;
        for (uint32_t spare = nw - ncol; spare; --spare) {
            uint32_t best = ncol;
            for (uint32_t i = 0; i < ncol; ++i)
                if (nch[i] / (w[i] + 1) >= 2 && (w[i] + 1 <= inplace || parked < room) &&
                    (best == ncol || nch[i] * w[best] > nch[best] * w[i]))
                    best = i;
            if (best == ncol) break;
            if (++w[best] > inplace) ++parked;
        }
        const uint32_t split = *std::max_element(w.begin(), w.end()) > 1 ? 1u : 0u;
        for (uint32_t wv = 0; wv < nw; ++wv)
            for (uint32_t i = 0; i < tmaxit; ++i) wp[wv * tmaxit + i] = make_uint2(0u, split << 22);
        uint32_t wv = 0, pbase = 0;
        for (uint32_t tile = 0; tile < ncol; ++tile) {
            for (uint32_t ks = 0; ks < w[tile]; ++ks, ++wv) {
                const uint32_t cb = nch[tile] * ks / w[tile], ce = nch[tile] * (ks + 1) / w[tile];
                wp[wv * tmaxit] = make_uint2(cb | ce << 16, tile | ks << 8 | w[tile] << 12 | pbase << 17 |
                                                               split << 22 | 1u << 24);
            }
            pbase += w[tile] > inplace ? w[tile] - inplace : 0;
        }
    } else {
        std::vector<uint32_t> order(ncol), cnt(nw, 0);
        std::vector<uint64_t> load(nw, 0);
        for (uint32_t i = 0; i < ncol; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return nch[x] > nch[y]; });
        for (uint32_t wv = 0; wv < nw; ++wv)
            for (uint32_t i = 0; i < tmaxit; ++i) wp[wv * tmaxit + i] = make_uint2(0u, 0u);
        for (uint32_t tile : order) {
            uint32_t best = nw;
            for (uint32_t wv = 0; wv < nw; ++wv)
                if (cnt[wv] < tmaxit && (best == nw || load[wv] < load[best])) best = wv;
            wp[best * tmaxit + cnt[best]++] = make_uint2(nch[tile] << 16, tile | 1u << 12 | 1u << 24);
            load[best] += nch[tile];
        }
    }
}

// k_fwd_mmt's tables (c-independent): years of at most 1 024 states.
//  * per (year, column tile) its K entries: every source k with m = 0 ..
//    the largest nX over the tile's new states (the rest of m <= |A_k| would
//    meet only zero slots), padded to whole pipeline chunks; and per K entry
//    and new state l of the tile, the byte offset in the Q row of Q_kl[m]
//    (the zero slot where m > nX_kl, for padded states and padded entries)
//    -- 64 bytes per entry, so the kernel's gathers need no lookup;
//  * per (year, wave) up to ROWS / 256 work items: tiles of years of more
//    than 16 tiles dealt longest list first to the least-loaded wave;
//    smaller years give every tile a wave and the spare waves to the tiles
//    with the longest lists, each tile's list split into as many slices
//    (at least two chunks each).
// False: the problem is not k_fwd_mmt's.
bool build_mmt_plan(MdpEnginePlan *eng)
{
    if (eng->npmax > 1024 || eng->maxA > 24 || eng->tmax < 2) return false;
    const MmtShape shp = mmt_shape(eng);
    const uint32_t rows = shp.rows, rt = shp.rt, pts = mmt_pts(rt), ps = mmt_ps(rt);
    const uint32_t tmaxit = rows > 256 ? rows / 256 : 1, cw = 4 * mmt_u(rt), inplace = shp.db ? 2u : 1u;
    const uint32_t none = (uint32_t)eng->ncoef_d;
    if (none > kOffMask) return false;
    eng->mmt_rt = rt;
    eng->mmt_rows = rows;
    eng->mmt_kt.clear();
    eng->mmt_cidx.clear();
    eng->mmt_ktile.assign((size_t)(eng->tmax + 1) * kMmtMaxTiles, make_uint2(0u, 1u));
    eng->mmt_wplan.assign((size_t)(eng->tmax + 1) * 16 * tmaxit, make_uint2(0u, 0u));
    double fl = 0.0;
    size_t ub = 0;
    for (uint32_t t = 1; t < eng->tmax; ++t) {
        const uint32_t npp = eng->np[t - 1], npc = eng->np[t], ncol = (npc + 15) / 16;
        const uint32_t *ud = eng->udesc_d.data() + ub;  // ud[l * npp + k]
        std::vector<uint32_t> nch(ncol);
        for (uint32_t tile = 0; tile < ncol; ++tile) {
            const size_t start = eng->mmt_kt.size();
            const uint32_t l1 = std::min(16 * tile + 16, npc);
            for (uint32_t k = 0; k < npp; ++k) {
                const uint32_t a = ud[k] >> 27;  // |A_k|
                uint32_t mx = 0;
                for (uint32_t l = 16 * tile; l < l1; ++l) mx = std::max(mx, (ud[(size_t)l * npp + k] >> kOffBits) & 31u);
                for (uint32_t m = 0; m <= mx; ++m) {  // V row k, y^m row, x^(a-m) row (bytes); m; k
                    eng->mmt_kt.push_back(make_uint2((k * pts * 8u) | ((m * ps * 8u) << 18),
                                                     ((a - m) * ps * 8u) | (m << 16) | (k << 21)));
                    for (uint32_t l = 16 * tile; l < 16 * tile + 16; ++l) {
                        uint32_t o = none;
                        if (l < npc) {
                            const uint32_t dsc = ud[(size_t)l * npp + k];
                            if (m <= ((dsc >> kOffBits) & 31u)) o = (dsc & kOffMask) + m;
                        }
                        eng->mmt_cidx.push_back(o * 8u);
                    }
                }
            }
            while ((eng->mmt_kt.size() - start) % cw) {
                eng->mmt_kt.push_back(make_uint2(0u, npp << 21));
                for (uint32_t l = 0; l < 16; ++l) eng->mmt_cidx.push_back(none * 8u);
            }
            nch[tile] = (uint32_t)((eng->mmt_kt.size() - start) / cw);
            eng->mmt_ktile[(size_t)t * kMmtMaxTiles + tile] = make_uint2((uint32_t)start, nch[tile]);
            fl += 2.0 * 16.0 * (double)(eng->mmt_kt.size() - start);
        }
        plan_waves(nch, tmaxit, inplace, (rows - ncol * 16) / 16, eng->mmt_wplan.data() + (size_t)t * 16 * tmaxit);
        ub += (size_t)npp * npc;
    }
    eng->mmt_flops_pt = fl + 2.0 * (eng->maxA + 1) + (double)eng->np[eng->tmax - 1];
    // (the offsets' table is the plan's largest: 64 bytes per K entry)
    const bool ok = mmt_lds(eng) <= eng->lds_max && eng->mmt_kt.size() < (1u << 26) && (size_t)none * 8u < 0xffffffffu;
    if (!ok) {
        eng->mmt_kt.clear();
        eng->mmt_cidx.clear();
    }
    return ok;
}

// k_fwd_hs's tables (c-independent; nvar <= 10, years of at most 1 024
// states).  Per year t >= 1:
//  * butterfly passes over W = the bits of year t - 1's states, up to
//    kHsRadix patches a pass: first the patches set in no hidden state the
//    year's products read, then greedily the one adding the fewest new cube
//    positions; a pass lists its cosets (g, the masks of the positions it
//    reads and writes: only those whose value still reaches a hidden state
//    the products read).  After the passes every such j holds U[j];
//  * the year's states ordered by (B & W, B), so a tile's 16 states share
//    their reachable hidden states; per tile K = the j in that down-closure
//    below some state of the tile, ascending, padded to whole pipeline
//    chunks (row 0, C = 0), and per (K entry, state) the byte offset of the
//    item Pc[j][B] in the column's Pg row (its zero slot, nitems, for j not
//    below B, padded states and padded entries);
//  * the states' cube positions in tile order (~0: padding), the free 16-row
//    park blocks (no state of the year in them), the wave plan.
// Year 0's positions head dpos.  Refused (false: k_fwd_mmt runs) for a
// year with a repeated state or an item the direct plan lacks.
bool build_hs_plan(MdpEnginePlan *eng)
{
    if (eng->nvar > 10 || eng->tmax < 2 || eng->npmax > 1024 || eng->ystate.size() < eng->tmax) return false;
    const uint32_t nb = std::max<uint32_t>(8u, eng->nvar);
    // waves a block (MDP_HS_WAVES): 8 for 8 variable patches (32 points, a
    // 64 KiB cube: two blocks a CU, whose phases overlap; measured 5 % faster
    // on the 256-state series, equal on the 128-state one, profiles/r06/hs),
    // else 16
    uint32_t nw = nb == 8 ? 8u : 16u;
    if (eng->opts.hs_waves) nw = *eng->opts.hs_waves == 8 && nb == 8 ? 8u : 16u;
    const uint32_t rt = nb == 8 ? (nw == 8 ? 2u : 4u) : nb == 9 ? 2u : 1u, pts = mmt_pts(rt);
    const uint32_t ncube = 1u << nb, tmaxit = ncube / 16 > nw ? ncube / 16 / nw : 1u, cw = 4 * mmt_u(rt);
    const uint32_t zero = eng->nitems;  // the Pg row's zero slot
    if ((uint64_t)zero * 8u >= 0xffffffffull) return false;
    // patches per v Pe pass (MDP_HS_RADIX, 1 .. kHsRadix; default 4, the
    // measured best: profiles/r06/hs -- 1 024 cosets x points fill the block
    // in one sweep; 5 left half the threads idle on 1 024-state years)
    const uint32_t radix = eng->opts.hs_radix.value_or(kHsRadix);
    std::unordered_map<uint64_t, uint32_t> item;  // (j, B) -> item
    for (uint32_t js = 0; js < eng->nj; ++js)
        for (uint32_t i = eng->cj_item0[js]; i < eng->cj_item0[js + 1]; ++i)
            item.emplace(((uint64_t)eng->cj_bits[js] << 32) | eng->itemB[i], i);
    std::vector<uint32_t> yoff(eng->tmax + 1, 0);
    for (uint32_t t = 0; t < eng->tmax; ++t) yoff[t + 1] = yoff[t] + eng->np[t];
    auto st = [&](uint32_t t, uint32_t l) { return eng->ystate[yoff[t] + l]; };
    eng->hs_kt.clear();
    eng->hs_cidx.clear();
    eng->hs_pass.clear();
    eng->hs_ppos.clear();
    eng->hs_dpos.clear();
    std::vector<uint2> ktile(kMmtMaxTiles), wtmp(nw * tmaxit);
    eng->hs_wplan.assign((size_t)(eng->tmax + 1) * nw * tmaxit, make_uint4(0u, 0u, 0u, 1u));
    eng->hs_pk.assign((size_t)(eng->tmax + 1) * 16, 0u);
    eng->hs_pbase.assign(eng->tmax + 1, 0u);
    eng->hs_dbase.assign(eng->tmax + 1, 0u);
    std::vector<uint8_t> seen(ncube, 0);
    auto distinct = [&](uint32_t t) {
        bool ok = true;
        for (uint32_t l = 0; l < eng->np[t]; ++l) {
            const uint32_t b = st(t, l);
            if (b >= ncube || seen[b]) ok = false;
            else seen[b] = 1;
        }
        for (uint32_t l = 0; l < eng->np[t]; ++l)
            if (st(t, l) < ncube) seen[st(t, l)] = 0;
        return ok;
    };
    if (!distinct(0)) return false;
    for (uint32_t l = 0; l < (eng->np[0] + 15) / 16 * 16; ++l) eng->hs_dpos.push_back(l < eng->np[0] ? st(0, l) : ~0u);
    double fb = 0.0, fm = 0.0;
    std::vector<uint8_t> live(ncube);
    std::vector<uint32_t> lv;
    for (uint32_t t = 1; t < eng->tmax; ++t) {
        const uint32_t npp = eng->np[t - 1], npc = eng->np[t], ncol = (npc + 15) / 16;
        if (!distinct(t)) return false;
        // butterfly passes
        std::fill(live.begin(), live.end(), 0);
        lv.clear();
        uint32_t W = 0;
        for (uint32_t k = 0; k < npp; ++k) {
            W |= st(t - 1, k);
            live[st(t - 1, k)] = 1;
            lv.push_back(st(t - 1, k));
        }
        // D: the hidden states below some state of year t - 1 (U's
        // support); N: those below some state of year t (U's reads, the
        // union of the year's K lists); M(rem): the positions whose value
        // still reaches N by the butterflies over the patches rem (N's
        // up-closure over rem) -- a pass reads live positions in M(before)
        // and writes positions in M(after) only
        std::vector<uint8_t> Dm(ncube, 0), Nm(ncube, 0), Mb(ncube), Ma(ncube);
        for (uint32_t k = 0; k < npp; ++k) Dm[st(t - 1, k)] = 1;
        for (uint32_t bit = 1; bit < ncube; bit <<= 1)
            for (uint32_t q = 0; q < ncube; ++q)
                if ((q & bit) && Dm[q]) Dm[q ^ bit] = 1;
        uint32_t nused = 0;  // patches set in some j of N
        for (uint32_t l = 0; l < npc; ++l) {
            const uint32_t key = st(t, l) & W;
            for (uint32_t j = key;; j = (j - 1) & key) {
                if (Dm[j] && !Nm[j]) {
                    Nm[j] = 1;
                    nused |= j;
                }
                if (!j) break;
            }
        }
        auto upclose = [&](uint32_t rem, std::vector<uint8_t> &M) {
            M = Nm;
            for (uint32_t bit = 1; bit < ncube; bit <<= 1)
                if (rem & bit)
                    for (uint32_t q = 0; q < ncube; ++q)
                        if (!(q & bit) && M[q]) M[q | bit] = 1;
        };
        // the patches of W: first those set in no j of N (each halves what
        // later passes touch), then greedily the one adding the fewest new
        // positions (ties: fewest values to move)
        std::vector<uint32_t> border;
        {
            std::vector<uint8_t> lt(live);
            std::vector<uint32_t> l2(lv);
            for (int phase = 0; phase < 2; ++phase)
                for (uint32_t rem = W & (phase ? nused : ~nused); rem;) {
                    uint32_t best = 0, bnew = ~0u, bpairs = ~0u;
                    for (uint32_t rr = rem; rr; rr &= rr - 1) {
                        const uint32_t bit = rr & (0u - rr);
                        uint32_t nw = 0, pr = 0;
                        for (uint32_t a : l2)
                            if (a & bit) {
                                ++pr;
                                nw += !lt[a ^ bit];
                            }
                        if (nw < bnew || (nw == bnew && pr < bpairs)) {
                            best = bit;
                            bnew = nw;
                            bpairs = pr;
                        }
                    }
                    rem &= ~best;
                    border.push_back((uint32_t)__builtin_ctz(best));
                    const size_t n2 = l2.size();
                    for (size_t i = 0; i < n2; ++i)
                        if ((l2[i] & best) && !lt[l2[i] ^ best]) {
                            lt[l2[i] ^ best] = 1;
                            l2.push_back(l2[i] ^ best);
                        }
                }
        }
        eng->hs_pbase[t] = (uint32_t)eng->hs_pass.size();
        const size_t npass = (border.size() + radix - 1) / radix;
        uint32_t remw = W;
        for (size_t ip = 0, b0 = 0; ip < npass; ++ip) {
            // passes of near-equal size (radix 4: 10 patches 4 + 3 + 3)
            const uint32_t r = (uint32_t)((border.size() - b0 + (npass - ip) - 1) / (npass - ip));
            uint32_t bp[kHsRadix] = {}, mask = 0, bits = 0;
            for (uint32_t k = 0; k < r; ++k) {
                bp[k] = border[b0 + k];
                mask |= 1u << bp[k];
                bits |= bp[k] << (5 * k);
            }
            b0 += r;
            upclose(remw, Mb);
            remw &= ~mask;
            upclose(remw, Ma);
            auto dep = [&](uint32_t q) {
                uint32_t o = 0;
                for (uint32_t k = 0; k < r; ++k)
                    if (q & (1u << k)) o |= 1u << bp[k];
                return o;
            };
            std::map<uint32_t, uint32_t> cos;  // g -> mask of positions read
            for (uint32_t a : lv) {
                if (!Mb[a]) continue;
                uint32_t q = 0;
                for (uint32_t k = 0; k < r; ++k)
                    if (a & (1u << bp[k])) q |= 1u << k;
                cos[a & ~mask] |= 1u << q;
            }
            const uint32_t base = (uint32_t)eng->hs_ppos.size();
            std::map<uint32_t, std::vector<uint32_t>> bymask;  // read | write << 16 -> its cosets
            for (auto &kv : cos) {
                uint32_t cl = kv.second;  // the read positions' subsets
                cl |= (cl & 0xaaaau) >> 1;
                cl |= (cl & 0xccccu) >> 2;
                cl |= (cl & 0xf0f0u) >> 4;
                cl |= (cl & 0xff00u) >> 8;
                uint32_t outm = 0;
                for (uint32_t q = 0; q < (1u << r); ++q)
                    if (((cl >> q) & 1u) && Ma[kv.first | dep(q)]) outm |= 1u << q;
                bymask[kv.second | outm << 16].push_back(kv.first);
            }
            // cosets grouped by masks, pts / 64 ... a wave's worth at a time
            // (64 / pts cosets a wave), each wave padded with copies of its
            // first coset (a lane of the same wave: identical values)
            const uint32_t cpw = 64u / pts;
            for (auto &mv : bymask)
                for (size_t i = 0; i < mv.second.size(); i += cpw)
                    for (uint32_t k = 0; k < cpw; ++k)
                        eng->hs_ppos.push_back(make_uint2(i + k < mv.second.size() ? mv.second[i + k] : mv.second[i],
                                                          mv.first));
            for (auto &kv : cos) {
                uint32_t cl = kv.second;
                cl |= (cl & 0xaaaau) >> 1;
                cl |= (cl & 0xccccu) >> 2;
                cl |= (cl & 0xf0f0u) >> 4;
                cl |= (cl & 0xff00u) >> 8;
                uint32_t outm = 0;
                for (uint32_t q = 0; q < (1u << r); ++q)
                    if (((cl >> q) & 1u) && Ma[kv.first | dep(q)]) outm |= 1u << q;
                fb += 2.0 * (double)r * (double)(1u << (r - 1)) + (ip + 1 == npass ? (double)(1u << r) : 0.0);
                for (uint32_t q = 0; q < (1u << r); ++q)
                    if (((outm >> q) & 1u) && !live[kv.first | dep(q)]) {
                        live[kv.first | dep(q)] = 1;
                        lv.push_back(kv.first | dep(q));
                    }
            }
            eng->hs_pass.push_back(make_uint4(bits, r, (uint32_t)eng->hs_ppos.size() - base, base));
        }
        // the year's states in tile order
        std::vector<uint32_t> ord(npc);
        for (uint32_t l = 0; l < npc; ++l) ord[l] = l;
        std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) {
            const uint32_t bx = st(t, x), by = st(t, y);
            return (bx & W) != (by & W) ? (bx & W) < (by & W) : bx < by;
        });
        eng->hs_dbase[t] = (uint32_t)eng->hs_dpos.size();
        for (uint32_t i = 0; i < ncol * 16; ++i) eng->hs_dpos.push_back(i < npc ? st(t, ord[i]) : ~0u);
        std::vector<uint32_t> nch(ncol);
        std::vector<uint32_t> K;
        for (uint32_t tile = 0; tile < ncol; ++tile) {
            K.clear();
            for (uint32_t i = 16 * tile; i < std::min(16 * tile + 16, npc); ++i) {
                const uint32_t key = st(t, ord[i]) & W;
                for (uint32_t j = key;; j = (j - 1) & key) {  // subsets of key (with j = 0 last)
                    if (Dm[j]) K.push_back(j);
                    if (!j) break;
                }
            }
            std::sort(K.begin(), K.end());
            K.erase(std::unique(K.begin(), K.end()), K.end());
            const size_t start = eng->hs_kt.size();
            for (uint32_t j : K) {
                eng->hs_kt.push_back(j * pts * 8u);
                for (uint32_t i = 16 * tile; i < 16 * tile + 16; ++i) {
                    uint32_t o = zero;
                    if (i < npc && !(j & ~st(t, ord[i]))) {
                        auto it = item.find(((uint64_t)j << 32) | st(t, ord[i]));
                        if (it == item.end()) return false;
                        o = it->second;
                    }
                    eng->hs_cidx.push_back(o * 8u);
                }
            }
            while ((eng->hs_kt.size() - start) % cw) {
                eng->hs_kt.push_back(0u);
                for (uint32_t l = 0; l < 16; ++l) eng->hs_cidx.push_back(zero * 8u);
            }
            nch[tile] = (uint32_t)((eng->hs_kt.size() - start) / cw);
            ktile[tile] = make_uint2((uint32_t)start, nch[tile]);
            fm += 2.0 * 16.0 * (double)(eng->hs_kt.size() - start);
        }
        // free park blocks
        std::vector<uint8_t> used(ncube / 16, 0);
        for (uint32_t l = 0; l < npc; ++l) used[st(t, l) / 16] = 1;
        uint32_t room = 0;
        for (uint32_t b = 0; b < ncube / 16 && room < 16; ++b)
            if (!used[b]) eng->hs_pk[(size_t)t * 16 + room++] = b * 16;
        plan_waves(nch, tmaxit, 1u, room, wtmp.data(), nw);
        for (uint32_t i = 0; i < nw * tmaxit; ++i) {
            const uint2 kt2 = ktile[wtmp[i].y & 0xffu];
            eng->hs_wplan[(size_t)t * nw * tmaxit + i] =
                (wtmp[i].y >> 24) ? make_uint4(wtmp[i].x, wtmp[i].y, kt2.x, kt2.y) : make_uint4(wtmp[i].x, wtmp[i].y, 0u, 1u);
        }
    }
    eng->hs_pbase[eng->tmax] = (uint32_t)eng->hs_pass.size();
    // the store positions per (16 positions of dpos, lane group kk): entries
    // kk + 4 r, r = 0 .. 3, 16 bits each (0xffff: padding)
    eng->hs_dpk.assign(eng->hs_dpos.size() / 16 * 4, make_uint2(0u, 0u));
    for (size_t b = 0; b < eng->hs_dpos.size() / 16; ++b)
        for (uint32_t kq = 0; kq < 4; ++kq) {
            uint32_t w[4];
            for (uint32_t r = 0; r < 4; ++r) {
                const uint32_t ps = eng->hs_dpos[b * 16 + kq + 4 * r];
                w[r] = ps == ~0u ? 0xffffu : ps;
            }
            eng->hs_dpk[b * 4 + kq] = make_uint2(w[0] | w[1] << 16, w[2] | w[3] << 16);
        }
    if (eng->hs_kt.empty()) eng->hs_kt.push_back(0u);
    if (eng->hs_ppos.empty()) eng->hs_ppos.push_back(make_uint2(0u, 0u));
    if (eng->hs_pass.empty()) eng->hs_pass.push_back(make_uint4(0u, 0u, 0u, 0u));
    eng->hs_mfma_pt = fm;
    eng->hs_flops_pt = fb + fm + (double)eng->np[eng->tmax - 1];
    eng->hs_rt = rt;
    eng->hs_nb = nb;
    eng->hs_nw = nw;
    if (eng->opts.hs_probe) eng->hs_probe = *eng->opts.hs_probe;
    return hs_lds(eng) <= eng->lds_max && eng->hs_kt.size() < (1u << 26);
}

// Wide-path plan: the direct plan's groups, items and per-use descriptors,
// plus the FP64 work per grid point of k_fwd_wide (every use a (nX+1)-term
// dot product with a weight multiply per term, one FMA into the state
// vector; the per-lane power tables; the final prior sum).  path: the wide
// forward the tables were built for.
int build_wide_plan(MdpEnginePlan *eng, const mdp_problem *p, MdpPath &path)
{
    path = MdpPath::WidePlain;
    int rc = build_direct_plan(eng, p);
    if (rc) return rc;
    // Q rows with at least one zero slot past the coefficients (slot ncoef:
    // k_fwd_mma's gathers of absent coefficients read it)
    eng->ldQ = ((size_t)eng->ncoef_d + 2) & ~(size_t)1;
    double f = 2.0 * (eng->maxA + 1) + 2.0 * eng->np[eng->tmax - 1];
    for (uint32_t d : eng->udesc_d) f += 3.0 * (((d >> kOffBits) & 31u) + 1.0) + 2.0;
    eng->wide_flops_pt = f;
    // k_fwd_mma's tables (c-independent): years of at most 256 states; per
    // year its K entries (k, |A_k|, m), padded to whole pipeline chunks with
    // entries naming the descriptor row npp (every transition absent), and the
    // transition descriptors [k][2^sh >= npcp] (Q-row offset | nX << kOffBits;
    // an absent transition names the zero slot with nX = 0)
    // MDP_WIDE_MMA: 0 -> k_fwd_wide; 1 -> round 5's k_fwd_mma (<= 256
    // states); 2 -> k_fwd_mmt (<= 1 024 states); 3 -> k_fwd_hs (nvar <= 10;
    // else k_fwd_mmt); unset -> k_fwd_hs for years of more than 64 states,
    // else k_fwd_mmt (measured, profiles/r06/hs: k_fwd_hs 1.3x / 4.4x / 5.2x
    // / 5.8x faster on 128 / 256 / 512 / 1 024 states, 1.27x slower on 64)
    const int mmode = eng->opts.wide_mma.value_or(eng->npmax > 64 ? 3 : 2);
    if (mmode == 3 && build_hs_plan(eng)) path = MdpPath::WideHs;
    else if ((mmode == 2 || mmode == 3) && build_mmt_plan(eng)) path = MdpPath::WideMmt;
    if (eng->npmax <= 256 && eng->maxA <= 24) {
        if (mmode == 1) {
            const uint32_t npm = eng->npmax <= 64 ? 64u : eng->npmax <= 128 ? 128u : 256u;
            const uint32_t pts = mma_pts(npm), ps = mma_ps(npm);
            const uint32_t none = (uint32_t)eng->ncoef_d;  // the zero slot, nX = 0
            eng->mma_npm = npm;
            eng->mma_kt.clear();
            eng->mma_desc.clear();
            eng->mma_kbase.assign(eng->tmax + 1, 0u);
            eng->mma_dbase.assign(eng->tmax + 1, 0u);
            eng->mma_ktmax = 16;
            size_t ub = 0;
            bool pad_overflow = false;
            for (uint32_t t = 1; t < eng->tmax; ++t) {
                const uint32_t npp = eng->np[t - 1], npc = eng->np[t], npcp = (npc + 15) / 16 * 16;
                uint32_t ld = 16;
                while (ld < npcp) ld *= 2;
                eng->mma_kbase[t] = (uint32_t)eng->mma_kt.size();
                eng->mma_dbase[t] = (uint32_t)eng->mma_desc.size();
                for (uint32_t k = 0; k < npp; ++k) {
                    const uint32_t a = eng->udesc_d[ub + k] >> 27;  // |A_k| (any use from k; l = 0)
                    for (uint32_t m = 0; m <= a; ++m)  // Va row k, xp row a - m, yp row m (bytes); m; k
                        eng->mma_kt.push_back(make_uint2((k * pts * 8u) | (((a - m) * ps * 8u) << 16),
                                                         (m * ps * 8u) | (m << 16) | (k * kMmaDummy)));
                }
                // padding names descriptor row npp through the 8-bit k field:
                // row 256 would wrap to row 0 (the advisor's round-5 finding),
                // so a 256-state year that needs padding leaves k_fwd_mma
                if (eng->mma_kt.size() % (4 * kMmaU) && npp > 255) pad_overflow = true;
                while (eng->mma_kt.size() % (4 * kMmaU)) eng->mma_kt.push_back(make_uint2(0u, npp * kMmaDummy));
                eng->mma_ktmax = std::max<uint32_t>(eng->mma_ktmax, (uint32_t)eng->mma_kt.size() - eng->mma_kbase[t]);
                for (uint32_t k = 0; k <= npp; ++k)
                    for (uint32_t l = 0; l < ld; ++l) {
                        uint32_t dv = none;
                        if (k < npp && l < npc) {
                            const uint32_t dsc = eng->udesc_d[ub + (size_t)l * npp + k];
                            dv = (dsc & kOffMask) | (((dsc >> kOffBits) & 31u) << kOffBits);
                        }
                        eng->mma_desc.push_back(dv);
                    }
                ub += (size_t)npp * npc;
            }
            eng->mma_kbase[eng->tmax] = (uint32_t)eng->mma_kt.size();
            eng->mma_dbase[eng->tmax] = (uint32_t)eng->mma_desc.size();
            // per year and wave its work item (k_fwd_mma): column tile, K
            // slice of S (at most 16 waves; slice 1 in the destination rows,
            // later ones in the rows past the year's column tiles; at least
            // two chunks each), chunk range
            eng->mma_wplan.assign((size_t)(eng->tmax + 1) * 16, make_uint2(0u, 0u));
            for (uint32_t t = 1; t < eng->tmax; ++t) {
                const uint32_t ncol = (eng->np[t] + 15) / 16, npcp = ncol * 16;
                const uint32_t nch = (eng->mma_kbase[t + 1] - eng->mma_kbase[t]) / (4 * kMmaU);
                const uint32_t room = 2 + (mma_rows(npm) - npcp) / npcp;
                const uint32_t S = std::min(std::min(16 / ncol, room), std::max(1u, nch / 2));
                for (uint32_t wv = 0; wv < 16; ++wv) {
                    const uint32_t item = wv % ncol, ks = wv / ncol;
                    const uint32_t cb = nch * ks / S, ce = nch * (ks + 1) / S;
                    eng->mma_wplan[(size_t)t * 16 + wv] =
                        make_uint2(cb | ce << 16, item | ks << 8 | S << 16 | (wv < ncol * S ? 1u : 0u) << 24);
                }
            }
            // (chunk reads past a year's entries are clamped into it; one
            // chunk of slack keeps the last year's clamp in the table)
            for (uint32_t i = 0; i < 4 * kMmaU; ++i) eng->mma_kt.push_back(make_uint2(0u, 0u));
            if (eng->mma_desc.empty()) eng->mma_desc.push_back(none);
            const size_t lmax = eng->lds_max;
            if (mma_lds(eng) <= lmax && none <= kOffMask && !pad_overflow) path = MdpPath::WideMma;
        }
    }
    return MDP_OK;
}

// Split a long series into chunks of whole years for the hipRTC forward
// kernel: at most `U` uses per chunk (straight-line code stays a bounded
// size), preferring a boundary year with one state (the smallest hand-over)
// in the last quarter of a chunk.  With `gather`, each chunk stages only the
// Q groups its uses read (at most kJitChunkQ doubles, a chunk-local layout of
// even-aligned groups) instead of the whole Q row.
int plan_chunks(MdpEnginePlan *eng, uint32_t U, bool gather, size_t qlimit)
{
    const MdpJitPlan &base = eng->jit_plan;
    const std::vector<uint32_t> &np = eng->np;
    const std::vector<uint32_t> &ud = eng->udesc_d;
    const uint32_t T = eng->tmax;
    const int epl = base.epl > 0 ? base.epl : mdp_jit_default_epl(ud);
    auto gsize = [](uint32_t d) { return (((d >> kOffBits) & 31u) + 2u) & ~1u; };  // nX + 1, even
    eng->chunks.clear();
    uint32_t t0 = 0;
    size_t u0 = 0;
    uint32_t e0 = 0;  // pending exponent of B at the chunk boundary (spom_jit.cpp)
    while (t0 + 1 < T) {
        size_t cur = 0, qloc = 0, u1 = u0, best_u1 = 0;
        uint32_t t1 = t0, best_t1 = 0;
        std::set<uint32_t> loc;
        while (t1 + 1 < T) {
            const size_t nu = (size_t)np[t1] * np[t1 + 1];
            size_t addq = 0;
            std::set<uint32_t> fresh;
            if (gather)
                for (size_t u = u1; u < u1 + nu; ++u) {
                    const uint32_t off = ud[u] & kOffMask;
                    if (!loc.count(off) && fresh.insert(off).second) addq += gsize(ud[u]);
                }
            if (cur > 0 && (cur + nu > U || (gather && qloc + addq > qlimit))) break;
            cur += nu;
            qloc += addq;
            loc.insert(fresh.begin(), fresh.end());
            u1 += nu;
            ++t1;
            if (np[t1] == 1 && 4 * cur >= 3 * (size_t)U) {
                best_t1 = t1;
                best_u1 = u1;
            }
        }
        if (t1 + 1 < T && best_t1 && best_t1 < t1) {
            t1 = best_t1;
            u1 = best_u1;
        }
        MdpJitPlan c = base;
        c.fused = false;
        c.epl = epl;
        c.np.assign(np.begin() + t0, np.begin() + t1 + 1);
        c.udesc.assign(ud.begin() + u0, ud.begin() + u1);
        c.first = t0 == 0;
        c.last = t1 + 1 == T;
        c.e0 = e0;
        e0 = mdp_jit_end_exp(c);
        if (gather) {  // chunk-local Q layout, groups in first-use order
            std::map<uint32_t, uint32_t> lo;
            c.qidx.clear();
            for (uint32_t &d : c.udesc) {
                const uint32_t off = d & kOffMask;
                auto it = lo.find(off);
                if (it == lo.end()) {
                    it = lo.emplace(off, (uint32_t)c.qidx.size()).first;
                    for (uint32_t m = 0; m < gsize(d); ++m) c.qidx.push_back(off + std::min(m, (d >> kOffBits) & 31u));
                }
                d = (d & ~kOffMask) | it->second;
            }
            c.ldq_row = base.ldQ;
        }
        eng->chunks.push_back(std::move(c));
        t0 = t1;
        u0 = u1;
    }
    return eng->chunks.empty() ? mdp_set_error(MDP_EUNSUPPORTED, "no forward chunks") : MDP_OK;
}

}  // namespace

// Z rows for a grid whose |c| <= cmax.  Z_j(c) = prod over the always-zero
// columns k of max(0, 1 - c S[j][k]) splits by the size of |c| S:
//  * |c| S <= 2^-55: the factor is exactly 1.0 -- dropped;
//  * 2^-55 < |c| S <= kZTau ("small"): never clamped, and their product is
//    exp(sum log(1 - c S)) = exp(-sum_i c^i P_i / i) with the power sums
//    P_i = sum_small S^i.  The series stops after kZTerms terms: the rest is
//    below sum_small (c S)^(kZTerms+1) / (kZTerms+1) <= 256 * 2^-63 / 9
//    < 2^-58 relative per 256 small columns (exp: ~1 ulp), so Z keeps
//    double precision while a row costs kZTerms FMAs and one exp instead of
//    an FMA and a multiply per column (config 3: 248 -> <= 24 columns a row);
//  * the rest ("large", |c| S > kZTau or not finite) stay explicit factors,
//    the largest first (the clamp test reads it).
// zs[k][row] / zsT[row][k] hold the large columns (kmax = the longest row
// rounded up to 8, zero padding = factor 1.0); zc[row][kZTerms] the series
// coefficients P_i / i (zero for a row without small columns: exp(0) = 1).
constexpr double kZTau = 0x1p-7;

void z_split(const MdpEnginePlan *eng, uint32_t js, double cmax, std::vector<double> &large, double *coef,
             std::vector<uint32_t> *cols)
{
    const uint32_t n = eng->n;
    large.clear();
    if (cols) cols->clear();
    size_t imax = 0;
    double pw[kZTerms] = {};
    for (uint32_t k = 0; k < n; ++k) {
        if (eng->isvar[k]) continue;
        const double sv = eng->Sj[(size_t)js * n + k];
        const double x = cmax * sv;
        if (x <= 0x1p-55) continue;  // false for NaN / inf: kept
        if (x <= kZTau) {
            double t = sv;
            for (int i = 0; i < kZTerms; ++i, t *= sv) pw[i] += t;
            continue;
        }
        if (!large.empty() && sv > large[imax]) imax = large.size();
        large.push_back(sv);
        if (cols) cols->push_back(k);
    }
    if (!large.empty()) std::swap(large[0], large[imax]);
    if (cols && !cols->empty()) std::swap((*cols)[0], (*cols)[imax]);
    if (coef)
        for (int i = 0; i < kZTerms; ++i) coef[i] = pw[i] / (double)(i + 1);
}

void mdp_plan_item_tables(const MdpEnginePlan *eng, std::vector<double> &sv, std::vector<uint2> &items)
{
    sv.assign((size_t)eng->nj * eng->nvar + 1, 0.0);
    for (uint32_t js = 0; js < eng->nj; ++js)
        for (uint32_t b = 0; b < eng->nvar; ++b)
            sv[(size_t)js * eng->nvar + b] = ((eng->cj_bits[js] >> (eng->nvar - 1 - b)) & 1u)
                                                  ? HUGE_VAL  // column of j: pC = fmin(c inf, 1) = 1.0
                                                  : eng->Sj[(size_t)js * eng->n + eng->var_cols[b]];
    items.assign(eng->nitems + 1, make_uint2(0u, 0u));
    for (uint32_t i = 0; i < eng->nitems; ++i) {
        const uint32_t r = eng->itemRow[i];
        items[i] = make_uint2(eng->itemB[i] | ((r & 0xffu) << 24), eng->cj_bits[r] | ((r >> 8) << 24));
    }
}

namespace {

// no fused kernel on the wide path, for a chunked series, Q rows built in HBM
// or state vectors in LDS
bool fused_path(const MdpEnginePlan *eng)
{
    return eng->path == MdpPath::Direct && eng->chunks.empty() && !eng->jit_plan.vlds;
}

// The c tables for the bound cmax.
void plan_ctables(const MdpEnginePlan *eng, double cmax, MdpCTables &t)
{
    const uint32_t nj = eng->nj;
    std::vector<std::vector<double>> rows(nj);
    t.zc.assign((size_t)nj * kZTerms + 1, 0.0);
    size_t kmax = 0;
    for (uint32_t js = 0; js < nj; ++js) {
        z_split(eng, js, cmax, rows[js], &t.zc[(size_t)js * kZTerms]);
        kmax = std::max(kmax, rows[js].size());
    }
    kmax = (kmax + 7) & ~(size_t)7;
    t.zs.assign(kmax * nj + 1, 0.0);
    for (uint32_t js = 0; js < nj; ++js)
        for (size_t k = 0; k < rows[js].size(); ++k) t.zs[js * kmax + k] = rows[js][k];
    // k_qrows' copy: row js's product chain q (columns k = q mod 4) contiguous
    t.zsq.assign(kmax * nj + 2, 0.0);  // + a double2 k_qrows may read at kmax 0
    for (uint32_t js = 0; js < nj; ++js)
        for (size_t k = 0; k < kmax; ++k) t.zsq[js * kmax + (k % 4) * (kmax / 4) + k / 4] = t.zs[js * kmax + k];
    t.cmax = cmax;
    t.kmax = (uint32_t)kmax;
    t.coltab.clear();
    t.ct_len = 0;
    if (!fused_path(eng)) return;
    // the fused kernel's column tables: one contiguous image it copies to LDS
    // (with zpad, all KZ zs rows, zero past kmax: the kernel reads them unmasked)
    const MdpJitPlan &pl = eng->jit_plan;
    const size_t kimg = pl.zpad ? std::max<size_t>(kmax, std::max<uint32_t>(8u, pl.kzmax)) : kmax;
    const size_t ct = ((size_t)pl.off_zs + kimg * nj + 127) & ~(size_t)127;
    std::vector<double> &img = t.coltab;
    img.assign(ct, 0.0);
    std::vector<double> sv;
    std::vector<uint2> items;
    mdp_plan_item_tables(eng, sv, items);
    memcpy(img.data(), sv.data(), (size_t)nj * eng->nvar * sizeof(double));
    memcpy(img.data() + pl.off_it, items.data(), (size_t)eng->nitems * sizeof(uint2));
    memcpy(img.data() + pl.off_qs, eng->qstart.data(), eng->qstart.size() * sizeof(uint32_t));
    memcpy(img.data() + pl.off_zc, t.zc.data(), (size_t)nj * kZTerms * sizeof(double));
    if (!eng->qitem.empty())
        memcpy(img.data() + pl.off_qi, eng->qitem.data(), eng->qitem.size() * sizeof(uint32_t));
    {
        const std::vector<uint32_t> rq = mdp_jit_reversed_index(pl.udesc, pl.ldQ);
        memcpy(img.data() + pl.off_rq, rq.data(), rq.size() * sizeof(uint32_t));
    }
    for (size_t k = 0; k < kmax; ++k)  // zs pairs (k, k+1) of a row adjacent: one ds_read_b128
        for (uint32_t js = 0; js < nj; ++js) img[pl.off_zs + ((k / 2) * nj + js) * 2 + (k & 1)] = t.zs[js * kmax + k];
    t.ct_len = (uint32_t)ct;
}

// The point list of forward kernels with `epl` points per lane: the e rows
// whose ratio form is s (x < y, x = min(e, 1), y = 1 - x, as the kernel
// computes them), then those of form t, each run padded to a multiple of epl
// with duplicates of its last row (bit 31: computed, not stored), so every
// lane's points share one form and so their coefficient reads.  A sorted
// grid keeps its order (the kernels' stores stay coalesced).
std::vector<uint32_t> point_list(const double *e, uint32_t ne, uint32_t epl)
{
    std::vector<uint32_t> s_rows, t_rows;
    for (uint32_t i = 0; i < ne; ++i) {
        const double x = e[i] > 1.0 ? 1.0 : e[i], y = 1.0 - x;
        (x >= y ? t_rows : s_rows).push_back(i);
    }
    std::vector<uint32_t> pl;
    pl.reserve(ne + 2 * epl);
    for (const auto *rows : {&s_rows, &t_rows}) {
        pl.insert(pl.end(), rows->begin(), rows->end());
        while (!rows->empty() && pl.size() % epl) pl.push_back(rows->back() | 0x80000000u);
    }
    if (pl.empty()) pl.assign(epl, 0x80000000u);
    return pl;
}

// c values per launch of a wide-path kernel that takes at most `fit` of them
// in its scratch (MDP_WIDE_CB: tests force several launches per slot)
uint32_t wide_cb(size_t most, size_t fit, int forced)
{
    const uint32_t cb = (uint32_t)std::min(most, std::max<size_t>(1, fit));
    return forced ? std::min(cb, (uint32_t)std::max(1, forced)) : cb;
}

}  // namespace

bool mdp_plan_fused_capable(const MdpEnginePlan *eng)
{
    return fused_path(eng) && fused_lds(eng, eng->jit_plan.ct_max) <= kFusedLdsMax;
}

int mdp_plan_grid(const MdpEnginePlan *eng, MdpCTables &ct, const double *e, uint32_t ne, const double *c, uint32_t nc,
                  uint32_t ncu, MdpGridPlan &g)
{
    // c < 0 is refused: the item factors are folded as |n_b - pC_b| (k_qrows
    // phase 2, k_witems, the fused prologue), which equals the reference's
    // (1 - piold)(1 - pC) + piold pC (main_MIDASPOM.c:40) only for pC >= 0;
    // at c < 0 the reference's pC = min(1, c S) is negative, not a probability
    // (and a NaN or infinite c: the pressures min(1, c S) are then clamped
    // by minNum, which drops NaN, where the reference would carry it)
    for (uint32_t i = 0; i < nc; ++i)
        if (!(c[i] >= 0.0) || std::isinf(c[i]))
            return mdp_set_error(MDP_EINVAL, "colonisation rate c[%u] = %g (the engine takes finite c >= 0)", i, c[i]);
    g = MdpGridPlan();
    for (uint32_t i = 0; i < ne; ++i) {  // the kernels' form test: x = min(e, 1), s-form where x < 1 - x
        const double x = e[i] > 1.0 ? 1.0 : e[i];
        g.ne_sform += x < 1.0 - x;
    }
    const MdpPath path = eng->path;
    const bool qglobal = path_q_global(path);  // Q rows from k_zrows + k_witems + k_wq
    if (path != MdpPath::Generic) {
        double cmax = eng->cbound;
        for (uint32_t i = 0; i < nc; ++i) cmax = std::max(cmax, std::fabs(c[i]));
        g.n_qrow = (size_t)nc * eng->ldQ;
        if (!(ct.cmax == cmax)) {
            plan_ctables(eng, cmax, ct);
            g.tables_new = true;
        }
    }
    if (qglobal) {
        g.n_zg = (size_t)nc * eng->nj + 1;
        // k_zrows stages kZRows rows of explicit columns in dynamic LDS
        g.zrows_lds = (size_t)kZRows * ct.kmax * sizeof(double);
        if (g.zrows_lds > kQrowsLdsMax)
            return mdp_set_error(MDP_EUNSUPPORTED, "%u explicit colonisation columns per row exceed the LDS of k_zrows",
                                 ct.kmax);
    }
    const int forced_cb = qglobal ? eng->opts.wide_cb.value_or(0) : 0;
    const size_t most_c = std::max<size_t>(1, std::min<size_t>(nc, 65535));  // a launch's grid y
    if (path == MdpPath::WideHs) {  // k_fwd_hs reads the item factors of its columns: rows of nitems + 1 (zero slot)
        const size_t ldp = (size_t)eng->nitems + 1;
        g.wide_cb_items = wide_cb(nc, kHsPgBytes / 8 / ldp, forced_cb);
        g.n_pg = (size_t)g.wide_cb_items * ldp;
        g.pg_zero = true;
    } else if (qglobal) {  // c values per k_witems launch: item factors within kWidePgBytes
        g.wide_cb_items = wide_cb(most_c, kWidePgBytes / 8 / std::max<size_t>(1, eng->nitems), forced_cb);
        g.n_pg = (size_t)g.wide_cb_items * eng->nitems + 1;
    }
    if (path_is_wide(path)) {
        // c values per k_fwd_wide launch: the two state vectors of every
        // point of a launch within kWideVBytes (the matrix-core forwards keep
        // them in LDS; k_fwd_hs does too, its reservation is unused)
        const size_t ne_pad = (size_t)std::max<uint32_t>(1u, (ne + kBlock - 1) / kBlock) * kBlock;
        g.wide_cb_fwd = wide_cb(most_c, kWideVBytes / 8 / (2 * (size_t)eng->npmax * ne_pad), forced_cb);
        if (path == MdpPath::WidePlain || path == MdpPath::WideHs) g.n_v = 2 * (size_t)eng->npmax * g.wide_cb_fwd * ne_pad;
    } else if (path_is_jit(path)) {
        // forward kernels with several points per lane read them from a list
        // that puts only e rows of one ratio form in a lane (spom_jit.cpp)
        const uint32_t epl = (uint32_t)eng->jit_epl;  // (the fused variant lists at the reading variant's: jit_source)
        if (epl > 1) {
            g.plist = point_list(e, ne, epl);
            for (uint32_t i = 0; i < g.plist.size() && g.plist_identity; ++i) g.plist_identity = g.plist[i] == i;
            g.nlist = (uint32_t)g.plist.size();
            if (!g.plist_identity) {  // an identity list is not uploaded: the kernels use the position
                g.elist.resize(g.plist.size() + 1);
                for (size_t i = 0; i < g.plist.size(); ++i)
                    g.elist[i] = ne ? e[g.plist[i] & 0x7fffffffu] : 0.0;  // (no rows: never run)
                g.elist[g.plist.size()] = ne ? e[0] : 0.0;
            }
        } else {
            g.nlist = ne;
        }
        g.nlist_epl = epl;
        // one e block per c column and a small per-c problem: the forward
        // kernel computes its column's Q itself (one launch); never for a
        // chunked series or Q rows built in HBM
        g.gy = (g.nlist + eng->jit_kblock * epl - 1) / (eng->jit_kblock * epl);
        g.fused = fused_path(eng) && fused_lds(eng, ct.ct_len) <= kFusedLdsMax && ct.kmax <= eng->jit_plan.kzmax &&
                  (eng->fused_mode == 1 || (eng->fused_mode == -1 && g.gy <= 1));
        // a column of a tall grid (an even number of e blocks, so no lane more
        // idles) in half the blocks of twice the threads: each block stages
        // its column's Q row once (config 3: forward 45.7-46.9 -> 44.3 us) --
        // while that still leaves a block for every CU (a column slab of
        // config 3, 1 024 x 128: 128 tall blocks would idle half the chip)
        g.tall = !g.fused && eng->chunks.empty() && !eng->jit_plan.vlds && !eng->jit_shape_env &&
                 eng->jit_kblock * 2 == (uint32_t)kJitKblockTall && g.gy >= 2 && g.gy % 2 == 0 &&
                 (uint64_t)nc * (g.gy / 2) >= ncu;
        g.variant = g.fused ? 1 : g.tall ? 2 : 0;
        if (!eng->chunks.empty()) {  // the state vectors handed between chunks
            g.ldv = g.gy * eng->jit_kblock * epl;
            uint32_t nb = 1;  // most states at a chunk boundary
            for (size_t i = 1; i < eng->chunks.size(); ++i) nb = std::max(nb, eng->chunks[i].np[0]);
            g.n_vscr = (size_t)nb * nc * g.ldv;
        }
        // c values per k_qrows workgroup: enough workgroups for every CU, within the LDS
        uint32_t cb = nc >= 1024 ? kQrowsMaxC : nc >= 512 ? 2u : 1u;  // power of two
        cb = std::min(cb, eng->nvar <= 8 ? 4u : eng->nvar <= 16 ? 2u : 1u);  // registers (k_qrows)
        while (cb > 1 && qrows_lds(eng, cb) > kQrowsLdsMax) cb >>= 1;
        g.qrows_cb = cb;
    } else {
        g.n_zpv = (size_t)nc * (eng->nvar + 1) * eng->nstates;
        g.n_r = (size_t)nc * ldR_of(eng);
        if (!eng->lds_part) g.n_gpart = (size_t)nc * eng->partP.size() * (eng->nvar + 1);
    }
    mdp_plan_steps(eng, g);
    if (eng->diag) {
        g.nst[0] = path_is_jit(path) ? (size_t)nc : (size_t)((eng->nstates + kZpvJ - 1) / kZpvJ) * ((nc + kZpvCT - 1) / kZpvCT);
        g.nst[1] = nc;
        g.nst[2] = (size_t)nc * ((ne + kBlock - 1) / kBlock);  // >= the JIT grid (EPL >= 1)
    }
    return MDP_OK;
}

void mdp_plan_fwd_launch(const MdpEnginePlan *eng, const MdpCTables &ct, uint32_t ne, uint32_t nc, MdpGridPlan &g)
{
    // threads per e block: kb (x spl with the split state-vector kernel)
    const uint32_t kb = g.fused ? eng->jit_kblock_fused : g.tall ? (uint32_t)kJitKblockTall : eng->jit_kblock;
    const uint32_t pro = g.fused ? eng->jit_pro_fused : 1u;
    const uint32_t epl = g.fused ? (uint32_t)eng->jit_epl_fused : (uint32_t)eng->jit_epl;
    const uint32_t spl = eng->jit_plan.vlds && (eng->jit_plan.vsplit == 2 || eng->jit_plan.vsplit == 4)
                             ? (uint32_t)eng->jit_plan.vsplit : 1u;
    const uint32_t fc = g.fused ? (uint32_t)eng->jit_plan.fused_cols : 1u;
    // several points per lane: the grid's point list
    g.fwd_listed = epl > 1 && !g.plist_identity;
    g.fwd_nlist = epl > 1 ? g.nlist : ne;
    const uint64_t gy = (g.fwd_nlist + kb * epl - 1) / (kb * epl);
    g.fwd_nblk = gy * ((nc + fc - 1) / fc);  // e blocks x column groups
    g.fwd_pro = pro;
    g.fwd_threads = g.fwd_nblk * kb * fc * spl;
    g.fwd_block = kb * fc * spl * pro;
    g.fwd_lds = g.fused ? (ct.ct_len + 2) * (uint32_t)sizeof(double) : 0u;  // + staging scratch
}

void mdp_plan_steps(const MdpEnginePlan *eng, MdpGridPlan &g)
{
    // the Q-global paths keep k_zrows for their item kernel, and run neither
    // without items; the direct path computes its Z rows inside k_qrows (slot
    // 0 idle), the fused kernel its Q rows as well
    const MdpStep none = MdpStep::None, zrows = eng->nitems ? MdpStep::Zrows : none;
    const MdpStep items = !eng->nitems ? none : eng->path == MdpPath::WideHs ? MdpStep::ItemsAll : MdpStep::ItemsQ;
    const MdpStep jit = eng->chunks.empty() ? MdpStep::FwdJit : MdpStep::FwdJitChunks;
    auto set = [&](MdpStep s0, MdpStep s1, MdpStep s2) { g.step[0] = s0, g.step[1] = s1, g.step[2] = s2; };
    switch (eng->path) {
    case MdpPath::Generic: return set(MdpStep::Zpv, eng->nuses ? MdpStep::Coefs : none, MdpStep::FwdGeneric);
    case MdpPath::Direct: return set(none, eng->nitems && !g.fused ? MdpStep::Qrows : none, jit);
    case MdpPath::DirectQGlobal: return set(zrows, items, jit);
    case MdpPath::WideHs: return set(zrows, items, MdpStep::FwdHs);
    case MdpPath::WideMmt: return set(zrows, items, MdpStep::FwdMmt);
    case MdpPath::WideMma: return set(zrows, items, MdpStep::FwdMma);
    case MdpPath::WidePlain: return set(zrows, items, MdpStep::FwdPlain);
    }
}

std::vector<std::string> mdp_plan_grid_kernels(const MdpEnginePlan *eng, const MdpGridPlan &g, uint32_t ne, uint32_t nc)
{
    std::set<std::string> names;
    auto note = [&](const char *fmt, auto... a) {
        char b[96];
        snprintf(b, sizeof b, fmt, a...);
        names.insert(b);
    };
    auto witems = [&]() { for_nv(eng, [&](auto nv) { note(kFmtWitems, nv()); }); };
    for (int k = 0; k < 3 && ne && nc; ++k) {
        switch (g.step[k]) {
        case MdpStep::None: break;
        case MdpStep::Zpv: names.insert("k_zpv"); break;
        case MdpStep::Coefs:
            for_coefs(eng, [&](auto ldsz, auto ldsp, auto nv) { note(kFmtCoefs, (int)ldsz(), (int)ldsp(), nv()); });
            break;
        case MdpStep::FwdGeneric: break;  // (left to its launcher)
        case MdpStep::Zrows: names.insert("k_zrows"); break;
        case MdpStep::Qrows:
            for_qrows(eng, g.qrows_cb, [&](auto nv, auto ex, auto cb) { note(kFmtQrows, nv(), (int)ex(), cb()); });
            break;
        case MdpStep::ItemsQ:
            witems();
            names.insert("k_wq");
            break;
        case MdpStep::ItemsAll:
            if (g.wide_cb_items >= nc) witems();
            break;
        case MdpStep::FwdJit:
            note(kFmtJit, g.fused ? "fused" : "reading", eng->maxA);
            if (g.tall) note(kFmtJitTall, kJitKblockTall);
            break;
        case MdpStep::FwdJitChunks:
            note(kFmtJitChunks, eng->maxA, eng->chunks.size(), eng->chunks[0].qidx.empty() ? "" : ",gather");
            break;
        case MdpStep::FwdHs:
            if (g.wide_cb_items < nc && eng->nitems) witems();
            note(kFmtHs, eng->hs_rt, eng->hs_nb);
            break;
        case MdpStep::FwdMmt: note(kFmtMmt, eng->mmt_rt, eng->mmt_rows, mmt_shape(eng).db ? "2buf" : "1buf"); break;
        case MdpStep::FwdMma: note(kFmtMma, eng->mma_npm); break;
        case MdpStep::FwdPlain: names.insert("k_fwd_wide"); break;
        }
    }
    return std::vector<std::string>(names.begin(), names.end());
}

// The source of the engine's forward kernel: variant 0 reading, 1 fused, 2
// reading at kJitKblockTall threads (a column of a tall grid in half the
// blocks: its Q row staged half as often).  Sets the engine's launch shape of
// the variant.
std::string jit_source(MdpEnginePlan *eng, int variant)
{
    const bool fused = variant == 1;
    MdpJitPlan plan = eng->jit_plan;
    plan.fused = fused;
    if (variant == 2) {  // the reading kernel's points per lane, more threads
        plan.epl = eng->jit_epl > 0 ? eng->jit_epl : mdp_jit_default_epl(plan.udesc);
        plan.kblock = kJitKblockTall;
        return mdp_jit_forward_source(plan);
    }
    // the reading variant's shape (e rows per block = kblock x epl, which
    // mdp_plan_grid's block count uses before it picks the variant)
    const int epl_r = plan.epl > 0 ? plan.epl : mdp_jit_default_epl(plan.udesc);
    const int kb_r = plan.kblock > 0 ? plan.kblock : kBlock;
    eng->jit_epl = epl_r;
    eng->jit_kblock = (uint32_t)kb_r;
    if (fused && !eng->jit_shape_env) {
        // the same e rows per block as the reading variant (kb_r x epl_r, the
        // grid shape is shared), the forward at its points per lane, and
        // twice the threads for the column-table prologue (pro 2): a
        // forward at one point per lane was LDS-bound (each broadcast pair
        // read feeds half the FMAs), while the prologue wants every thread
        plan.kblock = kb_r;
        plan.epl = epl_r;
        plan.pro = 2;
    }
    if (fused) {  // at most 1 024 threads a workgroup: fewer prologue threads, then fewer columns
        const int fc = std::max(1, plan.fused_cols);
        if (plan.kblock * fc * std::max(1, plan.pro) > 1024) plan.pro = 1;
        if (plan.kblock * fc > 1024) plan.fused_cols = std::max(1, 1024 / std::max(1, plan.kblock));
        eng->jit_plan.fused_cols = plan.fused_cols;  // the launch's columns per workgroup
    }
    const std::string src = mdp_jit_forward_source(plan);
    if (fused) {
        eng->jit_epl_fused = plan.epl;
        eng->jit_kblock_fused = (uint32_t)plan.kblock;
        eng->jit_pro_fused = (uint32_t)std::max(1, plan.pro);
    }
    eng->jit_flops_pt = plan.flops_pt;
    if (eng->opts.jit_dump) {  // <path>.hip (reading) / <path>.fused.hip
        if (FILE *f = fopen((*eng->opts.jit_dump + (fused ? ".fused.hip" : ".hip")).c_str(), "w")) {
            fputs(src.c_str(), f);
            fclose(f);
        }
    }
    return src;
}

// Compile (hipRTC, cached) that kernel.
int jit_build(MdpEnginePlan *eng, int variant)
{
    if (!eng->jit_code[variant].empty()) return MDP_OK;
    const std::string src = jit_source(eng, variant);
    if (mdp_jit_compile(src, eng->jit_code[variant], eng->jit_log) != 0)
        return mdp_set_error(MDP_EHIP, "hipRTC compilation of the forward kernel failed: %s",
                             eng->jit_log.c_str());
    eng->jit_src[variant] = src;
    return MDP_OK;
}

// Compile every chunk kernel of a long series (threads: hipRTC programs are
// independent).
int jit_build_chunks(MdpEnginePlan *eng)
{
    const size_t nch = eng->chunks.size();
    if (eng->chunk_code.size() == nch) return MDP_OK;
    std::vector<std::vector<char>> code(nch);
    std::vector<std::string> logs(nch);
    std::vector<int> rcs(nch, 0);
    std::vector<std::string> srcs(nch);
    double flops = 0.0;
    for (size_t i = 0; i < nch; ++i) {
        srcs[i] = mdp_jit_forward_source(eng->chunks[i]);
        flops += eng->chunks[i].flops_pt;
        if (eng->opts.jit_dump)
            if (FILE *f = fopen((*eng->opts.jit_dump + ".chunk" + std::to_string(i) + ".hip").c_str(), "w")) {
                fputs(srcs[i].c_str(), f);
                fclose(f);
            }
    }
    {
        std::vector<std::thread> th;
        size_t nt = std::min<size_t>(8, nch);
        if (eng->opts.jit_threads) nt = std::max<size_t>(1, std::min<size_t>(nch, *eng->opts.jit_threads));
        const bool verbose = eng->opts.jit_verbose;
        for (size_t t = 0; t < nt; ++t)
            th.emplace_back([&, t]() {
                for (size_t i = t; i < nch; i += nt) {
                    const auto t0 = std::chrono::steady_clock::now();
                    rcs[i] = mdp_jit_compile(srcs[i], code[i], logs[i]);
                    if (verbose)
                        fprintf(stderr, "chunk %zu: %zu uses, %.2f s\n", i, eng->chunks[i].udesc.size(),
                                std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
                }
            });
        for (auto &x : th) x.join();
    }
    for (size_t i = 0; i < nch; ++i)
        if (rcs[i]) {
            eng->jit_log = logs[i];
            return mdp_set_error(MDP_EHIP, "hipRTC compilation of forward chunk %zu failed: %s", i, logs[i].c_str());
        }
    eng->chunk_code = std::move(code);
    eng->chunk_src = std::move(srcs);
    eng->jit_epl = eng->chunks[0].epl;
    eng->jit_kblock = (uint32_t)eng->chunks[0].kblock;
    eng->jit_flops_pt = flops;
    return MDP_OK;
}

// ---------------------------------------------------------------------------
// mdp_plan_engine's steps
// ---------------------------------------------------------------------------
namespace {

constexpr uint32_t kVldsBlock = kBlock;  // vlds: points per workgroup (their states: npmax x kVldsBlock doubles of LDS)

// What the direct-path choice hands to the steps after it.
struct DirectChoice {
    bool vlds = false;      // years of 17-64 states on the specialised kernel, their state vectors in LDS
    bool want_jit = false;  // the specialised kernel is wanted and the direct plan is built
    bool qglobal = false;   // its Q rows are built in HBM
    bool gather = false, chunked = false;  // the series runs as chunks of years (gather: each its own Q layout)
    uint32_t chunk_uses = kJitChunkUses;   // target uses per chunk
    size_t qlimit = 0;      // coefficients a forward kernel may stage
};

// an option that was given overrides what the plan holds
template <typename T, typename U>
void take(T &dst, const std::optional<U> &src)
{
    if (src) dst = (T)*src;
}

// Which direct plan, if any: builds it (build_direct_plan) and sets ldQ, also
// when it is not wanted.  wide: in, the generic plan's verdict; out, cleared
// when the vlds kernel takes the wide years.
DirectChoice choose_direct(MdpEnginePlan *eng, const mdp_problem *p, bool &wide)
{
    const MdpOpts &o = eng->opts;
    DirectChoice dc;
    // years of 17-64 states: the specialised forward kernel with its
    // state vectors in LDS (plan.vlds), unless the series is so long that
    // hipRTC would take minutes; MDP_WIDE=1 forces the wide kernels
    if (wide && !o.wide && o.jit && eng->npmax <= kVldsMaxStates &&
        eng->nuses <= o.vlds_maxuses.value_or(kVldsMaxUses)) {
        wide = false;
        dc.vlds = true;
    }
    dc.want_jit = !wide && o.jit && build_direct_plan(eng, p) == MDP_OK;
    // k_qrows keeps every table of its c values in LDS; larger problems
    // build their Q rows in HBM (k_zrows + k_witems + k_wq, the same bits)
    dc.qglobal = dc.want_jit && (qrows_lds(eng, 1) > kQrowsLdsMax || o.qglobal);
    eng->ldQ = ((size_t)eng->ncoef_d + 1) & ~(size_t)1;
    // a series longer than kJitMaxUses uses (or a Q row past the LDS) runs
    // as chunks of years (MDP_JIT_CHUNK / MDP_JIT_GATHER force them)
    dc.chunk_uses = o.jit_chunk.value_or(kJitChunkUses);
    // coefficients a forward kernel may stage: what the LDS leaves beside
    // the wide years' state vectors (npmax x 256 lanes) when they are there
    // (halved: the forward kernel keeps each Q row twice, in stored and in
    // reversed group order -- spom_jit.cpp, the ratio forms)
    dc.qlimit = (dc.vlds ? std::min(kJitChunkQ, (kQrowsLdsMax - (size_t)eng->npmax * kVldsBlock * sizeof(double) - 2048) /
                                                    sizeof(double))
                         : kJitChunkQ) / 2;
    dc.gather = eng->ldQ > dc.qlimit || o.gather;
    dc.chunked = eng->nuses > kJitMaxUses || dc.gather || (o.jit_chunk && eng->nuses > dc.chunk_uses);
    return dc;
}

// eng->jit_plan from the direct plan and the options: the generator's
// switches, the series, the counts and the fused kernel's column-table layout.
void fill_jit_plan(MdpEnginePlan *eng, bool vlds)
{
    const MdpOpts &o = eng->opts;
    MdpJitPlan &plan = eng->jit_plan;
    if (vlds) {  // the wide years' states in LDS: one point per lane, never fused
        plan.vlds = true;
        // points per lane: 1, or 2 (MDP_VLDS_EPL=2: 128 lanes per wave
        // group, each Q read shared by two points)
        plan.epl = o.vlds_epl.value_or(1);
        plan.kblock = (int)kVldsBlock / plan.epl;
        plan.window = 16;
        eng->fused_mode = 0;
        take(plan.vsplit, o.vsplit);
    }
    plan.np = eng->np;
    plan.udesc = eng->udesc_d;
    plan.ldQ = eng->ldQ;
    plan.diag = eng->diag;
    take(plan.slots, o.jit_slots);
    take(plan.wpe, o.jit_wpe);
    take(plan.xcd, o.jit_xcd);
    take(plan.efast, o.jit_efast);
    take(eng->qrows_xcd, o.qrows_xcd);
    take(plan.epl, o.epl);
    take(plan.window, o.jit_window);
    take(eng->fused_mode, o.fused);
    take(plan.fused_cols, o.fused_cols);
    take(plan.hack, o.jit_hack);
    take(plan.fast_log, o.fast_log);
    if (!vlds) take(plan.kblock, o.jit_kblock);
    eng->jit_shape_env = o.epl || (o.jit_kblock && !vlds);
    take(plan.split_forms, o.jit_split);
    take(plan.rot, o.jit_rot);
    plan.nj = eng->nj;
    plan.nvar = eng->nvar;
    plan.nitems = eng->nitems;
    plan.ncoef = eng->ncoef_d;
    plan.nqi = (uint32_t)eng->qitem.size();
    {   // zs rows compiled into the fused kernel: the longest row of
        // explicit columns at |c| <= 1 (the default grid); a grid
        // with more (|c| > 1) runs k_zrows + k_qrows instead
        size_t kz = 0;
        std::vector<double> large;
        for (uint32_t js = 0; js < eng->nj; ++js) {
            z_split(eng, js, 1.0, large, nullptr);
            kz = std::max(kz, large.size());
        }
        plan.kzmax = (uint32_t)std::max<size_t>(8, (kz + 7) & ~(size_t)7);
    }
    plan.qmaxlen = 0;
    for (size_t q = 0; q + 1 < eng->qstart.size(); ++q)
        plan.qmaxlen = std::max(plan.qmaxlen, eng->qstart[q + 1] - eng->qstart[q]);
    auto even = [](size_t v) { return (uint32_t)((v + 1) & ~(size_t)1); };
    plan.off_it = even((size_t)eng->nj * eng->nvar);
    plan.off_qs = even(plan.off_it + eng->nitems);
    plan.off_qi = even(plan.off_qs + (eng->ncoef_d + 2) / 2);
    plan.off_rq = even(plan.off_qi + (eng->qitem.size() + 1) / 2);
    plan.off_zc = even(plan.off_rq + (eng->ldQ + 1) / 2);
    plan.off_zs = even(plan.off_zc + (size_t)eng->nj * kZTerms);
    // the largest image (kzmax >= 8 zs rows), and whether it fits the fused
    // kernel's LDS: then the zs image is always zero-padded to it
    const size_t ct_full = ((plan.off_zs + (size_t)plan.kzmax * eng->nj) + 127) & ~(size_t)127;
    plan.ct_max = (uint32_t)std::min<size_t>(ct_full, kFusedLdsMax / sizeof(double));
    plan.zpad = fused_lds(eng, ct_full) <= kFusedLdsMax;
}

// MDP_JIT_CHECK=1 without a device: compile every forward kernel of the plan,
// then MDP_ENODEV with the plan's counts in the message.
int report_offline(MdpEnginePlan *eng, const DirectChoice &dc)
{
    const MdpJitPlan &plan = eng->jit_plan;
    if (dc.chunked) {
        const int r = jit_build_chunks(eng);
        if (!r)
            mdp_set_error(MDP_ENODEV, "no HIP device available (forward kernels compiled; %zu chunks%s; "
                          "nj %u nitems %u ldQ %zu qglobal %d)", eng->chunks.size(), dc.gather ? ", gathered Q" : "",
                          plan.nj, plan.nitems, (size_t)plan.ldQ, (int)dc.qglobal);
        return r ? r : MDP_ENODEV;
    }
    const int r0 = jit_build(eng, false), r1 = r0 ? r0 : jit_build(eng, true);
    uint32_t ipr = 0;  // most items of one row
    for (uint32_t js = 0; js + 1 < eng->cj_item0.size(); ++js)
        ipr = std::max(ipr, eng->cj_item0[js + 1] - eng->cj_item0[js]);
    if (!r1)
        mdp_set_error(MDP_ENODEV,
                      "no HIP device available (forward kernels compiled; nj %u nitems %u "
                      "items/row %u ldQ %zu qitems %u qmaxlen %u kzmax %u qrows slots %u conflicts %u + %u fused LDS %zu)",
                      plan.nj, plan.nitems, ipr, (size_t)plan.ldQ, plan.nqi, plan.qmaxlen, plan.kzmax,
                      eng->npl_slots, eng->slot_conflicts, eng->slot_store_conflicts,
                      fused_lds(eng, ((plan.off_zs + (size_t)plan.kzmax * eng->nj) + 127) & ~(size_t)127));
    return r1 ? r1 : MDP_ENODEV;
}

// Compile now the variant the first grid most likely runs (the fused kernel
// wherever its tables fit: every grid of at most one e block per column takes
// it), the other on demand (set_grid_dev's jit_load).  False, with the log on
// stderr: no specialised kernel, the generic or wide kernels take the problem.
bool first_compile(MdpEnginePlan *eng, const DirectChoice &dc, MdpPlanMode mode, double *jit_t)
{
    auto st_now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const bool fused_first = eng->fused_mode == 1 || (eng->fused_mode == -1 && !dc.vlds && !dc.qglobal &&
                                                      fused_lds(eng, eng->jit_plan.ct_max) <= kFusedLdsMax);
    if (jit_t) jit_t[0] = st_now();
    const int jrc = mode == MdpPlanMode::TablesOnly ? MDP_OK
                    : dc.chunked                    ? jit_build_chunks(eng)
                                                    : jit_build(eng, fused_first);
    if (jit_t) jit_t[1] = st_now();
    if (jrc != MDP_OK)
        fprintf(stderr, "midaspom: hipRTC specialisation failed, using the %s kernels:\n%s\n", dc.vlds ? "wide" : "generic",
                eng->jit_log.c_str());
    return jrc == MDP_OK;
}

}  // namespace

// The planning half of mdp_engine_create_opts (declared in spom_engine.h).  On
// an error, and after an offline check (MDP_ENODEV with the counts in the
// message), the caller deletes the engine.
int mdp_plan_engine(MdpEnginePlan *eng, const mdp_problem *p, size_t lds_max, MdpPlanMode mode, double *jit_t)
{
    const MdpOpts &o = eng->opts;
    eng->lds_max = lds_max;
    // the path is decided in these locals and assigned once, at the end
    bool wide = false, jit = false;
    int rc = build_plan(eng, p, wide);
    if (rc) return rc;
    eng->fwd_lds_bytes = ldR_of(eng) * sizeof(double) + (eng->prog.size() + 1) * sizeof(uint32_t);
    eng->fwd_lds = eng->fwd_lds_bytes <= kFwdLds && !o.fwd_scalar;
    if (o.epl && (*o.epl == 1 || *o.epl == 2 || *o.epl == 4)) eng->epl = *o.epl;
    take(eng->diag, o.diag);
    const DirectChoice dc = choose_direct(eng, p, wide);
    if (dc.want_jit && eng->nuses > 0) {
        fill_jit_plan(eng, dc.vlds);
        if (dc.chunked && (rc = plan_chunks(eng, dc.chunk_uses, dc.gather, dc.qlimit))) return rc;
        if (mode == MdpPlanMode::OfflineCheck) return report_offline(eng, dc);
        jit = first_compile(eng, dc, mode, jit_t);
    }
    if (dc.vlds && !jit) {  // no specialised kernel after all: the wide kernels take the problem
        wide = true;
        eng->chunks.clear();
    } else if (dc.vlds) {
        eng->variant = (eng->npmax <= 32 ? 32u : eng->npmax <= 64 ? 64u : 128u) * 100u + eng->deg;
    }
    MdpPath path = !jit ? MdpPath::Generic : dc.qglobal ? MdpPath::DirectQGlobal : MdpPath::Direct;
    if (wide) {
        if ((rc = build_wide_plan(eng, p, path))) return rc;
        if (mode == MdpPlanMode::OfflineCheck) return mdp_set_error(MDP_ENODEV, "no HIP device available (wide path planned)");
    }
    eng->path = path;
    return MDP_OK;
}

// The arithmetic of mdp_engine_get_info, mdp_engine_work and
// mdp_engine_work_fact (the ABI wrappers, spom_engine.hip, pass what they
// take from the device contexts).
void mdp_plan_info(const MdpEnginePlan *eng, int n_devices, mdp_engine_info *info)
{
    info->n_devices = n_devices;
    info->npairs = eng->npairs;
    info->nuses = eng->nuses;
    info->ncoef = eng->ncoef;
    info->npmax = eng->npmax;
    info->variant = eng->variant + (path_is_jit(eng->path) ? 10000u : 0u);
}

void mdp_plan_work(const MdpEnginePlan *eng, uint64_t ne, uint64_t nc, double *flop_impl, double *flop_survey,
                   double *bytes_min)
{
    const double pts = (double)ne * (double)nc;
    // k_forward per point: every use is a (D+1)-term dot product (2(D+1)
    // flops) and one multiply-add into the state vector (2), plus the
    // (D+1)-term weight setup and the final prior sum.
    const double D = (double)eng->deg;
    double per_pt = (double)eng->nuses * (2.0 * (D + 1.0) + 2.0) + 3.0 * (D + 1.0) +
                    2.0 * (double)eng->npmax;
    switch (eng->path) {
    case MdpPath::Generic: break;
    case MdpPath::Direct:
    case MdpPath::DirectQGlobal: per_pt = eng->jit_flops_pt; break;  // the generated code's own count
    case MdpPath::WideHs: per_pt = eng->hs_flops_pt; break;
    case MdpPath::WideMmt: per_pt = eng->mmt_flops_pt; break;
    case MdpPath::WideMma:
    case MdpPath::WidePlain: per_pt = eng->wide_flops_pt; break;
    }
    if (flop_impl) *flop_impl = per_pt * pts;
    // SURVEY.md §8(d) F_alg (dense-in-j formulation)
    double fwd = 0;
    for (uint32_t t = 1; t < eng->tmax; ++t) fwd += (double)eng->np[t - 1] * eng->np[t];
    const double falg = 2.0 * eng->n * eng->nstates + (double)eng->nvar * eng->nstates * eng->nextid +
                        2.0 * eng->nstates * eng->npairs + 2.0 * eng->np[0] * fwd;
    if (flop_survey) *flop_survey = falg * pts;
    // compulsory bytes of k_forward: its coefficient stream once per c, the
    // e values, the output
    if (bytes_min)
        *bytes_min = 8.0 * ((double)nc * (eng->path != MdpPath::Generic ? eng->ldQ : ldR_of(eng)) + (double)ne + pts);
}

// cmax: the bound the device's c tables hold for (< 0: none yet); ns of nall:
// the current grid's e rows on the s-form, over the devices
void mdp_plan_work_fact(const MdpEnginePlan *eng, uint64_t ne, uint64_t nc, double cmax, double ns, double nall,
                        mdp_work *w)
{
    *w = mdp_work{};
    // per c value (the direct plan's tables; zero on the generic path, which
    // has none): Z rows, var-column pressures, item factors, Q sums
    if (!(cmax >= 0.0)) cmax = 1.0;  // no grid yet: the default [0, 1]
    std::vector<double> large;
    double coef[kZTerms];
    for (uint32_t js = 0; js < eng->nj; ++js) {
        z_split(eng, js, cmax, large, coef);
        // fma(-c, s, 1) and one multiply per explicit column; the small
        // columns' series: kZTerms FMAs, a multiply, the exp (counted 1)
        w->z_c += 3.0 * (double)large.size() + (coef[0] != 0.0 ? 2.0 * kZTerms + 2.0 : 0.0);
        w->pc_c += (double)eng->nvar;  // pC = c S[j][b] per var column
    }
    const uint32_t vmask = eng->nvar >= 32 ? ~0u : (1u << eng->nvar) - 1u;
    for (uint32_t i = 0; i < eng->nitems; ++i) {
        const uint32_t j = eng->cj_bits[eng->itemRow[i]], B = eng->itemB[i];
        const uint32_t free = (uint32_t)__builtin_popcount(~j & vmask);
        // 1 - pC where B_b = 0, one multiply per free column (the last one by Z)
        w->item_c += (double)__builtin_popcount(~B & ~j & vmask) + (double)free;
    }
    for (size_t q = 0; q + 1 < eng->qstart.size(); ++q) {
        const uint32_t len = eng->qstart[q + 1] - eng->qstart[q];
        if (len > 1) w->q_c += (double)(len - 1);
    }
    // per grid point: the weight table, every use's (nX+1)-term dot product
    // and its multiply-add into the state vector, the final prior sum
    std::vector<int> wmax(kMaxDeg + 1, -1);
    const std::vector<uint32_t> &ud = eng->udesc_d.empty() ? eng->udesc : eng->udesc_d;
    std::set<uint32_t> distinct;  // one descriptor = one transition value P(e, c)
    for (uint32_t d : ud) {
        const uint32_t nX = (d >> kOffBits) & 31u, nA = d >> 27;
        wmax[nA] = std::max(wmax[nA], (int)nX);
        w->use_pt += 2.0 * nX + 3.0;
        if (distinct.insert(d).second) w->use_pt_min += 2.0 * nX + 1.0;  // the dot product, once
    }
    // the state updates v'[l] = sum_k v[k] P[k][l]: npc (2 npp - 1) per year
    for (uint32_t t = 1; t < eng->tmax; ++t) w->use_pt_min += (double)eng->np[t] * (2.0 * eng->np[t - 1] - 1.0);
    w->weight_pt = 2.0 * eng->maxA;
    for (int a = 0; a <= kMaxDeg; ++a)
        if (wmax[a] >= 0) w->weight_pt += (double)(wmax[a] + 1);
    w->final_pt = 2.0 * eng->np[eng->tmax - 1] - 1.0;
    const double per_c = w->z_c + w->pc_c + w->item_c + w->q_c;
    const double per_pt = w->weight_pt + w->use_pt + w->final_pt;
    w->flop = (double)nc * per_c + (double)ne * (double)nc * per_pt;
    w->flop_min_direct = (double)nc * per_c + (double)ne * (double)nc * (w->weight_pt + w->use_pt_min + w->final_pt);
    // the ratio forms (ABI 8): per form from the plan, then the mean over the
    // current grid's e rows (half s-form before a grid is set)
    MdpJitPlan pl;
    pl.np = eng->np;
    pl.udesc = ud;
    const MdpRatioWork rw = mdp_jit_ratio_work(pl);
    const double fs = nall > 0.0 ? ns / nall : 0.5;
    w->setup_pt = fs * rw.setup_s + (1.0 - fs) * rw.setup_t;
    w->use_pt_ratio = fs * rw.use_s + (1.0 - fs) * rw.use_t;
    w->final_pt_ratio = rw.final_pt;
    w->pt_min = w->setup_pt + w->use_pt_ratio + w->final_pt_ratio;
    w->flop_min = (double)nc * per_c + (double)ne * (double)nc * w->pt_min;
}
