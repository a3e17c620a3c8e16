// midaspom_amd/csrc/plan_check.cpp -- the engine's host planner over one
// problem, without a device or the HIP runtime:
//   plan_check [--diag] [--sources] [--grid NE NC NCU [--e LO HI] [--c LO HI]
//              [--cbound B] [--list] [--ztables]] OBSFILE M D "OPTIONS"
// loads the observations (prior 0.5), parses the engine options, plans with
// the 160 KiB LDS of gfx950 and generates the forward sources the plan would
// compile (hipRTC is never called).  One line: the path taken, the counts of
// the MDP_JIT_CHECK message, and an FNV-1a digest of every plan table and
// generated source.  Exit 0, or mdp_last_error() on stderr and exit 1.
// --diag accepts the measurement-only option names (MDP_DIAG, MDP_JIT_HACK,
// MDP_JIT_WPE: the sources of libmidaspom_diag.so).  --sources adds one line
// per generated source,
//   src <name> bytes <n> fnv <16 hex> flops_pt <%.17g>
// named reading, fused and tall (the reading kernel at kJitKblockTall
// threads, of direct plans that are neither chunked nor vlds), or chunk<i>:
// two generators print the same lines exactly when they emit the same text.
// --grid plans one grid as mdp_engine_set_grid would on a device of NCU
// compute units (mdp_plan_grid; no device is asked): NE e values from LO to HI
// (mdp_grid; 0 to 1 unless given, descending where LO > HI) by NC c values
// (the same), under the |c| bound B if given.  After the summary line,
//   grid <fused|reading|tall|-> | gy nlist epl identity ne_sform | qrows_cb
//        wide_cb_items wide_cb_fwd | kmax ct_len zrows_lds | launch ... | buf ...
//        | kernels <the names a run notes for mdp_engine_launched, ';' between> | fnv ...
// with FNV-1a digests of the point list, its e values and each c table; a
// refused grid is mdp_last_error() on stderr and exit 1.  --list adds the
// point list itself (plist v v ...; bit 31 marks a padding duplicate).
// --ztables adds the grid's Z-row tables (MdpCTables, z_split) after those:
//   ztables nj <rows> kmax <kmax> cmax <%a>
// and one line per row,
//   zrow <row> bits <hidden state> nl <explicit columns> zs <patch>:<S %a> ...
//        | zsq <%a> ... | zc <%a> x 8
// zs: the row's kmax stored slots in order (the explicit "large" columns, the
// largest S first, then the padding, patch "-"), zsq: k_qrows' chain-major copy
// of the same slots, zc: the series coefficients P_i / i of the small columns.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "spom_engine.h"

#ifndef MDP_ENGINE_PLAN  // a planner from before the plan / engine split (scripts/jit_sources.py --rev)
using MdpEnginePlan = mdp_engine;
#endif

namespace {

// does the plan run the specialised forward kernel (a direct path)?
bool direct(const MdpEnginePlan *e)
{
#ifdef MDP_PLAN_PATH
    return path_is_jit(e->path);
#else  // a planner from before MdpPath (scripts/jit_sources.py --rev): its flags
    return e->jit && !e->wide;
#endif
}

uint64_t g_h = 0xcbf29ce484222325ull;  // FNV-1a, 64 bit

void mix(const void *p, size_t n)
{
    for (size_t i = 0; i < n; ++i) g_h = (g_h ^ ((const unsigned char *)p)[i]) * 0x100000001b3ull;
}
template <typename T>
void mix(const std::vector<T> &v)
{
    const uint64_t n = v.size();
    mix(&n, sizeof n);
    mix(v.data(), v.size() * sizeof(T));
}
void mix(const std::string &s) { mix(s.data(), s.size() + 1); }

bool g_sources = false;
std::string g_src_lines;  // printed after the summary line

void source(const char *name, const std::string &src, double flops_pt)
{
    mix(src);
    if (!g_sources) return;
    uint64_t h = 0xcbf29ce484222325ull;
    for (unsigned char c : src) h = (h ^ c) * 0x100000001b3ull;
    char b[160];
    snprintf(b, sizeof b, "src %s bytes %zu fnv %016llx flops_pt %.17g\n", name, src.size(), (unsigned long long)h, flops_pt);
    g_src_lines += b;
}

// every plan vector of MdpEnginePlan in declaration order, then the sources
void digest(MdpEnginePlan *e)
{
    for (MdpJitPlan &c : e->chunks) {
        mix(c.np), mix(c.udesc), mix(c.qidx);
    }
    mix(e->jit_plan.np), mix(e->jit_plan.udesc);
    mix(e->cj_bits), mix(e->cj_item0), mix(e->itemB), mix(e->qstart), mix(e->qitem), mix(e->udesc_d), mix(e->var_cols);
    mix(e->itemRow), mix(e->qslot), mix(e->qlane), mix(e->islot);
    mix(e->mma_kt), mix(e->mma_wplan), mix(e->mma_kbase), mix(e->mma_desc), mix(e->mma_dbase);
    mix(e->mmt_kt), mix(e->mmt_ktile), mix(e->mmt_wplan), mix(e->mmt_cidx);
    mix(e->hs_kt), mix(e->hs_cidx), mix(e->hs_pbase), mix(e->hs_dpos), mix(e->hs_dbase), mix(e->hs_pk);
    mix(e->hs_ppos), mix(e->hs_dpk), mix(e->hs_wplan), mix(e->hs_pass);
    mix(e->ystate), mix(e->isvar), mix(e->Sj);
    mix(e->np), mix(e->pairA), mix(e->pairB), mix(e->pairOff), mix(e->use_pair), mix(e->prog), mix(e->udesc);
    mix(e->pairPart0), mix(e->partP), mix(e->partK0);
    if (!e->chunks.empty()) {
        size_t i = 0;
        for (MdpJitPlan c : e->chunks) {
            const std::string src = mdp_jit_forward_source(c);
            source(("chunk" + std::to_string(i++)).c_str(), src, c.flops_pt);
        }
    } else if (direct(e)) {
        for (int variant = 0; variant < 2; ++variant) {
            const std::string src = jit_source(e, variant);
            source(variant ? "fused" : "reading", src, e->jit_flops_pt);
        }
    }
}

// The tall variant's source, after the digest (which it is no part of).
// jit_source reports no flop count for it, so the same plan goes through the
// generator once more for the count; the two texts must agree.
int tall_source(MdpEnginePlan *e)
{
    const uint64_t h = g_h;
    const std::string src = jit_source(e, 2);
    MdpJitPlan p = e->jit_plan;
    p.fused = false;
    p.epl = e->jit_epl;
    p.kblock = kJitKblockTall;
    if (mdp_jit_forward_source(p) != src) {
        fprintf(stderr, "plan_check: the tall source differs from its plan's\n");
        return 1;
    }
    source("tall", src, p.flops_pt);
    g_h = h;
    return 0;
}

std::string path_of(const MdpEnginePlan *e)
{
    char b[64];
#ifdef MDP_PLAN_PATH
    switch (e->path) {
    case MdpPath::Generic: return "generic";
    case MdpPath::Direct:
    case MdpPath::DirectQGlobal: break;
    case MdpPath::WideHs: snprintf(b, sizeof b, "wide-hs<%u,%u,%u>", e->hs_rt, e->hs_nb, e->hs_nw); return b;
    case MdpPath::WideMmt:
        snprintf(b, sizeof b, "wide-mmt<%u,%u,%s>", e->mmt_rt, e->mmt_rows, mmt_shape(e).db ? "2buf" : "1buf");
        return b;
    case MdpPath::WideMma: snprintf(b, sizeof b, "wide-mma<%u>", e->mma_npm); return b;
    case MdpPath::WidePlain: return "wide-plain";
    }
    const bool qglobal = e->path == MdpPath::DirectQGlobal;
#else  // a planner from before MdpPath (scripts/jit_sources.py --rev): its flags
    if (e->wide) {
        if (e->hs) snprintf(b, sizeof b, "wide-hs<%u,%u,%u>", e->hs_rt, e->hs_nb, e->hs_nw);
        else if (e->mmt) snprintf(b, sizeof b, "wide-mmt<%u,%u,%s>", e->mmt_rt, e->mmt_rows, mmt_shape(e).db ? "2buf" : "1buf");
        else if (e->mma) snprintf(b, sizeof b, "wide-mma<%u>", e->mma_npm);
        else snprintf(b, sizeof b, "wide-plain");
        return b;
    }
    if (!e->jit) return "generic";
    const bool qglobal = e->qglobal;
#endif
    if (!e->chunks.empty()) {
        snprintf(b, sizeof b, "chunked<%zu%s>", e->chunks.size(), e->chunks[0].qidx.empty() ? "" : ",gathered");
        return std::string(e->jit_plan.vlds ? "vlds " : "direct ") + b + (qglobal ? " qglobal" : "");
    }
    if (e->jit_plan.vlds) return "vlds";
#ifdef MDP_PLAN_GRID
    const bool fused = mdp_plan_fused_capable(e);
#else  // a planner from before mdp_plan_grid (scripts/jit_sources.py --rev)
    const bool fused = !qglobal && fused_lds(e, e->jit_plan.ct_max) <= kFusedLdsMax;
#endif
    return std::string("direct") + (fused ? " fused-capable" : "") + (qglobal ? " qglobal" : "");
}

template <typename T>
unsigned long long fnv(const std::vector<T> &v)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) h = (h ^ ((const unsigned char *)v.data())[i]) * 0x100000001b3ull;
    return h;
}

struct GridArgs {
    bool on = false, list = false, ztables = false;
    uint32_t ne = 0, nc = 0, ncu = 0;
    double e[2] = {0.0, 1.0}, c[2] = {0.0, 1.0}, cbound = 0.0;
};

#ifdef MDP_PLAN_GRID
// the --grid mode: plan the grid and print its line (after digest(): the
// generator has settled the forward shapes)
int grid_line(MdpEnginePlan *eng, const GridArgs &a)
{
    if (!eng->chunks.empty()) {  // the chunks' shape, as jit_build_chunks takes it from the generator
        MdpJitPlan c0 = eng->chunks[0];
        (void)mdp_jit_forward_source(c0);
        eng->jit_epl = c0.epl;
        eng->jit_kblock = (uint32_t)c0.kblock;
    }
    eng->cbound = a.cbound;
    std::vector<double> e(a.ne), c(a.nc);
    mdp_grid(a.ne, a.e[0], a.e[1], e.data());
    mdp_grid(a.nc, a.c[0], a.c[1], c.data());
    MdpCTables ct;
    MdpGridPlan g;
    if (mdp_plan_grid(eng, ct, e.data(), a.ne, c.data(), a.nc, a.ncu, g)) return 1;
    const bool jit = direct(eng);
    if (jit) mdp_plan_fwd_launch(eng, ct, a.ne, a.nc, g);
    std::string kernels;
    for (const std::string &k : mdp_plan_grid_kernels(eng, g, a.ne, a.nc)) kernels += (kernels.empty() ? "" : ";") + k;
    printf("grid %s | gy %u nlist %u epl %u identity %d ne_sform %u | qrows_cb %u wide_cb_items %u wide_cb_fwd %u | "
           "kmax %u ct_len %u zrows_lds %zu | launch nblk %llu threads %llu pro %u block %u lds %u nlist %u listed %d | "
           "buf qrow %zu zg %zu pg %zu pg_zero %d v %zu vscr %zu ldv %u zpv %zu r %zu gpart %zu stamps %zu,%zu,%zu | "
           "kernels %s | fnv plist %016llx elist %016llx zs %016llx zsq %016llx zc %016llx coltab %016llx\n",
           !jit ? "-" : g.fused ? "fused" : g.tall ? "tall" : "reading", g.gy, g.nlist, g.nlist_epl, (int)g.plist_identity,
           g.ne_sform, g.qrows_cb, g.wide_cb_items, g.wide_cb_fwd, ct.kmax, ct.ct_len, g.zrows_lds,
           (unsigned long long)g.fwd_nblk, (unsigned long long)g.fwd_threads, g.fwd_pro, g.fwd_block, g.fwd_lds, g.fwd_nlist,
           (int)g.fwd_listed, g.n_qrow, g.n_zg, g.n_pg, (int)g.pg_zero, g.n_v, g.n_vscr, g.ldv, g.n_zpv, g.n_r, g.n_gpart,
           g.nst[0], g.nst[1], g.nst[2], kernels.empty() ? "-" : kernels.c_str(), fnv(g.plist), fnv(g.elist), fnv(ct.zs),
           fnv(ct.zsq), fnv(ct.zc), fnv(ct.coltab));
    if (a.list) {
        printf("plist");
        for (uint32_t v : g.plist) printf(" %u", v);
        printf("\n");
    }
    if (a.ztables) {
        const uint32_t nrows = ct.zc.empty() ? 0u : eng->nj;  // (the generic path builds no c tables)
        printf("ztables nj %u kmax %u cmax %a\n", nrows, ct.kmax, ct.cmax);
        std::vector<double> large;
        std::vector<uint32_t> cols;
        for (uint32_t js = 0; js < nrows; ++js) {
            z_split(eng, js, ct.cmax, large, nullptr, &cols);  // (the patch of each stored column)
            printf("zrow %u bits %u nl %zu zs", js, eng->cj_bits[js], large.size());
            for (uint32_t k = 0; k < ct.kmax; ++k) {
                if (k < cols.size()) printf(" %u:%a", cols[k], ct.zs[(size_t)js * ct.kmax + k]);
                else printf(" -:%a", ct.zs[(size_t)js * ct.kmax + k]);
            }
            printf(" | zsq");
            for (uint32_t k = 0; k < ct.kmax; ++k) printf(" %a", ct.zsq[(size_t)js * ct.kmax + k]);
            printf(" | zc");
            for (int i = 0; i < kZTerms; ++i) printf(" %a", ct.zc[(size_t)js * kZTerms + i]);
            printf("\n");
        }
    }
    return 0;
}

#else
int grid_line(MdpEnginePlan *, const GridArgs &)
{
    fprintf(stderr, "plan_check: this planner plans no grid\n");
    return 2;
}
#endif

}  // namespace

int main(int argc, char **argv)
{
    bool diag = false;
    GridArgs grid;
    for (; argc > 1 && argv[1][0] == '-' && argv[1][1] == '-'; --argc, ++argv) {
        const std::string flag = argv[1];
        // a flag's values follow it (a value may be negative, so none is taken for a flag)
        auto values = [&](int n, double *v) {
            if (argc < 2 + n) return argc = 0, false;
            for (int i = 0; i < n; ++i) v[i] = atof(argv[2 + i]);
            argc -= n, argv += n;
            return true;
        };
        double v[3];
        if (flag == "--diag") diag = true;
        else if (flag == "--sources") g_sources = true;
        else if (flag == "--list") grid.list = true;
        else if (flag == "--ztables") grid.ztables = true;
        else if (flag == "--grid" && values(3, v)) grid.on = true, grid.ne = (uint32_t)v[0], grid.nc = (uint32_t)v[1], grid.ncu = (uint32_t)v[2];
        else if (flag == "--e" && values(2, grid.e)) continue;
        else if (flag == "--c" && values(2, grid.c)) continue;
        else if (flag == "--cbound" && values(1, &grid.cbound)) continue;
        else argc = 0;
    }
    if (argc != 5) {
        fprintf(stderr, "usage: plan_check [--diag] [--sources] [--grid NE NC NCU [--e LO HI] [--c LO HI] [--cbound B] "
                        "[--list] [--ztables]] OBSFILE M D \"OPTIONS\"\n");
        return 2;
    }
    auto fail = []() {
        fprintf(stderr, "plan_check: %s\n", mdp_last_error());
        return 1;
    };
    mdp_model *model = nullptr;
    if (mdp_model_load(argv[1], atof(argv[2]), 0.5f, atof(argv[3]), &model)) return fail();
    std::unique_ptr<mdp_model, void (*)(mdp_model *)> model_owner(model, mdp_model_free);
    mdp_problem prob;
    if (mdp_model_problem(model, &prob)) return fail();
    auto eng = std::make_unique<MdpEnginePlan>();
    if (parse_engine_opts(argv[4], eng->opts, diag)) return fail();
    if (mdp_plan_engine(eng.get(), &prob, 160 * 1024, MdpPlanMode::TablesOnly, nullptr)) return fail();
    digest(eng.get());
    const MdpJitPlan &pl = eng->jit_plan;
    printf("path %s | nj %u nitems %u ldQ %zu nqi %u qmaxlen %u kzmax %u slots %u conflicts %u + %u | digest %016llx\n",
           path_of(eng.get()).c_str(), eng->nj, eng->nitems, eng->ldQ, pl.nqi, pl.qmaxlen, pl.kzmax, eng->npl_slots,
           eng->slot_conflicts, eng->slot_store_conflicts, (unsigned long long)g_h);
    if (g_sources && direct(eng.get()) && eng->chunks.empty() && !pl.vlds && tall_source(eng.get())) return 1;
    fputs(g_src_lines.c_str(), stdout);
    if (grid.on && grid_line(eng.get(), grid)) return fail();
    return 0;
}
