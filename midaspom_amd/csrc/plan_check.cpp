// midaspom_amd/csrc/plan_check.cpp -- the engine's host planner over one
// problem, without a device or the HIP runtime:
//   plan_check [--diag] [--sources] OBSFILE M D "OPTIONS"
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
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "spom_engine.h"

namespace {

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

// every plan vector of mdp_engine in declaration order, then the sources
void digest(mdp_engine *e)
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
    } else if (e->jit) {
        for (int variant = 0; variant < 2; ++variant) {
            const std::string src = jit_source(e, variant);
            source(variant ? "fused" : "reading", src, e->jit_flops_pt);
        }
    }
}

// The tall variant's source, after the digest (which it is no part of).
// jit_source reports no flop count for it, so the same plan goes through the
// generator once more for the count; the two texts must agree.
int tall_source(mdp_engine *e)
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

std::string path_of(const mdp_engine *e)
{
    char b[64];
    if (e->wide) {
        if (e->hs) snprintf(b, sizeof b, "wide-hs<%u,%u,%u>", e->hs_rt, e->hs_nb, e->hs_nw);
        else if (e->mmt) snprintf(b, sizeof b, "wide-mmt<%u,%u,%s>", e->mmt_rt, e->mmt_rows, mmt_shape(e).db ? "2buf" : "1buf");
        else if (e->mma) snprintf(b, sizeof b, "wide-mma<%u>", e->mma_npm);
        else snprintf(b, sizeof b, "wide-plain");
        return b;
    }
    if (!e->jit) return "generic";
    if (!e->chunks.empty()) {
        snprintf(b, sizeof b, "chunked<%zu%s>", e->chunks.size(), e->chunks[0].qidx.empty() ? "" : ",gathered");
        return std::string(e->jit_plan.vlds ? "vlds " : "direct ") + b + (e->qglobal ? " qglobal" : "");
    }
    if (e->jit_plan.vlds) return "vlds";
    const bool fused = !e->qglobal && fused_lds(e, e->jit_plan.ct_max) <= kFusedLdsMax;
    return std::string("direct") + (fused ? " fused-capable" : "") + (e->qglobal ? " qglobal" : "");
}

}  // namespace

int main(int argc, char **argv)
{
    bool diag = false;
    for (; argc > 1 && argv[1][0] == '-' && argv[1][1] == '-'; --argc, ++argv) {
        const std::string flag = argv[1];
        if (flag == "--diag") diag = true;
        else if (flag == "--sources") g_sources = true;
        else argc = 0;
    }
    if (argc != 5) {
        fprintf(stderr, "usage: plan_check [--diag] [--sources] OBSFILE M D \"OPTIONS\"\n");
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
    auto eng = std::make_unique<mdp_engine>();
    if (parse_engine_opts(argv[4], eng->opts, diag)) return fail();
    if (mdp_plan_engine(eng.get(), &prob, 160 * 1024, MdpPlanMode::TablesOnly, nullptr)) return fail();
    digest(eng.get());
    const MdpJitPlan &pl = eng->jit_plan;
    printf("path %s | nj %u nitems %u ldQ %zu nqi %u qmaxlen %u kzmax %u slots %u conflicts %u + %u | digest %016llx\n",
           path_of(eng.get()).c_str(), eng->nj, eng->nitems, eng->ldQ, pl.nqi, pl.qmaxlen, pl.kzmax, eng->npl_slots,
           eng->slot_conflicts, eng->slot_store_conflicts, (unsigned long long)g_h);
    if (g_sources && eng->jit && !eng->wide && eng->chunks.empty() && !pl.vlds && tall_source(eng.get())) return 1;
    fputs(g_src_lines.c_str(), stdout);
    return 0;
}
