// midaspom_amd/csrc/plan_check.cpp -- the engine's host planner over one
// problem, without a device or the HIP runtime:
//   plan_check OBSFILE M D "OPTIONS"
// loads the observations (prior 0.5), parses the engine options, plans with
// the 160 KiB LDS of gfx950 and generates the forward sources the plan would
// compile (hipRTC is never called).  One line: the path taken, the counts of
// the MDP_JIT_CHECK message, and an FNV-1a digest of every plan table and
// generated source.  Exit 0, or mdp_last_error() on stderr and exit 1.
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
        for (MdpJitPlan c : e->chunks) mix(mdp_jit_forward_source(c));
    } else if (e->jit) {
        mix(jit_source(e, 0)), mix(jit_source(e, 1));
    }
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
    if (argc != 5) {
        fprintf(stderr, "usage: plan_check OBSFILE M D \"OPTIONS\"\n");
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
    if (parse_engine_opts(argv[4], eng->opts, false)) return fail();
    if (mdp_plan_engine(eng.get(), &prob, 160 * 1024, MdpPlanMode::TablesOnly, nullptr)) return fail();
    digest(eng.get());
    const MdpJitPlan &pl = eng->jit_plan;
    printf("path %s | nj %u nitems %u ldQ %zu nqi %u qmaxlen %u kzmax %u slots %u conflicts %u + %u | digest %016llx\n",
           path_of(eng.get()).c_str(), eng->nj, eng->nitems, eng->ldQ, pl.nqi, pl.qmaxlen, pl.kzmax, eng->npl_slots,
           eng->slot_conflicts, eng->slot_store_conflicts, (unsigned long long)g_h);
    return 0;
}
