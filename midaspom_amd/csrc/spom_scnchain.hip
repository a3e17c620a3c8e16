// midaspom_amd/csrc/spom_scnchain.hip -- the die-off and habitat-loss
// hypotheses through the chain of occupied-count classes, for first survey
// rows of up to 64 patches.  The reference's authors use it for their
// 26-segment figures (Rscript/simuls_traj.R, simtrajH11 / simtrajH21): one
// simulated year from a random start with exactly k occupied patches, for
// every k, tallied into the (n+1) x (n+1) matrix of class transitions -- A for
// a scenario year, B for a baseline year -- and
//   L = sum_k start[k] [A^ts B^tdis target]_k.
// One year per replicate instead of ts + tdis, and the matrix powers carry
// probabilities far below 1/nrep.  Lumping the 2^n states into n+1 classes is
// exact when the patches are exchangeable and an approximation otherwise
// (DESIGN.md).
//
// One replicate rg = rep0 + r of class k, the same for every grid point but
// for its rates (the counter holds no grid point):
//   start state   selection sampling of exactly k patches: need = k; for
//                 j = 0..n-1, u_j = word j & 3 of philox(seed; rg_lo, rg_hi,
//                 0xfffffffe, 16 k + (j >> 2)); patch j is occupied iff
//                 ((uint64)u_j (n - j)) >> 32 < need, and then need -= 1;
//   the year      sim_year<NM> (spom_sim_year.h) with year word t = k, so the
//                 classes use disjoint draws;
//   rates         scenario table: k_scnsim's Es and (Ks, Km) by kind;
//                 baseline table: E = min(1, e), (ks, km) = (0, 1);
//   tally         cnt[(g (n+1) + k)(n+1) + l] += 1, l the occupied count after
//                 the year.
// Contraction is off.
//
// k_scnchain<NM>: one lane per replicate, a work tile is (point, class, 256
// replicates) with wave-uniform rates.  A point's tiles are cut into runs
// (spom_scnchain_plan.h); a workgroup tallies a run into an LDS matrix of
// (n+1)^2 32-bit counters with LDS integer atomics and flushes its non-zero
// cells once, with global integer atomics: exact, the same for every split.
// k_chain_eval: one workgroup per point, the counts converted to doubles in
// LDS once, transposed (lane k reads At[l][k]: consecutive doubles), then the
// mat-vecs from LDS, one barrier per step; thread k owns class k.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <type_traits>
#include <vector>

#include "spom_dev.h"
#include "spom_scnchain_plan.h"

#pragma clang fp contract(off)

#include "spom_rng.h"
#include "spom_sim_year.h"

namespace {

struct ChainArgs {
    uint32_t n, kind, baseline, nc, nK, nd;
    uint64_t p0;     // first grid point of the launch
    uint64_t units;  // (point, run) pairs of the launch: npts x parts
    uint64_t parts;  // runs per point
    uint64_t tpc;    // tiles per class: ceil(nrep / 256)
    uint64_t tpp;    // tiles per point: (n + 1) tpc, class-major
    uint64_t rep0, nrep;
    uint32_t key0, key1;
};

template <int NM>
__global__ __launch_bounds__(kChainBlock) void k_scnchain(ChainArgs a, const double *__restrict__ M,
                                                          const double *__restrict__ srcv,
                                                          const double *__restrict__ ev, const double *__restrict__ cv,
                                                          const double *__restrict__ Kv,
                                                          uint32_t *__restrict__ tab)  // [npts][n+1][n+1] of the launch
{
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    double *Ts = dyn;  // NM = 8 only
    uint32_t *cnt = reinterpret_cast<uint32_t *>(dyn + (NM == kTabN ? (kTabN << kTabN) : 0));
    if constexpr (NM == kTabN) sim_year_table(a.n, M, Ts, kChainBlock);  // (the barrier: the first unit's)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t npairs = (a.n + 1) >> 1;
    const uint32_t ncl = a.n + 1, cells = ncl * ncl;
    const bool scen = !a.baseline;
    for (uint64_t unit = blockIdx.x; unit < a.units; unit += gridDim.x) {
        // workgroup-uniform: the unit's grid point and its run of tiles
        const uint64_t pl = unit / a.parts, q = unit - pl * a.parts;
        const uint64_t g = a.p0 + pl;
        for (uint32_t i = threadIdx.x; i < cells; i += kChainBlock) cnt[i] = 0;
        __syncthreads();
        double e, c, K = 1.0;
        const double *src = srcv;
        if (scen) {
            const uint32_t id = (uint32_t)(g % a.nd), iK = (uint32_t)((g / a.nd) % a.nK);
            const uint32_t ic = (uint32_t)((g / ((uint64_t)a.nd * a.nK)) % a.nc);
            const uint32_t ie = (uint32_t)(g / ((uint64_t)a.nd * a.nK * a.nc));
            e = ev[ie], c = cv[ic], K = Kv[iK];
            if (a.kind) src = srcv + (size_t)id * NM;
        } else {
            e = ev[g / a.nc], c = cv[g % a.nc];
        }
        double E = scen && !a.kind ? e / K : e;  // dieoff.c:56-57; baseline and loss: E = e (loss.c:57)
        if (E > 1) E = 1;
        const double ks = scen && a.kind ? K : 0.0, km = scen && !a.kind ? K : 1.0;
        const uint64_t t0 = a.tpp * q / a.parts, t1 = a.tpp * (q + 1) / a.parts;
        for (uint64_t tile = t0; tile < t1; ++tile) {
            // workgroup-uniform: the class; wave-uniform: the replicates
            const uint32_t k = (uint32_t)(tile / a.tpc);
            const uint64_t rb = (tile - k * a.tpc) * kChainBlock + (threadIdx.x & ~63u);
            if (rb >= a.nrep) continue;  // a wave past the last replicate
            const uint64_t r = rb + lane, rg = a.rep0 + r;
            if (r >= a.nrep) continue;
            // ---- start state: exactly k patches by selection sampling
            uint64_t occ = 0;
            uint32_t need = k;
            for (uint32_t j4 = 0; j4 < a.n && need; j4 += 4) {
                const u32x4 w = philox(a.key0, a.key1,
                                       u32x4{(uint32_t)rg, (uint32_t)(rg >> 32), 0xfffffffeu, 16u * k + (j4 >> 2)});
                const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                for (uint32_t i = 0; i < 4; ++i) {
                    const uint32_t j = j4 + i;
                    if (j < a.n && (uint32_t)(((uint64_t)u[i] * (a.n - j)) >> 32) < need) {
                        occ |= 1ull << j;
                        --need;
                    }
                }
            }
            // ---- one year.  Class 0 without a source: every sum is 0,
            // pC = c*0, and no draw is below 0
            if (k != 0 || (a.kind && scen)) occ = sim_year<NM>(a, M, src, Ts, rg, k, npairs, occ, E, c, ks, km);
            atomicAdd(&cnt[k * ncl + (uint32_t)__popcll(occ)], 1u);
        }
        __syncthreads();
        uint32_t *out = tab + pl * cells;
        for (uint32_t i = threadIdx.x; i < cells; i += kChainBlock) {
            const uint32_t v = cnt[i];
            if (v) atomicAdd(&out[i], v);
        }
        __syncthreads();  // (the next unit clears cnt)
    }
}

struct EvalArgs {
    uint32_t ncl;     // n + 1
    uint32_t steps;   // mat-vecs
    uint64_t p0;      // first grid point of the launch (tab is the launch's, v0 / vout / out the call's)
    uint64_t v0_div;  // the start vector of point g is row g / v0_div of v0 (0: row 0)
    double den;       // replicates per class of the table
};

// v <- (tab / den)^steps v0, vout[g][k] = v[k] (may be NULL), out[g] = sum_k
// start[k] v[k] ascending (may be NULL)
__global__ __launch_bounds__(kChainEvalBlock) void k_chain_eval(EvalArgs a, const uint32_t *__restrict__ tab,
                                                                const double *__restrict__ v0,
                                                                const double *__restrict__ start,
                                                                double *__restrict__ vout, double *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    const uint32_t ncl = a.ncl, k = threadIdx.x;
    double *At = dyn;            // At[l][k] = tab[k][l] / den
    double *v = dyn + ncl * ncl;  // two vectors of ncl
    const uint64_t pl = blockIdx.x, g = a.p0 + pl;
    if (a.steps) {
        const uint32_t *cnt = tab + pl * ncl * ncl;
        for (uint32_t i = threadIdx.x; i < ncl * ncl; i += kChainEvalBlock) {
            const uint32_t kk = i / ncl, l = i - kk * ncl;
            At[l * ncl + kk] = (double)cnt[i] / a.den;
        }
    }
    const double *vs = v0 + (a.v0_div ? g / a.v0_div : 0) * ncl;
    if (k < ncl) v[k] = vs[k];
    __syncthreads();
    uint32_t cur = 0;
    for (uint32_t t = 0; t < a.steps; ++t) {
        if (k < ncl) {
            const double *x = v + cur * ncl;
            double s = 0.0;
            for (uint32_t l = 0; l < ncl; ++l) s += At[l * ncl + k] * x[l];
            v[(cur ^ 1u) * ncl + k] = s;
        }
        __syncthreads();
        cur ^= 1u;
    }
    const double *x = v + cur * ncl;
    if (vout && k < ncl) vout[g * ncl + k] = x[k];
    if (out && k == 0) {
        double s = 0.0;
        for (uint32_t l = 0; l < ncl; ++l) s += start[l] * x[l];
        out[g] = s;
    }
}

}  // namespace

// (DevQueue: the device, stream and events, released after the buffers below)
struct mdp_scenario_chain : DevQueue {
    ChainPlan plan;
    char kname[32] = "";
    DevBuf<double> dM, dgrid;  // dgrid: [e | c | K | src[nd][nm] | zero row[nm]]
    DevBuf<double> dw;         // [start | target]
    DevBuf<uint32_t> dtab;     // the count table of one launch
    DevBuf<double> dvbase, dbyclass, dout;
    ~mdp_scenario_chain() { drain(); }  // (never opened: nothing below exists, no HIP call)
};

namespace {

// the device side of an engine, set up by the first call that needs it: the
// device, stream and events, then the table, uploaded once
int chain_device(mdp_scenario_chain *s)
{
    if (int rc = s->open()) return rc;
    return s->dM.empty() ? s->dM.assign(s->plan.M) : MDP_OK;
}

struct ChainGrid {
    const double *e, *c, *K, *dsrc;
    uint32_t ne, nc, nK, nd;  // nK = 0: no scenario axes (a baseline table alone)
};

// The axes and the source rows into s->dgrid, after every device form still
// pending has been waited for (spom_dev.h, the stream rule): the copy is
// synchronous on the null stream, which nothing orders against a caller's
// non-blocking stream.
int chain_upload(mdp_scenario_chain *s, const ChainGrid &gr)
{
    std::vector<double> src;
    chain_src(s->plan, gr.nK == 0, gr.dsrc, gr.nd, &src);
    std::vector<double> h;
    h.insert(h.end(), gr.e, gr.e + gr.ne);
    h.insert(h.end(), gr.c, gr.c + gr.nc);
    if (gr.nK) h.insert(h.end(), gr.K, gr.K + gr.nK);
    h.insert(h.end(), src.begin(), src.end());
    h.resize(h.size() + s->plan.nm, 0.0);
    if (int rc = s->settle()) return rc;
    return s->dgrid.assign(h);
}

// the count table of a call's largest launch, cleared launch by launch
size_t chain_tab_cells(const ChainPlan &p, const ChainCall &call)
{
    uint64_t npts = 0;
    for (const ChainLaunch &l : call.launches) npts = std::max(npts, l.npts);
    return (size_t)(npts * (p.n + 1) * (p.n + 1));
}

size_t chain_counts_lds(const ChainPlan &p)
{
    return (p.nm == (uint32_t)kTabN ? sizeof(double) * (kTabN << kTabN) : 0) + sizeof(uint32_t) * (p.n + 1) * (p.n + 1);
}

// one launch of a counting call on st: the table cleared, then counted
int chain_count_launch(mdp_scenario_chain *s, const ChainCall &call, const ChainLaunch &l, bool baseline,
                       const ChainGrid &gr, uint64_t seed, uint64_t rep0, uint64_t nrep, hipStream_t st)
{
    const ChainPlan &p = s->plan;
    const size_t cells = (size_t)(p.n + 1) * (p.n + 1);
    const double *de = s->dgrid.get(), *dc = de + gr.ne, *dK = dc + gr.nc, *dsrc = dK + gr.nK;
    const uint32_t nsrc = gr.nK && p.kind == 1 ? gr.nd : 1u;  // chain_src's rows, before the zero row
    const double *dzero = dsrc + (size_t)nsrc * p.nm;
    ChainArgs a{};
    a.n = p.n;
    a.kind = (uint32_t)p.kind;
    a.baseline = baseline;
    a.nc = gr.nc;
    a.nK = baseline ? 1u : gr.nK;
    a.nd = baseline ? 1u : gr.nd;
    a.p0 = l.p0;
    a.units = l.units;
    a.parts = l.parts;
    a.tpc = call.tiles_per_class;
    a.tpp = call.tiles_per_point;
    a.rep0 = rep0;
    a.nrep = nrep;
    a.key0 = (uint32_t)seed;
    a.key1 = (uint32_t)(seed >> 32);
    HIP_TRY(hipMemsetAsync(s->dtab.get(), 0, l.npts * cells * sizeof(uint32_t), st));
    const size_t lds = chain_counts_lds(p);
    if (int rc = dev_for_padded(p.nm, [&](auto NM) {
            hipLaunchKernelGGL(k_scnchain<decltype(NM)::value>, dim3(l.nwg), dim3(kChainBlock), lds, st, a, s->dM.get(),
                               baseline ? dzero : dsrc, de, dc, dK, s->dtab.get());
            return MDP_OK;
        }))
        return rc;
    HIP_TRY(hipGetLastError());
    return MDP_OK;
}

// the evaluation of one launch's points on st, from the table the launch left
int chain_eval_launch(mdp_scenario_chain *s, const ChainLaunch &l, uint32_t steps, uint64_t den, const double *v0,
                      uint64_t v0_div, double *vout, double *out, hipStream_t st)
{
    const uint32_t ncl = s->plan.n + 1;
    EvalArgs a{};
    a.ncl = ncl;
    a.steps = steps;
    a.p0 = l.p0;
    a.v0_div = v0_div;
    a.den = (double)den;
    const size_t lds = sizeof(double) * ((size_t)ncl * ncl + 2 * ncl);  // <= 34.8 KB
    hipLaunchKernelGGL(k_chain_eval, dim3((uint32_t)l.npts), dim3(kChainEvalBlock), lds, st, a, s->dtab.get(), v0,
                       s->dw.get(), vout, out);
    HIP_TRY(hipGetLastError());
    return MDP_OK;
}

struct ChainJob {
    int ts, tdis;
    ChainGrid gr;
    uint64_t seed, nrep, nbase;
    ChainCall scn, base;
};

// the refusals of _lik, _lik_device and _time_kernels
int chain_job(const ChainPlan &p, int ts, int tdis, const double *e, uint32_t ne, const double *c, uint32_t nc,
              const double *K, uint32_t nK, const double *dsrc, uint32_t nd, uint64_t seed, uint64_t nrep,
              uint64_t nbase, const double *start, const double *target, ChainJob *job)
{
    if (int rc = chain_eval_check(p, ts, tdis, nrep, nbase, start, target)) return rc;
    if (int rc = chain_call(p, false, e, ne, c, nc, K, nK, dsrc, nd, nrep, false, &job->scn)) return rc;
    if (int rc = chain_call(p, true, e, ne, c, nc, K, nK, dsrc, nd, nbase, false, &job->base)) return rc;
    job->ts = ts, job->tdis = tdis;
    job->gr = ChainGrid{e, c, K, dsrc, ne, nc, nK, nd};
    job->seed = seed, job->nrep = nrep, job->nbase = nbase;
    return MDP_OK;
}

// the device side of a job: the grid, the weights, the buffers (every pending
// device form waited for first)
int chain_prepare(mdp_scenario_chain *s, const ChainJob &job, const double *start, const double *target,
                  bool want_by_class, bool want_out)
{
    const ChainPlan &p = s->plan;
    const uint32_t ncl = p.n + 1;
    if (int rc = chain_upload(s, job.gr)) return rc;
    std::vector<double> ws, wt;
    chain_weights(p, start, target, &ws, &wt);
    ws.insert(ws.end(), wt.begin(), wt.end());
    if (int rc = s->dw.assign(ws)) return rc;
    if (int rc = s->dtab.grow(std::max(chain_tab_cells(p, job.scn), chain_tab_cells(p, job.base)))) return rc;
    if (int rc = s->dvbase.grow((size_t)job.base.G * ncl)) return rc;
    if (want_by_class)
        if (int rc = s->dbyclass.grow((size_t)job.scn.G * ncl)) return rc;
    if (want_out)
        if (int rc = s->dout.grow((size_t)job.scn.G)) return rc;
    return MDP_OK;
}

// every launch of a job on st: the baseline pass leaves v = B^tdis target per
// (e, c) in dvbase, the scenario pass starts from it
int chain_run(mdp_scenario_chain *s, const ChainJob &job, double *d_by_class, double *d_out, hipStream_t st)
{
    const uint32_t ncl = s->plan.n + 1;
    const double *dtarget = s->dw.get() + ncl;
    for (const ChainLaunch &l : job.base.launches) {
        if (job.tdis)
            if (int rc = chain_count_launch(s, job.base, l, true, job.gr, job.seed, 0, job.nbase, st)) return rc;
        if (int rc = chain_eval_launch(s, l, (uint32_t)job.tdis, job.nbase, dtarget, 0, s->dvbase.get(), nullptr, st))
            return rc;
    }
    for (const ChainLaunch &l : job.scn.launches) {
        if (job.ts)
            if (int rc = chain_count_launch(s, job.scn, l, false, job.gr, job.seed, 0, job.nrep, st)) return rc;
        if (int rc = chain_eval_launch(s, l, (uint32_t)job.ts, job.nrep, s->dvbase.get(), (uint64_t)job.gr.nK * job.gr.nd,
                                       d_by_class, d_out, st))
            return rc;
    }
    return MDP_OK;
}

}  // namespace

extern "C" {

// Every refusal comes before the engine exists; the engine's device side is
// set up by the first call that computes, after that call's own refusals.
int mdp_scenario_chain_create(const int32_t *row, uint32_t n, double m, float p, double d, int kind, int device,
                              const char *options, mdp_scenario_chain **out)
{
    if (!out) return mdp_set_error(MDP_EINVAL, "null argument");
    *out = nullptr;
    ChainOpts opts;
    if (int rc = chain_parse_opts(options, &opts)) return rc;
    std::unique_ptr<mdp_scenario_chain> s(new (std::nothrow) mdp_scenario_chain());
    if (!s) return mdp_set_error(MDP_ENOMEM, "out of host memory");
    if (int rc = chain_plan(row, n, m, p, d, kind, opts, &s->plan)) return rc;
    s->device = device;
    snprintf(s->kname, sizeof s->kname, "k_scnchain<%u>", s->plan.nm);
    *out = s.release();
    return MDP_OK;
}

void mdp_scenario_chain_destroy(mdp_scenario_chain *s)
{
    delete s;  // (its destructor releases the device side)
}

const char *mdp_scenario_chain_kernel(const mdp_scenario_chain *s) { return s ? s->kname : ""; }

int mdp_scenario_chain_target(const mdp_scenario_chain *s, double *target)
{
    if (!s || !target) return mdp_set_error(MDP_EINVAL, "null argument");
    std::copy(s->plan.target.begin(), s->plan.target.end(), target);
    return MDP_OK;
}

int mdp_scenario_chain_counts(mdp_scenario_chain *s, int baseline, const double *e, uint32_t ne, const double *c,
                              uint32_t nc, const double *K, uint32_t nK, const double *dsrc, uint32_t nd, uint64_t seed,
                              uint64_t rep0, uint64_t nrep, uint64_t *cnt)
{
    if (!s) return mdp_set_error(MDP_EINVAL, "null scenario chain");
    if (!cnt) return mdp_set_error(MDP_EINVAL, "null count table");
    ChainCall call;
    if (int rc = chain_call(s->plan, baseline != 0, e, ne, c, nc, K, nK, dsrc, nd, nrep, true, &call)) return rc;
    if (nrep == 0) return MDP_OK;
    if (int rc = chain_device(s)) return rc;
    const ChainGrid gr{e, c, K, dsrc, ne, nc, baseline ? 0u : nK, baseline ? 0u : nd};
    if (int rc = chain_upload(s, gr)) return rc;
    if (int rc = s->dtab.grow(chain_tab_cells(s->plan, call))) return rc;
    const size_t cells = (size_t)(s->plan.n + 1) * (s->plan.n + 1);
    std::vector<uint32_t> h;
    for (const ChainLaunch &l : call.launches) {
        if (int rc = chain_count_launch(s, call, l, baseline != 0, gr, seed, rep0, nrep, s->stream)) return rc;
        h.resize((size_t)l.npts * cells);
        HIP_TRY(hipMemcpyAsync(h.data(), s->dtab.get(), h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        uint64_t *dst = cnt + (size_t)l.p0 * cells;
        for (size_t i = 0; i < h.size(); ++i) dst[i] += h[i];
    }
    return MDP_OK;
}

int mdp_scenario_chain_eval(const mdp_scenario_chain *s, int ts, int tdis, uint32_t ne, uint32_t nc, uint32_t nK,
                            uint32_t nd, const uint64_t *cnt_scn, uint64_t nrep, const uint64_t *cnt_base,
                            uint64_t nbase, const double *start, const double *target, double *out, double *by_class)
{
    if (!s) return mdp_set_error(MDP_EINVAL, "null scenario chain");
    return chain_eval(s->plan, ts, tdis, ne, nc, nK, nd, cnt_scn, nrep, cnt_base, nbase, start, target, out, by_class);
}

int mdp_scenario_chain_lik_device(mdp_scenario_chain *s, int ts, int tdis, const double *e, uint32_t ne,
                                  const double *c, uint32_t nc, const double *K, uint32_t nK, const double *dsrc,
                                  uint32_t nd, uint64_t seed, uint64_t nrep, uint64_t nbase, const double *start,
                                  const double *target, double *d_out, void *stream)
{
    if (!s) return mdp_set_error(MDP_EINVAL, "null scenario chain");
    if (!d_out) return mdp_set_error(MDP_EINVAL, "null output");
    ChainJob job;
    if (int rc = chain_job(s->plan, ts, tdis, e, ne, c, nc, K, nK, dsrc, nd, seed, nrep, nbase, start, target, &job))
        return rc;
    if (int rc = chain_device(s)) return rc;
    if (int rc = chain_prepare(s, job, start, target, false, false)) return rc;
    hipStream_t st = (hipStream_t)stream;  // as given: NULL is HIP's null stream
    s->launched_on(st);
    return chain_run(s, job, nullptr, d_out, st);
}

int mdp_scenario_chain_lik(mdp_scenario_chain *s, int ts, int tdis, const double *e, uint32_t ne, const double *c,
                           uint32_t nc, const double *K, uint32_t nK, const double *dsrc, uint32_t nd, uint64_t seed,
                           uint64_t nrep, uint64_t nbase, const double *start, const double *target, double *out,
                           double *by_class)
{
    if (!s) return mdp_set_error(MDP_EINVAL, "null scenario chain");
    if (!out) return mdp_set_error(MDP_EINVAL, "null output");
    ChainJob job;
    if (int rc = chain_job(s->plan, ts, tdis, e, ne, c, nc, K, nK, dsrc, nd, seed, nrep, nbase, start, target, &job))
        return rc;
    if (int rc = chain_device(s)) return rc;
    if (int rc = chain_prepare(s, job, start, target, by_class != nullptr, true)) return rc;
    if (int rc = chain_run(s, job, by_class ? s->dbyclass.get() : nullptr, s->dout.get(), s->stream)) return rc;
    const size_t G = (size_t)job.scn.G, ncl = s->plan.n + 1;
    HIP_TRY(hipMemcpyAsync(out, s->dout.get(), G * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    if (by_class)
        HIP_TRY(hipMemcpyAsync(by_class, s->dbyclass.get(), G * ncl * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return MDP_OK;
}

int mdp_scenario_chain_time_kernels(mdp_scenario_chain *s, int ts, int tdis, const double *e, uint32_t ne,
                                    const double *c, uint32_t nc, const double *K, uint32_t nK, const double *dsrc,
                                    uint32_t nd, uint64_t seed, uint64_t nrep, uint64_t nbase, int reps, double *ms)
{
    if (!s) return mdp_set_error(MDP_EINVAL, "null scenario chain");
    ChainJob job;
    if (int rc = chain_job(s->plan, ts, tdis, e, ne, c, nc, K, nK, dsrc, nd, seed, nrep, nbase, nullptr, nullptr, &job))
        return rc;
    if (!ms || reps <= 0) return mdp_set_error(MDP_EINVAL, "bad timing request");
    if (int rc = chain_device(s)) return rc;
    if (int rc = chain_prepare(s, job, nullptr, nullptr, false, true)) return rc;
    const uint32_t ncl = s->plan.n + 1;
    hipStream_t st = s->stream;
    // phase 0: the baseline counts, 1: the scenario counts, 2: both evaluations
    // (of the table the last launch left: the same work for any counts)
    auto phase = [&](int ph) -> int {
        if (ph != 1)
            for (const ChainLaunch &l : job.base.launches) {
                if (ph == 0) {
                    if (int rc = chain_count_launch(s, job.base, l, true, job.gr, seed, 0, nbase, st)) return rc;
                } else if (int rc = chain_eval_launch(s, l, (uint32_t)tdis, nbase, s->dw.get() + ncl, 0, s->dvbase.get(),
                                                      nullptr, st))
                    return rc;
            }
        if (ph != 0)
            for (const ChainLaunch &l : job.scn.launches) {
                if (ph == 1) {
                    if (int rc = chain_count_launch(s, job.scn, l, false, job.gr, seed, 0, nrep, st)) return rc;
                } else if (int rc = chain_eval_launch(s, l, (uint32_t)ts, nrep, s->dvbase.get(), (uint64_t)nK * nd,
                                                      nullptr, s->dout.get(), st))
                    return rc;
            }
        return MDP_OK;
    };
    for (int ph = 0; ph < 3; ++ph) {
        if (int rc = phase(ph)) return rc;  // warm-up
        if (int rc = s->time(st, reps, &ms[ph], [&]() { return phase(ph); })) return rc;
    }
    return MDP_OK;
}

}  // extern "C"
