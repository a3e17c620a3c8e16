// midaspom_amd/csrc/spom_scnsim.hip -- the die-off and habitat-loss
// hypotheses by simulation, for first survey rows the exact scenario engine
// (spom_scenario.hip, 2^n states, n <= 16) cannot hold: 17..64 patches with
// k_scnsim<NM>, 65..1024 with k_scnsim_wave<NP> further down, and any
// smaller row.  The reference's authors do the same in R
// (Rscript/simuls_traj.R, simtrajH1 / simtrajH2): draw an initial state, run
// ts years under the scenario and tdis baseline years, tally the final state.
//
// With a uniform initial state the estimator is exact in expectation:
//   L = sum_i sum_s [PK^ts P^tdis]_{i,s} prior_s
//     = 2^n E[ prior(final) 1{final compatible with the row} ]
// (main_MIDASPOM_dieoff.c:304-351, main_MIDASPOM_loss.c:341-386).
//
// One replicate rg = rep0 + r, the same for every grid point but for its
// rates (common random numbers: the counter holds no grid point):
//   initial state  w = philox(seed; rg_lo, rg_hi, 0xffffffff, 1 + (k >> 7)):
//                  patch k occupied iff bit k & 31 of word (k >> 5) & 3 (fair
//                  bits; one counter per 128 patches, {.., 1} for k < 64);
//   year t         the future engine's addressing (spom_future.hip): pair
//                  m = k >> 1, w = philox(seed; rg_lo, rg_hi, t, m), word
//                  2(k&1) the extinction draw, 2(k&1)+1 the colonisation draw;
//   rates          s1_k = sum over surviving l != k, ascending, of M[l][k];
//                  scenario years t < ts:
//                    die-off (dieoff.c:51-83)  E = min(1, e/K), pC = min(1, (c s1) K)
//                    loss (loss.c:52-105)      E = min(1, e),   pC = min(1, c (s1 + src_k K))
//                  baseline years: E = min(1, e), pC = min(1, c s1).
// Contraction is off: every product is rounded before the next operation.
//
// GPU design of k_scnsim<NM>: one lane per (grid point, replicate), the 64 lanes of a wave on
// one grid point, so K, e, c, E and the source row are wave-uniform (scalar
// operands).  A work tile is (point, 256 replicates); workgroups of 256
// threads walk the tiles grid-stride.  Occupancy is one 64-bit mask; the
// year is the future engine's (lane_year<NM>, spom_sim_year.h) on the unscaled
// M, K applied after the sum.  The tallies happen once per trajectory: ballots
// per wave, then 64-bit integer atomics into the global tables -- exact, the
// same for every split.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <type_traits>
#include <vector>

#include "spom_dev.h"
#include "spom_scnsim_plan.h"

#pragma clang fp contract(off)

#include "spom_rng.h"
#include "spom_sim_year.h"  // kTabN, sim_year_table, sim_year<NM>, wide_year<NP>: the model's year

namespace {

struct SimArgs {
    uint32_t n, nmiss, ts, tdis;
    uint32_t nc, nK, nd, kind;
    uint64_t p0;       // first grid point of the launch
    uint64_t tiles;    // work tiles of the launch: points x tpp
    uint64_t tpp;      // tiles per point: ceil(nrep / 256)
    uint64_t rep0, nrep;
    uint32_t key0, key1;
    uint64_t live, fixed, missmask;
};

template <int NM>
__global__ __launch_bounds__(kSimBlock) void k_scnsim(SimArgs a, const double *__restrict__ M,
                                                      const double *__restrict__ srcv,
                                                      const double *__restrict__ ev, const double *__restrict__ cv,
                                                      const double *__restrict__ Kv,
                                                      const uint32_t *__restrict__ miss,
                                                      unsigned long long *__restrict__ hist,
                                                      unsigned long long *__restrict__ match)
{
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    double *Ts = dyn;
    if constexpr (NM == kTabN) {
        sim_year_table(a.n, M, Ts, kSimBlock);
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t npairs = (a.n + 1) >> 1;
    const uint32_t years = a.ts + a.tdis;
    for (uint64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        // workgroup-uniform: the tile's grid point; wave-uniform: its replicates
        const uint64_t pl = tile / a.tpp;
        const uint64_t g = a.p0 + pl;
        const uint64_t rb = (tile - pl * a.tpp) * kSimBlock + (threadIdx.x & ~63u);
        if (rb >= a.nrep) continue;  // a wave past the last replicate
        const uint64_t r = rb + lane, rg = a.rep0 + r;
        const bool act = r < a.nrep;
        const uint32_t id = (uint32_t)(g % a.nd), iK = (uint32_t)((g / a.nd) % a.nK);
        const uint32_t ic = (uint32_t)((g / ((uint64_t)a.nd * a.nK)) % a.nc);
        const uint32_t ie = (uint32_t)(g / ((uint64_t)a.nd * a.nK * a.nc));
        const double e = ev[ie], c = cv[ic], K = Kv[iK];
        double Eb = e;  // baseline and loss: E = e (loss.c:57)
        if (Eb > 1) Eb = 1;
        double Es = a.kind ? e : e / K;  // dieoff.c:56-57
        if (Es > 1) Es = 1;
        const double Ks = a.kind ? K : 0.0, Km = a.kind ? 1.0 : K;
        const double *src = srcv + (size_t)id * NM;
        // ---- initial state: 64 fair bits
        uint64_t occ = 0;
        if (act) {
            const u32x4 w = philox(a.key0, a.key1, u32x4{(uint32_t)rg, (uint32_t)(rg >> 32), 0xffffffffu, 1u});
            occ = (((uint64_t)w.y << 32) | w.x) & a.live;
        }
        // ---- ts scenario years, then tdis baseline years
        for (uint32_t t = 0; t < years; ++t) {
            const bool scen = t < a.ts;
            // nobody left in the wave and no source in this or any later
            // year: every sum is 0, pC = c*0, and no draw is below 0
            if (!(a.kind && scen) && __ballot(act && occ != 0) == 0) break;
            if (act) occ = sim_year<NM>(a, M, src, Ts, rg, t, npairs, occ, scen ? Es : Eb, c, scen ? Ks : 0.0,
                                        scen ? Km : 1.0);
        }
        // ---- tallies of the final state
        if (hist) {  // one atomic per distinct occupied count in the wave
            const uint32_t m = (uint32_t)__popcll(occ);
            unsigned long long *row = hist + g * (a.n + 1);
            uint64_t rem = __ballot(act);
            while (rem) {
                const uint32_t lead = (uint32_t)__builtin_ctzll(rem);
                const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)m, (int)lead);
                const uint64_t same = __ballot(act && m == v);
                if (lane == lead) atomicAdd(&row[v], (unsigned long long)__popcll(same));
                rem &= ~same;
            }
        }
        if (match) {  // compatible with the row: its completion, the first missing patch the MSB
            const bool ok = act && ((occ ^ a.fixed) & ~a.missmask) == 0;
            uint32_t j = 0;
            for (uint32_t q = 0; q < a.nmiss; ++q) j = (j << 1) | (uint32_t)((occ >> miss[q]) & 1u);
            unsigned long long *row = match + (g << a.nmiss);
            uint64_t rem = __ballot(ok);
            while (rem) {
                const uint32_t lead = (uint32_t)__builtin_ctzll(rem);
                const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)j, (int)lead);
                const uint64_t same = __ballot(ok && j == v);
                if (lane == lead) atomicAdd(&row[v], (unsigned long long)__popcll(same));
                rem &= ~same;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// k_scnsim_wave<NP>: rows of 65..1024 patches (and any smaller row).  One
// wave per (grid point, replicate), the shape of k_future_wide<NP>
// (spom_future.hip): lane lambda owns the patch pairs m = lambda + 64*j,
// j < NP, and holds patch 2m + p in bit 2j + p of its occupancy word.  The
// survivors of a year are 2*NP wave ballots, walked in ascending patch order
// (j, then lane, then parity); every step adds one row of the unscaled
// Toeplitz table, a window of the two-sided distance image in LDS
// (spom_scnsim_plan.h), to the lane's 2*NP running sums: wide_year<NP> of
// spom_sim_year.h, the function k_future_wide calls, so the same stream and the
// same sums in the same order, K applied after the sum by sim_year's expression:
// on n <= 64 patches the tables of k_scnsim<NM>, bit for bit.  A work tile is
// (point, 4 replicates), one per wave of the workgroup.
// ---------------------------------------------------------------------------
struct SimWaveArgs {
    uint32_t n, nmiss, ts, tdis;
    uint32_t nc, nK, nd, kind;
    uint64_t p0;       // first grid point of the launch
    uint64_t tiles;    // work tiles of the launch: points x tpp
    uint64_t tpp;      // tiles per point: ceil(nrep / 4)
    uint64_t rep0, nrep;
    uint32_t key0, key1;
    uint32_t len, pad;  // len: doubles per copy of the distance image
};

template <int NP>
__global__ __launch_bounds__(kSimBlock) void k_scnsim_wave(SimWaveArgs a, const double *__restrict__ image,
                                                           const double *__restrict__ srcv,
                                                           const double *__restrict__ ev, const double *__restrict__ cv,
                                                           const double *__restrict__ Kv,
                                                           const uint32_t *__restrict__ rowbits,  // fixed[64] | missmask[64]
                                                           const uint32_t *__restrict__ miss,
                                                           unsigned long long *__restrict__ hist,
                                                           unsigned long long *__restrict__ match)
{
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    // both copies of the distance image: 2*len doubles
    double2 *G2 = reinterpret_cast<double2 *>(dyn);
    for (uint32_t i = threadIdx.x; i < a.len; i += kSimBlock) G2[i] = reinterpret_cast<const double2 *>(image)[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t npairs = (a.n + 1) >> 1;
    const uint32_t years = a.ts + a.tdis;
    const uint32_t fixed = rowbits[lane], missmask = rowbits[64 + lane];
    // bit 2j+p set where patch 2*(lane + 64*j) + p exists
    uint32_t live = 0;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const uint32_t k0 = 2 * (lane + 64u * j);
        if (k0 < a.n) live |= 1u << (2 * j);
        if (k0 + 1 < a.n) live |= 2u << (2 * j);
    }
    for (uint64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        // workgroup-uniform: the tile's grid point; wave-uniform: its replicate
        const uint64_t pl = tile / a.tpp;
        const uint64_t g = a.p0 + pl;
        const uint64_t r = (tile - pl * a.tpp) * kSimWaveReps + wave;
        if (r >= a.nrep) continue;  // a wave past the last replicate
        const uint64_t rg = a.rep0 + r;
        const uint32_t id = (uint32_t)(g % a.nd), iK = (uint32_t)((g / a.nd) % a.nK);
        const uint32_t ic = (uint32_t)((g / ((uint64_t)a.nd * a.nK)) % a.nc);
        const uint32_t ie = (uint32_t)(g / ((uint64_t)a.nd * a.nK * a.nc));
        const double e = ev[ie], c = cv[ic], K = Kv[iK];
        double Eb = e;  // baseline and loss: E = e (loss.c:57)
        if (Eb > 1) Eb = 1;
        double Es = a.kind ? e : e / K;  // dieoff.c:56-57
        if (Es > 1) Es = 1;
        const double Ks = a.kind ? K : 0.0, Km = a.kind ? 1.0 : K;
        const double *src = srcv + (size_t)id * (128 * NP);
        // ---- initial state: patch k = 2*(lane + 64*j) + p from bit k & 31 of
        // word (k >> 5) & 3 of counter (rg, 0xffffffff, 1 + (k >> 7)); k >> 7 = j
        uint32_t occ = 0;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const u32x4 w = philox(a.key0, a.key1, u32x4{(uint32_t)rg, (uint32_t)(rg >> 32), 0xffffffffu, 1u + j});
            const uint32_t q = (lane >> 4) & 3u;
            const uint32_t word = q == 0 ? w.x : q == 1 ? w.y : q == 2 ? w.z : w.w;
            occ |= ((word >> (2 * (lane & 15u))) & 3u) << (2 * j);
        }
        occ &= live;
        // ---- ts scenario years, then tdis baseline years
        for (uint32_t t = 0; t < years; ++t) {
            const bool scen = t < a.ts;
            // the replicate is extinct and no source in this or any later
            // year: every sum is 0, pC = c*0, and no draw is below 0
            if (!(a.kind && scen) && __ballot(occ != 0) == 0) break;
            // (ks, km) as sim_year: pC = (c (s1 + src_k ks)) km
            const double ks = scen ? Ks : 0.0, km = scen ? Km : 1.0;
            occ = wide_year<NP>(a, G2, src, rg, t, lane, npairs, live, occ, scen ? Es : Eb, [&](double s, double sv) {
                const double sk = sv * ks;   // loss.c:95-98: the product is rounded before the add
                return (c * (s + sk)) * km;  // dieoff.c:78 (c s1) K
            });
        }
        // ---- tallies of the final state: one integer atomic per table
        if (hist) {
            uint32_t m = 0;
#pragma unroll
            for (int b = 0; b < 2 * NP; ++b) m += (uint32_t)__popcll(__ballot((occ >> b) & 1u));
            if (lane == 0) atomicAdd(&hist[g * (a.n + 1) + m], 1ull);
        }
        if (match) {  // compatible with the row: its completion, the first missing patch the MSB
            const bool ok = ((occ ^ fixed) & ~missmask & live) == 0;
            uint32_t j = 0;
            for (uint32_t q = 0; q < a.nmiss; ++q) {
                const uint32_t mq = miss[q];
                j = (j << 1) | (uint32_t)(__ballot(lane == (mq >> 8) && ((occ >> (mq & 0xffu)) & 1u)) != 0);
            }
            if (__ballot(!ok) == 0 && lane == 0) atomicAdd(&match[(g << a.nmiss) + j], 1ull);
        }
    }
}

}  // namespace

// (DevQueue: the device, stream and events, released after the buffers below)
struct mdp_scenario_sim : DevQueue {
    SimPlan plan;
    char kname[32] = "";
    DevBuf<double> dM, dgrid;  // dM: the lane kernel's table, or the wave kernel's image
    DevBuf<uint32_t> drow;     // the wave kernel's fixed[64] | missmask[64]
    DevBuf<uint32_t> dmiss;
    DevBuf<unsigned long long> dhist, dmatch;
    ~mdp_scenario_sim() { drain(); }  // (never opened: nothing below exists, no HIP call)
};

namespace {

// the device side of an engine, set up by the first call that needs it: the
// device, stream and events, then the tables, uploaded once
int sim_device(mdp_scenario_sim *s)
{
    if (int rc = s->open()) return rc;
    const SimPlan &p = s->plan;
    if (s->dM.empty())
        if (int rc = s->dM.assign(p.np ? p.image : p.M)) return rc;
    if (s->dmiss.empty())
        if (int rc = s->dmiss.assign(p.np ? p.wmiss : p.miss)) return rc;
    if (p.np && s->drow.empty()) {
        std::vector<uint32_t> rowbits(p.wfixed);
        rowbits.insert(rowbits.end(), p.wmissmask.begin(), p.wmissmask.end());
        if (int rc = s->drow.assign(rowbits)) return rc;
    }
    return MDP_OK;
}

struct SimGrid {
    int ts, tdis;
    const double *e, *c, *K, *dsrc;
    uint32_t ne, nc, nK, nd;
};

// doubles of s->dgrid before the source rows: the three axes, rounded up to
// an even count (k_scnsim_wave reads the rows as double2)
size_t sim_src_at(const SimGrid &gr) { return ((size_t)gr.ne + gr.nc + gr.nK + 1) & ~(size_t)1; }

// the axes and the source rows into s->dgrid: [e | c | K | (pad) | src[nd][ld]].
// The copy is synchronous on the null stream, which nothing orders against a
// caller's non-blocking stream: a device form still pending -- on the stream of
// this call or on any other -- reads the buffer and is waited for first
// (spom_dev.h, the stream rule).  The host forms leave nothing behind on
// s->stream.
int sim_upload(mdp_scenario_sim *s, const SimGrid &gr)
{
    std::vector<double> src;
    sim_src(s->plan, gr.dsrc, gr.nd, &src);
    std::vector<double> h;
    h.reserve(sim_src_at(gr) + src.size());
    h.insert(h.end(), gr.e, gr.e + gr.ne);
    h.insert(h.end(), gr.c, gr.c + gr.nc);
    h.insert(h.end(), gr.K, gr.K + gr.nK);
    h.resize(sim_src_at(gr), 0.0);
    h.insert(h.end(), src.begin(), src.end());
    if (int rc = s->settle()) return rc;
    return s->dgrid.assign(h);
}

// every launch of a call on st; the tables accumulate
int sim_launch(mdp_scenario_sim *s, const SimCall &call, const SimGrid &gr, uint64_t seed, uint64_t rep0,
               uint64_t nrep, unsigned long long *d_hist, unsigned long long *d_match, hipStream_t st)
{
    const SimPlan &p = s->plan;
    const double *de = s->dgrid.get(), *dc = de + gr.ne, *dK = dc + gr.nc, *dsrc = de + sim_src_at(gr);
    // the fields SimArgs and SimWaveArgs share, of launch l
    auto common = [&](auto &a, const SimLaunch &l) {
        a.n = p.n;
        a.nmiss = p.nmiss;
        a.ts = (uint32_t)gr.ts;
        a.tdis = (uint32_t)gr.tdis;
        a.nc = gr.nc;
        a.nK = gr.nK;
        a.nd = gr.nd;
        a.kind = (uint32_t)p.kind;
        a.p0 = l.p0;
        a.tiles = l.tiles;
        a.tpp = call.tiles_per_point;
        a.rep0 = rep0;
        a.nrep = nrep;
        a.key0 = (uint32_t)seed;
        a.key1 = (uint32_t)(seed >> 32);
    };
    if (p.np) {
        const size_t lds = (size_t)2 * p.wlen * sizeof(double);  // both copies of the image: <= 32 KB
        for (const SimLaunch &l : call.launches) {
            SimWaveArgs a{};
            common(a, l);
            a.len = p.wlen;
            if (int rc = dev_for_pairs(p.np, [&](auto NP) {
                    hipLaunchKernelGGL(k_scnsim_wave<decltype(NP)::value>, dim3(l.nwg), dim3(kSimBlock), lds, st, a,
                                       s->dM.get(), dsrc, de, dc, dK, s->drow.get(), s->dmiss.get(), d_hist, d_match);
                    return MDP_OK;
                }))
                return rc;
            HIP_TRY(hipGetLastError());
        }
        return MDP_OK;
    }
    const size_t lds = p.nm == kTabN ? sizeof(double) * (kTabN << kTabN) : 0;
    for (const SimLaunch &l : call.launches) {
        SimArgs a{};
        common(a, l);
        a.live = p.live;
        a.fixed = p.fixed;
        a.missmask = p.missmask;
        if (int rc = dev_for_padded(p.nm, [&](auto NM) {
                hipLaunchKernelGGL(k_scnsim<decltype(NM)::value>, dim3(l.nwg), dim3(kSimBlock), lds, st, a, s->dM.get(), dsrc,
                                   de, dc, dK, s->dmiss.get(), d_hist, d_match);
                return MDP_OK;
            }))
            return rc;
        HIP_TRY(hipGetLastError());
    }
    return MDP_OK;
}

}  // namespace

extern "C" {

// Every refusal comes before the engine exists; the engine's device side is
// set up by the first call that computes, after that call's own refusals.
int mdp_scenario_sim_create(const int32_t *row, uint32_t n, double m, float p, double d, int kind, int device,
                            const char *options, mdp_scenario_sim **out)
{
    if (!out) return mdp_set_error(MDP_EINVAL, "null argument");
    *out = nullptr;
    SimOpts opts;
    if (int rc = sim_parse_opts(options, &opts)) return rc;
    std::unique_ptr<mdp_scenario_sim> s(new (std::nothrow) mdp_scenario_sim());
    if (!s) return mdp_set_error(MDP_ENOMEM, "out of host memory");
    if (int rc = sim_plan(row, n, m, p, d, kind, opts, &s->plan)) return rc;
    s->device = device;
    if (s->plan.np) snprintf(s->kname, sizeof s->kname, "k_scnsim_wave<%u>", s->plan.np);
    else snprintf(s->kname, sizeof s->kname, "k_scnsim<%u>", s->plan.nm);
    *out = s.release();
    return MDP_OK;
}

void mdp_scenario_sim_destroy(mdp_scenario_sim *s)
{
    delete s;  // (its destructor releases the device side)
}

const char *mdp_scenario_sim_kernel(const mdp_scenario_sim *s) { return s ? s->kname : ""; }

int mdp_scenario_sim_tables_device(mdp_scenario_sim *s, int ts, int tdis, const double *e, uint32_t ne,
                                   const double *c, uint32_t nc, const double *K, uint32_t nK, const double *dsrc,
                                   uint32_t nd, uint64_t seed, uint64_t rep0, uint64_t nrep, uint64_t *d_hist,
                                   uint64_t *d_match, void *stream)
{
    if (!s) return mdp_set_error(MDP_EINVAL, "null scenario simulator");
    SimCall call;
    if (int rc = sim_call(s->plan, ts, tdis, e, ne, c, nc, K, nK, dsrc, nd, nrep, d_hist != nullptr,
                          d_match != nullptr, &call))
        return rc;
    if (int rc = sim_device(s)) return rc;
    hipStream_t st = (hipStream_t)stream;  // as given: NULL is HIP's null stream
    const SimGrid gr{ts, tdis, e, c, K, dsrc, ne, nc, nK, nd};
    if (int rc = sim_upload(s, gr)) return rc;
    s->launched_on(st);
    if (d_hist) HIP_TRY(hipMemsetAsync(d_hist, 0, call.hist_cells * sizeof(uint64_t), st));
    if (d_match) HIP_TRY(hipMemsetAsync(d_match, 0, call.match_cells * sizeof(uint64_t), st));
    return sim_launch(s, call, gr, seed, rep0, nrep, (unsigned long long *)d_hist, (unsigned long long *)d_match, st);
}

int mdp_scenario_sim_tables(mdp_scenario_sim *s, int ts, int tdis, const double *e, uint32_t ne, const double *c,
                            uint32_t nc, const double *K, uint32_t nK, const double *dsrc, uint32_t nd, uint64_t seed,
                            uint64_t rep0, uint64_t nrep, uint64_t *hist, uint64_t *match)
{
    if (!s) return mdp_set_error(MDP_EINVAL, "null scenario simulator");
    SimCall call;
    if (int rc = sim_call(s->plan, ts, tdis, e, ne, c, nc, K, nK, dsrc, nd, nrep, hist != nullptr, match != nullptr,
                          &call))
        return rc;
    if (nrep == 0) return MDP_OK;
    if (int rc = sim_device(s)) return rc;
    if (hist)
        if (int rc = s->dhist.grow((size_t)call.hist_cells)) return rc;
    if (match)
        if (int rc = s->dmatch.grow((size_t)call.match_cells)) return rc;
    int rc = mdp_scenario_sim_tables_device(s, ts, tdis, e, ne, c, nc, K, nK, dsrc, nd, seed, rep0, nrep,
                                            hist ? (uint64_t *)s->dhist.get() : nullptr,
                                            match ? (uint64_t *)s->dmatch.get() : nullptr, s->stream);
    if (rc) return rc;
    std::vector<uint64_t> hh(hist ? (size_t)call.hist_cells : 0), hm(match ? (size_t)call.match_cells : 0);
    if (hist)
        HIP_TRY(hipMemcpyAsync(hh.data(), s->dhist.get(), hh.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream));
    if (match)
        HIP_TRY(hipMemcpyAsync(hm.data(), s->dmatch.get(), hm.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->waited_for(s->stream);
    for (size_t i = 0; i < hh.size(); ++i) hist[i] += hh[i];
    for (size_t i = 0; i < hm.size(); ++i) match[i] += hm[i];
    return MDP_OK;
}

int mdp_scenario_sim_lik(const mdp_scenario_sim *s, const uint64_t *match, size_t npoints, uint64_t nrep, double *out)
{
    if (!s) return mdp_set_error(MDP_EINVAL, "null scenario simulator");
    return sim_lik(s->plan, match, npoints, nrep, out);
}

int mdp_scenario_sim_time_kernel(mdp_scenario_sim *s, int ts, int tdis, const double *e, uint32_t ne, const double *c,
                                 uint32_t nc, const double *K, uint32_t nK, const double *dsrc, uint32_t nd,
                                 uint64_t seed, uint64_t nrep, int reps, double *ms)
{
    if (!s) return mdp_set_error(MDP_EINVAL, "null scenario simulator");
    const bool want_match = s->plan.nmiss <= kSimMaxMatchMissing;
    SimCall call;
    if (int rc = sim_call(s->plan, ts, tdis, e, ne, c, nc, K, nK, dsrc, nd, nrep, true, want_match, &call)) return rc;
    if (!ms || reps <= 0 || nrep == 0) return mdp_set_error(MDP_EINVAL, "bad timing request");
    if (int rc = sim_device(s)) return rc;
    if (int rc = s->dhist.grow((size_t)call.hist_cells)) return rc;
    if (want_match)
        if (int rc = s->dmatch.grow((size_t)call.match_cells)) return rc;
    const SimGrid gr{ts, tdis, e, c, K, dsrc, ne, nc, nK, nd};
    if (int rc = sim_upload(s, gr)) return rc;
    HIP_TRY(hipMemsetAsync(s->dhist.get(), 0, call.hist_cells * sizeof(uint64_t), s->stream));
    if (want_match) HIP_TRY(hipMemsetAsync(s->dmatch.get(), 0, call.match_cells * sizeof(uint64_t), s->stream));
    auto launch = [&]() {
        return sim_launch(s, call, gr, seed, 0, nrep, s->dhist.get(), want_match ? s->dmatch.get() : nullptr, s->stream);
    };
    if (int rc = launch()) return rc;  // warm-up
    return s->time(s->stream, reps, ms, launch);
}

}  // extern "C"
