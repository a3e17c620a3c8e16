/*
 * include/midaspom.h -- C ABI of the MI355X-native MIDASPOM posterior-grid engine.
 *
 * The reference (nalcala/MIDASPOM) is one monolithic main() per program with
 * no library API; these entry points are the seams a C caller of the
 * reference's pipeline would bind.  Each declaration cites
 * the region of /root/reference/sources/main_MIDASPOM.c it replaces.
 *
 * Conventions
 *  - plain pointers and sizes only; no torch / HIP types in signatures
 *    (streams are passed as void*, i.e. a hipStream_t; it is used exactly as
 *    given, so NULL is HIP's null stream -- the stream torch's default
 *    `torch.cuda.current_stream().cuda_stream == 0` names);
 *  - every int-returning function returns MDP_OK (0) or a negative MDP_E*
 *    code; the reason is in mdp_last_error() (thread-local).  Nothing aborts
 *    or exits across the ABI;
 *  - an engine is not re-entrant; one host thread drives all its devices;
 *  - Streams.  The device forms (mdp_engine_run, mdp_scenario_run,
 *    mdp_future_simulate_device / _summary_device with mdp_future_check,
 *    mdp_scenario_sim_tables_device, mdp_scenario_chain_lik_device, the two
 *    *_time_kernels) launch on the caller's stream and return; what the
 *    caller queues on that stream afterwards is ordered after them.  A call on a handle gives the result
 *    it would give alone, whatever earlier device-form calls on that handle
 *    are still pending on any stream.  Only the caller's output buffers are
 *    the caller's to order.  A call that rewrites or reuses device state a
 *    pending launch may read -- a new grid (mdp_engine_set_grid,
 *    mdp_scenario_set_grid, every mdp_scenario_sim_tables* and
 *    mdp_scenario_chain_* computing call), a host form,
 *    a device form on a stream other than the pending one -- first waits for
 *    the device; a device form behind another on the same stream does not
 *    wait and makes no extra HIP call.  A stream need not outlive the work it
 *    was given, but a device form on a stream that reuses the handle value of
 *    one destroyed with work pending counts as "the same stream": synchronise
 *    a stream before destroying it if that can happen;
 *  - results are deterministic (no floating-point atomics in any reduction;
 *    the future engine's integer counts -- the per-year extinct counts and
 *    the summary tables hist / occ of mdp_future_summary -- use LDS and
 *    global integer atomics, exact in any order).
 */
#ifndef MIDASPOM_H
#define MIDASPOM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDP_OK 0
#define MDP_EINVAL (-1)       /* bad argument / malformed problem          */
#define MDP_EIO (-2)          /* cannot open / write a file                */
#define MDP_ENOMEM (-3)       /* host or device allocation failed          */
#define MDP_EHIP (-4)         /* HIP runtime error                         */
#define MDP_ENODEV (-5)       /* no usable GPU                             */
#define MDP_EUNSUPPORTED (-6) /* problem outside the engine's limits       */

#define MDP_ABI_VERSION 9

/* ------------------------------------------------------------------ */
/* Host model: parse + state enumeration (the reference's L2 layer)    */
/* ------------------------------------------------------------------ */

/* Parsed and enumerated observation model (opaque, host memory). */
typedef struct mdp_model mdp_model;

/* Read an occupancy file and enumerate its states.
 * Replaces main_MIDASPOM.c:137-287 (parse :141-167 with quirk Q6, variable
 * columns :172-175, dispersal M :177-188, state bits :198-211, per-year
 * observed states + float32 prior :214-255, short-id dedup :256-287).
 * m = mean dispersal distance (-m), p = prior occupancy of missing year-0
 * patches (-p, used as float32 like :66), d = segment length (-d). */
int mdp_model_load(const char *path, double m, float p, double d, mdp_model **out);

/* Same, from an in-memory observation matrix obs[tmax][n] (values -1/0/1). */
int mdp_model_from_obs(const int32_t *obs, uint32_t n, uint32_t tmax, double m, float p,
                       double d, mdp_model **out);

void mdp_model_free(mdp_model *model);

/* Read-only view of a model; pointers stay owned by the model. */
typedef struct mdp_problem {
    uint32_t n;                 /* patches (columns)                                 */
    uint32_t tmax;              /* years (rows)                                      */
    uint32_t nvar;              /* columns ever non-zero; nstates = 2^nvar           */
    uint32_t nextid;            /* distinct observed states ("short ids")            */
    const int32_t *obs;         /* [tmax][n] parsed observations                     */
    const uint32_t *var_cols;   /* [nvar] ascending column indices                   */
    const double *M;            /* [n][n] dispersal kernel, row-major, diag 0        */
    const uint32_t *short_state;/* [nextid] state id (first var column = MSB)        */
    const uint32_t *year_off;   /* [tmax+1] offsets into year_ids                    */
    const uint32_t *year_ids;   /* [year_off[tmax]] short ids of each year's states  */
    const float *prior;         /* [year_off[1]] float32 prior of year-0 states      */
} mdp_problem;

int mdp_model_problem(const mdp_model *model, mdp_problem *view);

/* ------------------------------------------------------------------ */
/* Grid, normalisation and posterior writer (the reference's L3/L5)    */
/* ------------------------------------------------------------------ */

/* g[i] = i*win + lo for i < s-1, g[s-1] = hi; returns win = (hi-lo)/(s-1).
 * Replaces main_MIDASPOM.c:120 and :312-319. */
double mdp_grid(uint32_t s, double lo, double hi, double *g);

/* Ltot = 2 log(win) + log(sum_k sum_l w_k w_l exp(loglik[k][l])), trapezoid
 * weights 1/2 at the grid ends.  Replaces main_MIDASPOM.c:413-425. */
double mdp_log_total(const double *loglik, uint32_t s, double win);
/* Same on any s x s view: log L of (e row k, c column l) at loglik[k*se +
 * l*sc] -- (s, 1) is the reference's lik[k][l], (1, s) the [c][e] layout the
 * device engine writes fastest (MDP_LAYOUT_CE).  Same summation order, so the
 * same bits (ABI 7). */
double mdp_log_total_view(const double *loglik, uint32_t s, size_t se, size_t sc, double win);

/* Posterior text file: "%.20lf\t" of exp(loglik-ltot) per cell, "\n" per row
 * (rows = e, columns = c).  Replaces main_MIDASPOM.c:427-436.  raw != 0
 * writes loglik itself (the MPI build's Ltot == 0 branch,
 * main_MIDASPOM_MPI.c:527). */
int mdp_write_posterior(const char *path, const double *loglik, uint32_t s, double ltot,
                        int raw);
/* Same on the view loglik[i*se + j*sc] (row i = e, column j = c); the bytes
 * written are the same as for the row-major matrix (ABI 7).  Memory held
 * while writing is bounded (a few MB per host thread) whatever s is. */
int mdp_write_posterior_view(const char *path, const double *loglik, uint32_t s, size_t se, size_t sc, double ltot,
                             int raw);

/* ------------------------------------------------------------------ */
/* GPU likelihood engine (the reference's hot loop, L3 + L4 + L6)      */
/* ------------------------------------------------------------------ */

typedef struct mdp_engine mdp_engine;

/* Build the engine on n_devices GPUs (devices == NULL -> 0..n_devices-1;
 * n_devices == 0 -> the calling thread's current HIP device).  Copies the
 * problem tables to device memory it owns and precomputes the grid-invariant
 * colonisation sums.  Replaces the setup half of main_MIDASPOM.c:341-360
 * (per-point recomputation of S = piall*M moves here, once). */
int mdp_engine_create(const mdp_problem *problem, const int *devices, int n_devices,
                      mdp_engine **out);

/* Same with engine options (ABI 7): "NAME=VALUE" pairs separated by ';', ','
 * or white space, selecting among the engine's parity-tested kernel variants
 * (MDP_FUSED=0|1, MDP_WIDE=1, MDP_JIT_CHUNK=<uses>, ...).
 * The library reads no tuning knob from the environment; mdp_engine_create
 * is this call with options == NULL (the measured defaults).  Measurement-only
 * options (MDP_DIAG, MDP_JIT_HACK, MDP_JIT_WPE) exist only in the diag build
 * (libmidaspom_diag.so, -DMDP_DIAG_BUILD); elsewhere they, like any unknown
 * name, return MDP_EINVAL. */
int mdp_engine_create_opts(const mdp_problem *problem, const int *devices, int n_devices,
                           const char *options, mdp_engine **out);

void mdp_engine_destroy(mdp_engine *engine);

/* out[ie*nc + ic] = log L(e[ie], c[ic]) (-inf where L == 0), host memory.
 * Rows are split over the engine's devices in contiguous slabs (remainder to
 * device 0, as main_MIDASPOM_MPI.c:361-368).  Replaces main_MIDASPOM.c:341-395
 * (and the MPI gather :482-506).  Every c must be finite and >= 0
 * (MDP_EINVAL otherwise, here and in mdp_engine_set_grid): the reference's
 * pC = min(1, c S) (:350-358) is a probability only there, and the kernels'
 * item factors |n - pC| and minNum clamps assume it. */
int mdp_loglik_grid(mdp_engine *engine, const double *e, uint32_t ne, const double *c,
                    uint32_t nc, double *out);

/* Device-resident variant for single-device engines (one process per GPU):
 * upload the grid once, then compute into caller-owned device memory
 * d_out[ie*ld_out + ic] on `stream` (hipStream_t; NULL = HIP's null stream).
 * mdp_engine_run is asynchronous w.r.t. the host.
 * mdp_engine_set_layout (ABI 6) selects the layout mdp_engine_run writes:
 * MDP_LAYOUT_EC (default) d_out[ie*ld_out + ic], the reference's lik[i][j]
 * (main_MIDASPOM.c:390); MDP_LAYOUT_CE d_out[ic*ld_out + ie] (ld_out >= ne),
 * where each workgroup's e values of one c column are contiguous, so its
 * stores coalesce.  Same kernels and values; mdp_loglik_grid is always EC. */
#define MDP_LAYOUT_EC 0
#define MDP_LAYOUT_CE 1
int mdp_engine_set_layout(mdp_engine *engine, int layout);
/* mdp_loglik_grid with the host result in either layout (ABI 7): EC
 * out[ie*nc + ic] (= mdp_loglik_grid), or CE out[ic*ne + ie] -- what every
 * device slab holds natively; mdp_log_total_view / mdp_write_posterior_view
 * read it in place (se = 1, sc = ne), so the drop-in CLIs never transpose. */
int mdp_loglik_grid_layout(mdp_engine *engine, const double *e, uint32_t ne, const double *c, uint32_t nc,
                           int layout, double *out);
int mdp_engine_set_grid(mdp_engine *engine, const double *e, uint32_t ne, const double *c,
                        uint32_t nc);
/* The bound the per-c tables of the following grids are built for (ABI 9):
 * max(|c| over the grid, cbound).  The Z rows split their always-zero
 * columns into explicit factors and a log series by |c| S, so
 * two grids with different max |c| evaluate some columns in different (equally
 * exact, ~1e-15) forms.  Ranks that compute column slabs of ONE grid pass
 * that grid's max |c| here, so each computes the bits a single-rank run
 * would (midaspom_amd/dist.py).  0 (the default) uses the grid's own. */
int mdp_engine_set_cbound(mdp_engine *engine, double cbound);
int mdp_engine_run(mdp_engine *engine, double *d_out, uint32_t ld_out, void *stream);

/* Kernel timing: when enabled, every kernel of a run is launched with its own
 * start/stop events (stamped from the dispatch, no extra packets on the
 * stream).  mdp_engine_kernel_ms fills up to max_k mean durations (ms) over
 * the runs since the previous call, in launch order, and returns the count;
 * mdp_engine_kernel_name gives the slot's kernel ("" for a slot the engine's
 * path does not launch: the direct path runs k_qrows + k_forward, the
 * generic path k_zpv + k_coefs + k_forward). */
int mdp_engine_set_profiling(mdp_engine *engine, int enable);
int mdp_engine_kernel_ms(mdp_engine *engine, double *ms, int max_k);
const char *mdp_engine_kernel_name(const mdp_engine *engine, int k);

/* Per-kernel durations without per-launch events: one full run into d_out,
 * then each kernel of the path launched `reps` times back to back between two
 * events on `stream`; ms[k] = mean duration of slot k (0 where the path has no
 * such kernel; names via mdp_engine_kernel_name), and a final full run leaves
 * d_out as mdp_engine_run computes it.  Returns the number of slots filled. */
int mdp_engine_time_kernels(mdp_engine *engine, double *d_out, uint32_t ld_out, void *stream, int reps,
                            double *ms, int max_k);

/* Diagnostics (diag build, option MDP_DIAG=1 at engine creation): text
 * report of per-workgroup s_memtime phase durations (shader cycles) of the
 * last run's kernels; returns the report length (0 when disabled). */
int mdp_engine_diag_report(mdp_engine *engine, char *buf, size_t len);

/* Work accounting of one run on a grid of ne x nc points (host arithmetic on
 * the enumerated problem): flops of the forward kernel in
 * the implemented factorised form, and the SURVEY.md §8(d) dense-form F_alg. */
int mdp_engine_work(const mdp_engine *engine, uint64_t ne, uint64_t nc, double *flop_impl,
                    double *flop_survey, double *bytes_min);

/* Closed-form FP64 work of the factorised algorithm on an ne x nc grid
 * (DESIGN.md §5), computed from the plan's dimensions alone -- not from any
 * kernel's emitted code -- so a roofline fraction can be recomputed from the
 * problem and a kernel duration.  Per c value: Z rows (3 flops per explicit
 * always-zero column and 2*8 + 2 for the series over the small ones, for the
 * engine's current grid), var-column pressures
 * (1 per row and var column), item factors (1 - pC where B_b = 0, one
 * multiply per free column), Q sums (len - 1 adds per entry).
 *
 * Per grid point, the algorithmic minimum of the ratio forms the forward
 * kernels evaluate (ABI 8): setup_pt -- y = 1 - x, the
 * ratio's division, the power tables past their first powers (g's on s-form
 * points only); use_pt_ratio -- every distinct Q group's Horner chain once
 * (2 nX), g^d once per distinct (group, d > 0) on s-form points, each
 * year's state update npc (2 npp - 1), the source pre-scales, the
 * deferred-exponent flushes; final_pt_ratio -- the prior sum (np_last), the
 * final B^E, log.  Those three are means over the engine's current e grid
 * (its s-form share; one half before a grid is set); pt_min is their sum and
 * flop_min = nc * per-c + ne * nc * pt_min.
 *
 * Legacy (rounds 1-4, the direct form P = sum_m Q[m] W[|A|][m] with a
 * per-point weight table, which the ratio forms no longer build):
 * weight_pt (2 maxA powers + one product per W entry used), use_pt (every
 * use 2 nX + 3), use_pt_min (each distinct transition's dot product once,
 * 2 nX + 1, plus the state updates), final_pt (2 np_last - 1); flop =
 * nc * per-c + ne * nc * (weight_pt + use_pt + final_pt) and
 * flop_min_direct the same with use_pt_min.  The per-c terms are zero on
 * the generic path (MDP_JIT=0), which has no direct plan. */
typedef struct mdp_work {
    double z_c, pc_c, item_c, q_c;        /* per c value */
    double weight_pt, use_pt, final_pt;   /* per grid point (legacy direct form) */
    double flop;                          /* the grid's total, every use (legacy) */
    double use_pt_min;                    /* per grid point, distinct transitions once (legacy) */
    double flop_min;                      /* the grid's algorithmic minimum (ratio forms, ABI 8) */
    double setup_pt, use_pt_ratio, final_pt_ratio, pt_min;  /* per grid point, ratio forms (ABI 8) */
    double flop_min_direct;               /* legacy: the direct form's minimum (flop_min before ABI 8) */
} mdp_work;
int mdp_engine_work_fact(const mdp_engine *engine, uint64_t ne, uint64_t nc, mdp_work *work);

/* Engine facts: number of devices, distinct transition pairs, forward
 * "uses" (one per consecutive-year state pair), coefficients per c value,
 * max states per year, selected kernel variant. */
typedef struct mdp_engine_info {
    int n_devices;
    uint32_t npairs;
    uint32_t nuses;
    uint32_t ncoef;
    uint32_t npmax;
    uint32_t variant;
} mdp_engine_info;
int mdp_engine_get_info(const mdp_engine *engine, mdp_engine_info *info);

/* The kernel instantiations this engine has launched so far, space-separated
 * and sorted (e.g. "k_qrows<16,0,2> mdp_fwd_jit<reading,maxA12>"): which
 * template of each hot-path kernel ran, for tests and profiles.  Writes at
 * most len bytes (NUL-terminated) and returns the full length. */
int mdp_engine_launched(const mdp_engine *engine, char *buf, size_t len);

/* y[i] = log(x[i]) on the current device with the forward kernels' own FP64
 * log (a range reduction and an atanh series; the hipRTC kernels use it for
 * log L), for its accuracy test against the host's libm. */
int mdp_log_check(const double *x, double *y, size_t n);

/* ------------------------------------------------------------------ */
/* Scenario likelihoods: in-situ die-off and habitat loss              */
/* (main_MIDASPOM_dieoff.c / main_MIDASPOM_loss.c)     */
/* ------------------------------------------------------------------ */

/* K grid, log10-spaced on [lo, hi] (dieoff.c:284-286, loss.c:315-317);
 * source-distance grid, linear on [lo, hi] (loss.c:319-322).  Return g[0]. */
double mdp_kgrid(uint32_t s, double lo, double hi, double *K);
double mdp_dgrid(uint32_t s, double lo, double hi, double *d);

typedef struct mdp_scenario mdp_scenario;

/* Engine for the likelihood of the FIRST survey row `row` (n patches, values
 * -1/0/1; dieoff.c:185-232) under the die-off (kind 0) or habitat-loss
 * (kind 1) scenario, on HIP device `device`.  m, p, d as for mdp_model_load
 * (-m, -p, -d).  n <= 16: n <= 8 runs the LDS-resident kernel (factorised
 * Pc tables in LDS), larger n a kernel whose state vectors live in HBM. */
int mdp_scenario_create(const int32_t *row, uint32_t n, double m, float p, double d, int kind, int device,
                        mdp_scenario **out);
/* Same with options (ABI 7): "MDP_SCN_BIG=1" / "MDP_SCN_ROW=1" force the
 * HBM-state / row-parallel kernel for any n they support (tests);
 * "MDP_SCN_LAUNCH_PTS=N" caps the grid points per launch of those two
 * kernels (tests: launch boundaries on small grids; 0 or unset = no cap). */
int mdp_scenario_create_opts(const int32_t *row, uint32_t n, double m, float p, double d, int kind, int device,
                             const char *options, mdp_scenario **out);
void mdp_scenario_destroy(mdp_scenario *scenario);

/* out[((ie*nc + ic)*nK + iK)*nd + id] = L(e, c, K[, dsrc]) =
 * sum_i sum_s [PK^ts P^tdis]_{i,s} prior_s  (not normalised, not log), with
 * ts years before the event (-b) and tdis after (-a).  Die-off
 * (dieoff.c:304-351): PK = Pe(e/K) Pc(c K); dsrc ignored (nd = 1).  Loss
 * (loss.c:341-386): PK = Pe(e) Pc(c, source K at distance dsrc).  The
 * reference programs are the cases ne = nc = 1 (K column, or K x d table);
 * the engine evaluates any (e, c, K[, d]) product grid.  Host memory. */
int mdp_scenario_lik(mdp_scenario *scenario, int ts, int tdis, const double *e, uint32_t ne,
                     const double *c, uint32_t nc, const double *K, uint32_t nK, const double *dsrc,
                     uint32_t nd, double *out);

/* ------------------------------------------------------------------ */
/* Forward simulation of extinction under management scenarios         */
/* (main_MIDASPOM_future.c)                      */
/* ------------------------------------------------------------------ */

/* Input readers of the future program.  *row = the LAST survey row of an
 * occupancy file (n from line 1, tokens streamed across lines;
 * future.c:193-225); *post = the necstep x necstep posterior matrix, necstep
 * = separators on its first line (future.c:237-262).  Free with mdp_free. */
int mdp_future_read_survey(const char *path, uint32_t *n, uint32_t *tmax, int32_t **row);
int mdp_future_read_posterior(const char *path, uint32_t *necstep, double **post);
void mdp_free(void *p);

typedef struct mdp_future mdp_future;

/* Engine for the replicate loop of future.c:343-386 on HIP device `device`:
 * last survey row (n <= 64 patches, values -1/0/1, <= 30 missing), the
 * posterior it samples (e, c) from (row-major necstep^2; e = ie*0.01 and
 * c = ic*0.01 as hard-coded at :370-371), m = mean dispersal (-m), d =
 * segment length (-d), KD = relative population size (-D), KS = source
 * size (-S), dS = source distance (-s). */
int mdp_future_create(const int32_t *last_row, uint32_t n, const double *post, uint32_t necstep, double m,
                      double d, double KD, double KS, double dS, int device, mdp_future **out);
void mdp_future_destroy(mdp_future *future);

/* counts[t] += number of replicates r in [rep0, rep0 + nrep) with every patch
 * empty after year t+1, t < tfut (future.c:381-385; Lik[] there).  Draws are
 * Philox4x32-10 keyed by `seed` and addressed by (replicate, year, patch):
 * results do not depend on how replicates are split (over GPUs, ranks or
 * calls).  Host memory. */
int mdp_future_simulate(mdp_future *future, uint64_t seed, uint64_t rep0, uint64_t nrep, uint32_t tfut,
                        uint64_t *counts);
/* Same into caller-owned device memory d_counts[tfut] (overwritten, not
 * accumulated) on `stream` (NULL = HIP's null stream); asynchronous.  A
 * replicate whose posterior draw needs more look-back than the engine holds
 * raises a sticky device error flag; mdp_future_check waits for `stream`,
 * reads and clears the flag, and returns MDP_EUNSUPPORTED when it was set --
 * the counts of some launch since the previous check are then not valid, so
 * one check after several launches covers all of them (the host form
 * mdp_future_simulate checks its own launch with a separate flag). */
int mdp_future_simulate_device(mdp_future *future, uint64_t seed, uint64_t rep0, uint64_t nrep, uint32_t tfut,
                               uint64_t *d_counts, void *stream);
int mdp_future_check(mdp_future *future, void *stream);
/* Mean duration (ms) of the simulation kernel over `reps` back-to-back
 * launches of replicates [0, nrep) between two events. */
int mdp_future_time_kernel(mdp_future *future, uint64_t seed, uint64_t nrep, uint32_t tfut, int reps, double *ms);
/* The generator itself: out[4] = Philox4x32-10(key, ctr[4]) (host). */
int mdp_future_philox(uint64_t key, const uint32_t *ctr, uint32_t *out);

/* Added after ABI 9 without a version bump (MDP_ABI_VERSION stays 9): detect
 * the three functions below by symbol lookup.
 *
 * mdp_future_create with options, "NAME=VALUE" pairs in the grammar of
 * mdp_engine_create_opts; NULL or "" is mdp_future_create.  One name:
 *   MDP_FUT_WIDE=0     (default) the lane kernels k_future<NM> only: one
 *                      replicate per lane, n <= 64, more is MDP_EUNSUPPORTED
 *   MDP_FUT_WIDE=auto  k_future<NM> for n <= 64, the patch-parallel
 *                      k_future_wide<NP> (one replicate per wave, the patches
 *                      over its lanes) for 65 <= n <= 1024
 *   MDP_FUT_WIDE=1     k_future_wide<NP> for every 1 <= n <= 1024 (the
 *                      kernel-variant switch of the tests)
 * Both kernels draw from the same addressed stream and add the same terms in
 * the same order: the counts do not depend on the kernel.  An unknown name or
 * value is MDP_EINVAL, n > 1024 MDP_EUNSUPPORTED under every setting; <= 30
 * missing patches, tfut <= 12288 and the 65536-replicate look-back hold for
 * both.  Every refusal comes before the first device call.  simulate,
 * simulate_device, check and time_kernel take either kind of engine. */
int mdp_future_create_opts(const int32_t *last_row, uint32_t n, const double *post, uint32_t necstep, double m,
                           double d, double KD, double KS, double dS, int device, const char *opts,
                           mdp_future **out);
/* Name of the simulation kernel the engine launches, e.g. "k_future<16>" or
 * "k_future_wide<2>" (owned by the engine). */
const char *mdp_future_kernel(const mdp_future *future);
/* The ensemble itself: words[r*W + k/64] bit k%64 = patch k occupied after
 * tfut years in replicate rep0 + r, r < nrep, W = ceil(n/64) (overwritten;
 * host memory).  tfut = 0 gives the completion of the last survey each
 * replicate starts from.  Engines running k_future_wide only (the lane
 * kernels keep no state: MDP_EUNSUPPORTED); nrep * W above 2^20 words per
 * call is MDP_EUNSUPPORTED. */
int mdp_future_states(mdp_future *future, uint64_t seed, uint64_t rep0, uint64_t nrep, uint32_t tfut,
                      uint64_t *words);

/* Also added after ABI 9 without a version bump: the ensemble's summaries.
 * For replicates r in [rep0, rep0 + nrep) and years t < tfut, on the same
 * addressed stream (and so the same trajectories) as mdp_future_simulate:
 *   hist[t*(n+1) + m] += replicates with exactly m occupied patches after
 *                        year t+1, m = 0..n   (hist[t][0] is counts[t])
 *   occ[t*n + k]      += replicates with patch k occupied after year t+1
 * Host memory; either table may be NULL, not both.  Both kinds of engine.
 * The tables are counted in LDS over windows of years (one launch per window,
 * the replicates resting in device records in between) with integer atomics:
 * exact, the same bits for every split and window length.  tfut outside
 * 1..12288 or tfut*(2n+1) > 2^21 cells is MDP_EUNSUPPORTED, both tables NULL
 * MDP_EINVAL, before any device call.  The look-back overflow is reported as
 * by mdp_future_simulate.
 * One more option of mdp_future_create_opts:
 *   MDP_FUT_SUM_YEARS=N  at most N years per window (0 or unset: the engine's
 *                        choice, what fits 16 KB of LDS); any other value than
 *                        0..12288 is MDP_EINVAL.  The window-boundary switch
 *                        of the tests; the tables do not depend on it. */
int mdp_future_summary(mdp_future *future, uint64_t seed, uint64_t rep0, uint64_t nrep, uint32_t tfut,
                       uint64_t *hist, uint64_t *occ);
/* Same into caller-owned device memory (overwritten, not accumulated) on
 * `stream`, asynchronously; the look-back flag is the sticky one of
 * mdp_future_simulate_device, read by mdp_future_check. */
int mdp_future_summary_device(mdp_future *future, uint64_t seed, uint64_t rep0, uint64_t nrep, uint32_t tfut,
                              uint64_t *d_hist, uint64_t *d_occ, void *stream);
/* Mean duration (ms) of the summary path (every window's launch and the
 * table's reset) over `reps` runs of replicates [0, nrep) between two events. */
int mdp_future_time_summary(mdp_future *future, uint64_t seed, uint64_t nrep, uint32_t tfut, int reps, double *ms);

/* Device-resident form of mdp_scenario_lik (one process per GPU): upload the
 * grid once (set_grid; ts, tdis and the axes as above), then compute into
 * caller-owned device memory d_out[ne*nc*nK*nd] (same layout) on `stream`
 * (NULL = HIP's null stream), asynchronously.  time_kernels: ms[0] =
 * mean duration of the v = P^tdis w kernel, ms[1] = of the PK^ts kernel,
 * each launched `reps` times back to back between two events. */
int mdp_scenario_set_grid(mdp_scenario *scenario, int ts, int tdis, const double *e, uint32_t ne, const double *c,
                          uint32_t nc, const double *K, uint32_t nK, const double *dsrc, uint32_t nd);
int mdp_scenario_run(mdp_scenario *scenario, double *d_out, void *stream);
int mdp_scenario_time_kernels(mdp_scenario *scenario, double *d_out, void *stream, int reps, double *ms);

/* ------------------------------------------------------------------ */
/* Simulated scenario likelihoods for rows of up to 1024 patches        */
/* (Rscript/simuls_traj.R, simtrajH1 / simtrajH2)                       */
/* ------------------------------------------------------------------ */

/* Also added after ABI 9 without a version bump.  The two hypotheses of
 * mdp_scenario_lik by Monte Carlo, for first survey rows beyond the 16 patches
 * of the exact engine (and any smaller one).  A replicate draws a uniform
 * initial state over the 2^n, runs ts years under the scenario (kind 0
 * die-off: E = e/K, pC = (c s1) K; kind 1 loss: E = e, pC = c (s1 + src K))
 * and tdis baseline years (E = e, pC = c s1), and its final state is tallied:
 *   L = 2^n E[prior(final) 1{final compatible with the row}]
 * exactly in expectation.  Draws are Philox4x32-10 keyed by `seed`, addressed
 * by (replicate, year, patch pair) as in the future engine.  The initial
 * state: patch k is occupied iff bit k & 31 of word (k >> 5) & 3 of
 * philox(seed; rep_lo, rep_hi, 0xffffffff, 1 + (k >> 7)) is set -- one
 * counter per 128 patches, {.., 0xffffffff, 1} for the first (for k < 64 the
 * definition the lane kernel has always had).  Counter word 3 >= 1 under word
 * 2 = 0xffffffff meets neither a year's draws (word 2 = t <= 12287) nor the
 * future engine's {.., 0xffffffff, 0}.  The grid point is not in the
 * counter, so every point sees the same replicates (common random numbers)
 * and no result depends on how replicates or points are split, nor on the
 * kernel that runs them.
 *
 * create: row, n, m, p, d, kind as mdp_scenario_create; 1 <= n <= 64, or
 * <= 1024 under MDP_SIM_WAVE.  No device call is made before the first
 * computing call, and every refusal of every call comes before its first
 * device call.  Options:
 *   MDP_SIM_WAVE=0|auto|1   the kernel family.  0 (default): the lane kernel
 *                           k_scnsim<NM>, one replicate per lane, n <= 64.
 *                           auto: k_scnsim<NM> for n <= 64, the patch-parallel
 *                           k_scnsim_wave<NP> (one replicate per wave, NP =
 *                           1, 2, 4, 8 patch pairs per lane for n <= 128,
 *                           256, 512, 1024) beyond.  1: k_scnsim_wave<NP> for
 *                           every n <= 1024.  Same tables where both run.
 * and the test hooks
 *   MDP_SIM_NM=8|16|32|64   the instantiation k_scnsim<NM>, at least the one
 *                           n needs (the smallest NM >= n); smaller, or with
 *                           a wave kernel selected: MDP_EINVAL
 *   MDP_SIM_NP=1|2|4|8      the instantiation k_scnsim_wave<NP>, at least the
 *                           one n needs; smaller, or with a lane kernel
 *                           selected: MDP_EINVAL
 *   MDP_SIM_LAUNCH_PTS=N    at most N grid points per launch (0: no cap)
 * Refusals: MDP_EINVAL for n = 0, a row value outside {-1, 0, 1}, both
 * tables NULL, ts < 0 or tdis < 0, a negative or non-finite e, c or dsrc, a K
 * that is not finite and > 0, an unknown option name or value;
 * MDP_EUNSUPPORTED for n > 64 (n > 1024 under MDP_SIM_WAVE=auto or 1), `match`
 * with more than 10 missing patches, ts + tdis > 12288, more than 2^20 grid
 * points or 2^24 cells in a table, nrep > 2^31 per call.
 *
 * Past 64 patches `match` is a weak statistic under a uniform start: a
 * replicate matches n observed patches with probability near 2^-n, so the
 * table is empty for any feasible nrep unless the scenario itself drives the
 * state to the row.  `hist` (read through the share of replicates ending at
 * the observed count, Rscript/simuls_traj.R) stays informative. */
typedef struct mdp_scenario_sim mdp_scenario_sim;
int mdp_scenario_sim_create(const int32_t *row, uint32_t n, double m, float p, double d, int kind, int device,
                            const char *options, mdp_scenario_sim **out);
void mdp_scenario_sim_destroy(mdp_scenario_sim *sim);
/* "k_scnsim<32>" or "k_scnsim_wave<2>" (owned by the engine) */
const char *mdp_scenario_sim_kernel(const mdp_scenario_sim *sim);
/* Over replicates [rep0, rep0 + nrep) and the grid points g = ((ie*nc + ic)*nK
 * + iK)*nd + id (the layout of mdp_scenario_lik; nd = 1 and dsrc ignored for
 * kind 0), G = ne*nc*nK*nd:
 *   hist[g*(n+1) + m]       += replicates with m occupied patches at the end
 *   match[(g << nmiss) + j] += replicates whose final state is completion j
 *                              of the row (the first missing patch is the
 *                              MSB of j, dieoff.c:205-232)
 * Host memory, 64-bit counts; either table may be NULL, not both. */
int mdp_scenario_sim_tables(mdp_scenario_sim *sim, int ts, int tdis, const double *e, uint32_t ne, const double *c,
                            uint32_t nc, const double *K, uint32_t nK, const double *dsrc, uint32_t nd, uint64_t seed,
                            uint64_t rep0, uint64_t nrep, uint64_t *hist, uint64_t *match);
/* Same into caller-owned device memory (overwritten, not accumulated); the
 * launches are asynchronous on `stream` (NULL = HIP's null stream), after the
 * grid has been uploaded -- which waits for the device when an earlier
 * device-form call of this simulator is still pending (Conventions, Streams),
 * and for nothing otherwise. */
int mdp_scenario_sim_tables_device(mdp_scenario_sim *sim, int ts, int tdis, const double *e, uint32_t ne,
                                   const double *c, uint32_t nc, const double *K, uint32_t nK, const double *dsrc,
                                   uint32_t nd, uint64_t seed, uint64_t rep0, uint64_t nrep, uint64_t *d_hist,
                                   uint64_t *d_match, void *stream);
/* out[g] = (sum_j (double)prior_j * (double)match[g][j], j ascending) * 2^n
 * / nrep, prior_j the float prior of completion j (dieoff.c:230).  For
 * n > 64 the mean is scaled, ldexp(sum / nrep, n): 0 for a zero sum and never
 * NaN (2^1024 is not a double), the same value wherever the first form is
 * finite.  Host. */
int mdp_scenario_sim_lik(const mdp_scenario_sim *sim, const uint64_t *match, size_t npoints, uint64_t nrep,
                         double *out);
/* Mean duration (ms) of `reps` runs of the call's launches over replicates
 * [0, nrep) (hist, and match when the row has <= 10 missing patches). */
int mdp_scenario_sim_time_kernel(mdp_scenario_sim *sim, int ts, int tdis, const double *e, uint32_t ne,
                                 const double *c, uint32_t nc, const double *K, uint32_t nK, const double *dsrc,
                                 uint32_t nd, uint64_t seed, uint64_t nrep, int reps, double *ms);

/* ------------------------------------------------------------------ */
/* Count-class chain likelihoods for rows of up to 64 patches           */
/* (Rscript/simuls_traj.R, simtrajH11 / simtrajH21)                     */
/* ------------------------------------------------------------------ */

/* Also added after ABI 9 without a version bump.  The estimator behind the
 * reference's 26-segment figures: instead of whole trajectories, ONE simulated
 * year from a random start with exactly k occupied patches, for every class
 * k = 0..n, tallied into the (n+1) x (n+1) matrix of transitions between
 * occupied-count classes -- A for a scenario year, B for a baseline year --
 * and the likelihood read off the matrix powers,
 *   out[g] = sum_k start[k] [A_g^ts B^tdis target]_k,
 * which carry probabilities far below 1/nrep.  Lumping the 2^n states into
 * n+1 classes is exact when the patches are exchangeable (d = 0, and for loss
 * a source at distance 0) and an approximation otherwise.  Unlike
 * the R script, class 0 is simulated like every other class: under habitat
 * loss the source recolonises an empty row.
 *
 * The replicate model, per table (scenario: points g = ((ie*nc + ic)*nK +
 * iK)*nd + id; baseline: g = ie*nc + ic), class k and replicate rg = rep0 + r:
 *   start state  exactly k patches by selection sampling: need = k; for
 *                j = 0..n-1 ascending, u_j = word j & 3 of philox(seed;
 *                rg_lo, rg_hi, 0xfffffffe, 16*k + (j >> 2)); patch j is
 *                occupied iff ((uint64)u_j * (n - j)) >> 32 < need, and then
 *                need -= 1.  Counter word 2 = 0xfffffffe meets neither a
 *                year's draws (word 2 = t <= 12287) nor the initial states of
 *                the simulator and the future engine (0xffffffff).
 *   one year     the simulator's year with year word t = k: pair m =
 *                patch >> 1 draws philox(seed; rg_lo, rg_hi, k, m), words
 *                2(p&1) and 2(p&1)+1 the extinction and colonisation draws.
 *                The classes use disjoint draws; the grid point is not in
 *                the counter, so every point shares its replicates.
 *   rates        scenario table: mdp_scenario_sim's scenario year (die-off
 *                E = min(1, e/K), pC = (c s1) K; loss E = min(1, e), pC =
 *                c (s1 + src K)); baseline table: E = min(1, e), pC = c s1.
 *   tally        cnt[(g*(n+1) + k)*(n+1) + l] += 1, l the number of occupied
 *                patches after the year.
 * No count depends on how replicates, classes or points are split over calls,
 * launches, workgroups or GPUs, nor on the kernel instantiation.
 *
 * The evaluation, with a[k][l] = (double)cnt_scn / (double)nrep and b[k][l] =
 * (double)cnt_base / (double)nbase: v = target; tdis times v'[k] = sum_l
 * b[k][l] v[l]; ts times v'[k] = sum_l a[k][l] v[l]; by_class[g][k] = v[k];
 * out[g] = sum_k start[k] v[k].  Every sum ascending from 0.0, each product
 * rounded before its add.  Defaults (NULL): start[k] = 1/(n+1), the script's
 * mean(Pf[, m+1]); target[n1 + j] = (C(nmiss, j) p^j) (1-p)^(nmiss-j) with p
 * = (double)(float)p, n1 the observed 1s and nmiss the -1s of the row.
 * start[k] = C(n, k) is the weighting under which exchangeable patches
 * reproduce sum over the rows with the target's count of mdp_scenario_lik.
 *
 * create: row, n, m, p, d, kind, device as mdp_scenario_sim_create; 1 <= n <=
 * 64.  No device call is made before the first computing call, and every
 * refusal of every call comes before its first device call.  Options (test
 * hooks; no result depends on them):
 *   MDP_CHAIN_NM=8|16|32|64   the instantiation k_scnchain<NM>, at least the
 *                             one n needs; smaller: MDP_EINVAL
 *   MDP_CHAIN_LAUNCH_PTS=N    grid points per launch (0: the planner's cut,
 *                             a device count table of at most 256 MiB)
 *   MDP_CHAIN_PARTS=N         workgroups that share a grid point, each
 *                             flushing its own tally (0: the planner's choice)
 * Refusals: MDP_EINVAL for n = 0, a row value outside {-1, 0, 1}, an unknown
 * option name or value, ts < 0 or tdis < 0, a negative or non-finite e, c or
 * dsrc, a K that is not finite and > 0, a negative or non-finite weight,
 * nrep = 0 or nbase = 0 in eval / lik; MDP_EUNSUPPORTED for n > 64, ts + tdis >
 * 12288, more than 2^20 grid points, nrep or nbase > 2^31, and for counts a
 * table of more than 2^24 cells. */
typedef struct mdp_scenario_chain mdp_scenario_chain;
int mdp_scenario_chain_create(const int32_t *row, uint32_t n, double m, float p, double d, int kind, int device,
                              const char *options, mdp_scenario_chain **out);
void mdp_scenario_chain_destroy(mdp_scenario_chain *chain);
/* "k_scnchain<32>" (owned by the engine) */
const char *mdp_scenario_chain_kernel(const mdp_scenario_chain *chain);
/* the default target[n+1] */
int mdp_scenario_chain_target(const mdp_scenario_chain *chain, double *target);
/* cnt += the counts of replicates [rep0, rep0 + nrep) per class: the scenario
 * table [ne*nc*nK*nd][n+1][n+1], or (baseline != 0; K, nK, dsrc and nd are
 * ignored) the baseline table [ne*nc][n+1][n+1].  Host memory, 64-bit counts. */
int mdp_scenario_chain_counts(mdp_scenario_chain *chain, int baseline, const double *e, uint32_t ne, const double *c,
                              uint32_t nc, const double *K, uint32_t nK, const double *dsrc, uint32_t nd, uint64_t seed,
                              uint64_t rep0, uint64_t nrep, uint64_t *cnt);
/* The evaluation on host tables of nrep and nbase replicates per class:
 * out[ne*nc*nK*nd], by_class[ne*nc*nK*nd][n+1] (may be NULL).  Host
 * arithmetic: no device call. */
int mdp_scenario_chain_eval(const mdp_scenario_chain *chain, int ts, int tdis, uint32_t ne, uint32_t nc, uint32_t nK,
                            uint32_t nd, const uint64_t *cnt_scn, uint64_t nrep, const uint64_t *cnt_base,
                            uint64_t nbase, const double *start, const double *target, double *out, double *by_class);
/* Counts (rep0 = 0) and evaluation on the device, the result in host memory:
 * the bits mdp_scenario_chain_eval returns on mdp_scenario_chain_counts'
 * tables.  The count tables stay on the device, cut into launches. */
int mdp_scenario_chain_lik(mdp_scenario_chain *chain, int ts, int tdis, const double *e, uint32_t ne, const double *c,
                           uint32_t nc, const double *K, uint32_t nK, const double *dsrc, uint32_t nd, uint64_t seed,
                           uint64_t nrep, uint64_t nbase, const double *start, const double *target, double *out,
                           double *by_class);
/* Same into caller-owned device memory d_out[ne*nc*nK*nd] (overwritten); the
 * launches are asynchronous on `stream` (NULL = HIP's null stream), after the
 * grid has been uploaded -- which waits for the device when an earlier
 * device-form call of this engine is still pending (Conventions, Streams). */
int mdp_scenario_chain_lik_device(mdp_scenario_chain *chain, int ts, int tdis, const double *e, uint32_t ne,
                                  const double *c, uint32_t nc, const double *K, uint32_t nK, const double *dsrc,
                                  uint32_t nd, uint64_t seed, uint64_t nrep, uint64_t nbase, const double *start,
                                  const double *target, double *d_out, void *stream);
/* Mean durations (ms) over `reps` runs: ms[0] the baseline counts, ms[1] the
 * scenario counts (each with its table's reset), ms[2] both evaluations. */
int mdp_scenario_chain_time_kernels(mdp_scenario_chain *chain, int ts, int tdis, const double *e, uint32_t ne,
                                    const double *c, uint32_t nc, const double *K, uint32_t nK, const double *dsrc,
                                    uint32_t nd, uint64_t seed, uint64_t nrep, uint64_t nbase, int reps, double *ms);

/* Thread-local description of the last error. */
const char *mdp_last_error(void);

int mdp_abi_version(void);

/* Number of visible HIP devices (0 when none); the CLIs use it to deal work
 * over GPUs. */
int mdp_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* MIDASPOM_H */
