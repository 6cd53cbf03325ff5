/*
 * hdpm.h -- C ABI of the MI355X-native Neal-8 / split-merge reassignment engine.
 *
 * Drop-in boundary for the hot path of Filippo-Galli/Split_and_merge_Gibbs_sampling.
 * The reference exposes this path as in-process C++ calls behind one Rcpp export; each
 * entry point below names the reference interface it replaces.  An Rcpp adapter that
 * keeps the reference's R-facing signature is given in INTEGRATION.md.
 *
 * Conventions
 *   - The caller owns every host buffer; the context owns device memory.
 *   - Every call returns an int status (HDPM_OK = 0); hdpm_last_error() describes it.
 *     No C++ exception crosses this boundary.
 *   - One context per host thread per GPU.  The library never calls the R API.
 *   - The R random stream (Mersenne-Twister, the 625 words of .Random.seed after the
 *     kind word) lives in the context and is consumed in the reference's order; it can
 *     be set and read back explicitly.
 *   - Categorical data are codes 1..m_j (the reference's NumericMatrix values).
 *     `codes` is row-major N x D uint8; `centers` are K x D doubles (integer-valued, as
 *     the reference's NumericVector centers), `sigma` K x D doubles.
 */
#ifndef HDPM_H
#define HDPM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HDPM_OK          0
#define HDPM_E_VALIDATE  1  /* validate_state failed -> Rcpp::stop in the reference      */
#define HDPM_E_GSL       2  /* norm_const2 threw (GSL 2F1 overflow)                         */
#define HDPM_E_PROB      3  /* FixupProb stop(): no positive / non-finite probability      */
#define HDPM_E_WALKER    4  /* Walker alias table (Rcpp sample, > 200 categories) failed  */
#define HDPM_E_ARG       5  /* invalid argument or capacity                                 */
#define HDPM_E_DEVICE    6  /* HIP runtime error                                            */
#define HDPM_E_NODEVICE  7  /* no usable gfx950 device                                      */

typedef struct hdpm_ctx hdpm_ctx;

/* Parameters of run_markov_chain (code/launcher.cpp:7-14), same names and meaning. */
typedef struct {
    int32_t verbose, m, iterations, L, burnin, t, r;
    int32_t neal8, split_merge, n8_step_size, sam_step_size, thinning;
} hdpm_chain_params;

/* Per-context counters (cumulative since hdpm_ctx_create or hdpm_reset_stats). */
typedef struct {
    int64_t sweeps, rounds, restarts, exact_points, moves, checked_rounds, prepass_points;
    double  t_prepass_ms, t_resolve_ms, t_stats_ms, t_host_phi_ms, t_rng_ms, t_loglik_ms, t_exact_ms;
    /* latent pool generation (la:74-77, 124-128): calls, entries, wall time, and for the
     * device generator its phases: stream slice, attempt tables, host walk, values */
    int64_t pool_calls, pool_entries, pool_device_calls;
    double  t_pool_ms, t_pool_mt_ms, t_pool_accept_ms, t_pool_parse_ms, t_pool_values_ms;
    /* update_phi speculated while the device sweeps: passes run, and clusters whose
     * speculative draws were kept (the sweep left them untouched) */
    int64_t phi_spec_runs, phi_spec_clusters;
    /* prepass launches timed with HIP events (every 8th; t_prepass_ms covers these) and
     * their points */
    int64_t prepass_timed, prepass_timed_points;
    /* device random-stream windows generated: all, and those started from the host state
     * (a window that did not cover the next draws) */
    int64_t rng_windows, rng_windows_fresh;
    /* points the prepass could not prove "stay" (exact rows built for them) */
    int64_t listed_points;
    /* split-merge moves (sm:542-598): count, wall time, and its parts: restricted scans
     * on the device (upload + kernels + wait), update_phi draws, acceptance terms */
    int64_t sm_moves;
    double  t_sm_ms, t_sm_scan_ms, t_sm_phi_ms, t_sm_terms_ms;
    /* update_phi on the device (csrc/phi.hip): updates committed there, and updates it
     * handed back to the host (a case it does not restate: Walker, rhig's bisection path, a
     * drift outside its window, ...); the status of the last one (PhiStatus, 0 = ok).  One
     * update_phi counts once: a speculated update that did not complete and was run again
     * counts as what the second run did (its status stays in phi_fallback_status_mask) */
    int64_t phi_device_calls, phi_device_fallbacks, phi_device_last_status;
    /* update stream slices found in a copy made an iteration ahead, and such copies made */
    int64_t phi_lookahead_hits, phi_lookahead_copies;
    /* next sweeps enqueued before the iteration's update was joined, and those that ran;
     * go decisions refused because the wait kernel's limit was near (the sweep ran
     * unpipelined), and enqueued sweeps gated off on the device and re-run from point 0 */
    int64_t pipe_enqueued, pipe_runs, pipe_refused, pipe_recovered;
    /* device update_phi by composition trees (every pick fixed), and tree-mode updates re-run
     * by the per-start-drift walks (a pick depended on the uniform) */
    int64_t phi_tree_calls, phi_tree_retries;
    /* device pool generations whose entry starts fell back to the sequential host walk (the
     * segment parse's chain left a window: an entry longer than mean + 14 sd; or HDPM_DBG_POOL_SERIAL_PARSE) */
    int64_t pool_walk_fallbacks;
    /* update_phi speculated on the device beside the sweep (phi_mode device): launched, and
     * committed as the iteration's update (the sweep moved no point) */
    int64_t phi_dspec_launched, phi_dspec_used;
    /* resolver launches by the device-wide fixed-point resolver (k_resolve_fpg) */
    int64_t fpg_launches;
    /* split-merge update_phi calls (sm:221, 387, 584) run on the device */
    int64_t phi_sm_device_calls;
    /* bit s set: a device update_phi was handed back with PhiStatus s (bit 15: the status was
     * ok but the stream position could not be adopted) */
    int64_t phi_fallback_status_mask;
    /* split-merge device updates re-run with a wider drift window (the drift left the first) */
    int64_t phi_sm_window_retries;
    /* k_resolve_fpg launches that gave up at a grid barrier (a workgroup not resident within the
     * limit, HDPM_OPT_FPG_WAIT_US) and were continued from their first undecided point by the
     * one-workgroup resolver */
    int64_t fpg_aborts;
    /* exact-row launches by the mass kernels: a wave per point (k_exact_rows_mass) and a thread
     * per point (k_exact_rows_lanes) */
    int64_t exact_mass_launches, exact_lanes_launches;
    /* launches that listed every point (a context's first launch, or more than half the points
     * expected uncertain: a chain far from convergence) */
    int64_t dense_launches;
    /* split-merge restricted scans walked on many CUs (k_sm_scan_wide), and those that gave up
     * (grid not resident) and ran on one workgroup */
    int64_t sm_wide_scans, sm_wide_fallbacks;
    /* device update_phi calls enqueued on the fast path (csrc/phi.hip launch_phi2: every pick
     * fixed, no copies), and those of them handed to the general kernels or the host */
    int64_t phi_fast_calls, phi_fast_handbacks;
    /* recorded iterations' labels (hdpm_iterations_record, la:145): taken from the host mirror
     * with the sweep's move log applied (12 B per moved point), and downloaded whole (N words) */
    int64_t labels_mirrored, labels_downloaded;
    /* device updates whose stream state came back with their outputs (k_phi2_values copies the
     * block of the position after the draws; no state copy to wait for) */
    int64_t phi_state_direct;
    /* chained device updates (the next iteration's, enqueued behind the current speculation
     * before it ran): launched, committed, and dropped at the go (the update before them was not
     * the one committed) */
    int64_t phi_chain_launched, phi_chain_used, phi_chain_dropped;
    /* sweeps enqueued ahead that the device started itself (k_pipe_wait's own go behind a
     * completed device update, no host round trip), and goes the host could not follow (the
     * chain state is then undefined and the context reports an error; never expected) */
    int64_t pipe_auto, pipe_desync;
    /* restricted Gibbs samplers run as one device chain (every scan, its table update and its
     * update_phi({c1, c2}) enqueued together, sm:163-225): chains, scans run in them, and chains
     * the host continued from their first unfinished scan or update (an update the device handed
     * back, a draw outside the stream window) */
    int64_t sm_chain_runs, sm_chain_scans, sm_chain_resumes;
    /* the early conditional go of the host update's pipeline: goes the host gave for a sweep
     * enqueued ahead at the join of the speculated update, before the running sweep had ended
     * (the wait kernel then decides from that sweep's control block, no host round trip);
     * those behind which the device went, and those it declined (the running sweep moved
     * points or needed another launch: the enqueued kernels gated themselves off).
     * pipe_early == pipe_early_ran + pipe_early_off.  HDPM_PIPE_EARLY=0 in the environment
     * (read once per process) leaves every go to the sweep's end, for A/B runs. */
    int64_t pipe_early, pipe_early_ran, pipe_early_off;
    /* rounds of sweeps enqueued ahead whose end the host took from the control block's sequence
     * word (ResolveCtl::seq) instead of an event behind the resolver.  HDPM_RES_WORD=0 in the
     * environment (read once per process) keeps the event. */
    int64_t resolved_by_word;
} hdpm_stats;

int         hdpm_device_count(void);
int         hdpm_ctx_create(int32_t device, hdpm_ctx** out);
void        hdpm_ctx_destroy(hdpm_ctx* ctx);
const char* hdpm_last_error(const hdpm_ctx* ctx);

/* aux_data (code/common_functions.hpp:65-72): data, n, attrisize, gamma, v, w. */
int hdpm_set_data(hdpm_ctx* ctx, const uint8_t* codes, int32_t n, int32_t d, const int32_t* attrisize,
                  double gamma, const double* v, const double* w);

/* R RNG: set.seed(seed) semantics, or the 625-word state (mti, mt[624]). */
int hdpm_rng_set_seed(hdpm_ctx* ctx, uint32_t seed);
int hdpm_rng_set_state(hdpm_ctx* ctx, const int32_t* state625);
int hdpm_rng_get_state(const hdpm_ctx* ctx, int32_t* state625);

/* internal_state (code/common_functions.hpp:32-63): c_i (labels 0..K-1), centers, sigma. */
int hdpm_set_state(hdpm_ctx* ctx, const int32_t* c_i, int32_t K, const double* centers, const double* sigma);
int hdpm_get_state(hdpm_ctx* ctx, int32_t* c_i, int32_t* K, double* centers, double* sigma, int32_t cap);

/* Latent-parameter pool (code/launcher.cpp:67-77): P entries of (center, sigma). */
int hdpm_set_pool(hdpm_ctx* ctx, const double* centers, const double* sigma, int64_t P);
int hdpm_get_pool(hdpm_ctx* ctx, double* centers, double* sigma, int64_t P);
/* Draw P prior entries from the context stream exactly as la:74-77 / la:124-128. */
int hdpm_generate_pool(hdpm_ctx* ctx, int64_t P);

/* One Neal-8 sweep: N calls of sample_allocation (code/neal8.hpp:4-5, neal8.cpp:10-160)
 * in index order, i.e. the loop code/launcher.cpp:95-99.  Consumes m+1 uniforms/point. */
int hdpm_neal8_sweep(hdpm_ctx* ctx, int32_t m);

/* update_phi (code/common_functions.hpp:113, .cpp:511-591); idx == NULL -> all clusters. */
int hdpm_update_phi(hdpm_ctx* ctx, const int32_t* cluster_indexes, int32_t n_idx);

/* compute_loglikelihood (code/common_functions.hpp:105, .cpp:379-401). */
int hdpm_compute_loglikelihood(hdpm_ctx* ctx, double* out);

/* The N x K log-likelihood matrix and integer Hamming counts against the current
 * clusters (code/neal8.cpp:40-50 inner loop), L[i*K+k], H[i*K+k]. */
int hdpm_loglik_matrix(hdpm_ctx* ctx, double* L, int32_t* H);

/* split_restricted_gibbs_sampler (code/split_merge.hpp:13, .cpp:163-225) on the state. */
int hdpm_restricted_gibbs(hdpm_ctx* ctx, const int32_t* S, int32_t nS, int32_t i1, int32_t i2, int32_t t);

/* logprobgs_c_i (code/split_merge.hpp:11, .cpp:96-161): gamma_star = context state,
 * gamma = launch labels g_c_i. */
int hdpm_logprobgs_c_i(hdpm_ctx* ctx, const int32_t* g_c_i, const int32_t* S, int32_t nS, int32_t i1,
                       int32_t i2, double* out);

/* split_and_merge (code/split_merge.hpp:217-219, .cpp:542-598). */
int hdpm_split_and_merge(hdpm_ctx* ctx, int32_t t, int32_t r, int32_t idx_1_sm, int32_t* accepted);

/* run_markov_chain (code/launcher.cpp:6-174).  c_i_init may be NULL (random init with L
 * labels).  Output buffers (any may be NULL): out_total_cls[iterations],
 * out_c_i[iterations * n], out_loglik[iterations], out_accepted[iterations], final_ass[n];
 * out_time_s = wall seconds of the sampling loop (results$time). */
int hdpm_run_markov_chain(hdpm_ctx* ctx, const hdpm_chain_params* p, const int32_t* c_i_init,
                          int32_t* out_total_cls, int32_t* out_c_i, double* out_loglik,
                          int32_t* out_accepted, int32_t* final_ass, double* out_time_s);

/* The two halves of run_markov_chain, for callers that drive the loop themselves:
 * hdpm_init_chain = la:27-77 (initial labels, centers, sigmas, update_phi, latent pool of
 * n*m*thinning entries); hdpm_iteration = one pass of the loop body la:85-132 for
 * iteration `iter` (Neal-8 sweep + update_phi, split-merge, pool regeneration when
 * iter % 1000 == 0, compute_loglikelihood).  idx_1_sm is carried by the caller. */
int hdpm_init_chain(hdpm_ctx* ctx, const hdpm_chain_params* p, const int32_t* c_i_init);
int hdpm_iteration(hdpm_ctx* ctx, const hdpm_chain_params* p, int32_t iter, int32_t* idx_1_sm,
                   int32_t* accepted, double* loglik);
/* `count` consecutive iterations iter0 .. iter0+count-1 (accepted / loglik: count entries
 * each, may be NULL).  Same chain as calling hdpm_iteration for each; between two
 * iterations of the batch the next sweep is launched on the device before this call's
 * host work for the current one is done (the loop of la:85-154 without R in between). */
int hdpm_iterations(hdpm_ctx* ctx, const hdpm_chain_params* p, int32_t iter0, int32_t count, int32_t* idx_1_sm,
                    int32_t* accepted, double* loglik);

/* hdpm_iterations with the saved iterations recorded (la:139-153, the R driver's sampling phase):
 * iteration iter is saved when iter >= thinning * burnin and iter % thinning == 0; the s-th saved
 * iteration of this call writes total_cls[s] (K), c_i[s * n .. s * n + n) (its labels; may be
 * NULL), and appends its K x d centers and sigmas (doubles, as hdpm_get_state) to the context's
 * record, taken with hdpm_record_take.  *nsaved: saved iterations of this call.  Unlike
 * hdpm_get_state between hdpm_iteration calls, nothing is dropped: the next sweep stays
 * pipelined, and a label vector comes from the host's mirror of the labels (kept across sweeps
 * without moves, updated from the sweep's move log otherwise) instead of an N-word download. */
int hdpm_iterations_record(hdpm_ctx* ctx, const hdpm_chain_params* p, int32_t iter0, int32_t count, int32_t* idx_1_sm,
                           int32_t* accepted, double* loglik, int32_t* total_cls, int32_t* c_i, int32_t* nsaved);
/* The recorded centers / sigmas (rows of d doubles, in saved-iteration order) appended since the
 * last take: *nrows is their number; with centers and sigmas non-NULL (nrows rows each) they are
 * copied out and the record is cleared. */
int hdpm_record_take(hdpm_ctx* ctx, double* centers, double* sigmas, int64_t* nrows);

/* Diagnostics / testing. */
/* Draw `count` raw 32-bit MT outputs (MT_genrand before scaling) on the device and advance
 * the context stream past them (same values as `count` host draws). */
int hdpm_rng_fill_device(hdpm_ctx* ctx, int64_t count, uint32_t* out);
int hdpm_get_stats(const hdpm_ctx* ctx, hdpm_stats* out);
int hdpm_reset_stats(hdpm_ctx* ctx);
/* The addends of the last split-merge move's log acceptance ratio (code/split_merge.cpp:438-540),
 * as the move computed them: a host-side record, filled by every move that reaches the
 * acceptance test (sm:591) -- through hdpm_split_and_merge, hdpm_iteration* or
 * hdpm_run_markov_chain alike -- and costing no kernel, copy or wait.  A move that returns an
 * error leaves kind = 0.  term[] holds the fourteen function values in the reference's source
 * order, unsigned (the signs belong to the formula).
 *   split (sm:438-487): 0 log(alpha); 1, 2 lgamma(n) of gamma_star's c(i1), c(i2); 3, 4
 *     priors(gamma_star, c(i1) / c(i2)); 5 lgamma(n) of gamma's c(i1); 6 priors(gamma, c(i1));
 *     7-9 the three loglikelihood_hamming calls; 10-12 the three logprobgs_phi calls;
 *     13 logprobgs_c_i.  size[] = the sizes under terms 1, 2, 5.
 *     log_prior = t0 + t1 + t2 + t3 + t4 - t5 - t6, log_likelihood = t7 + t8 - t9,
 *     log_proposal = t10 - t11 - t12 - t13.
 *   merge (sm:489-540): 0 lgamma(n) of gamma_star's c(i1); 1 priors(gamma_star, c(i1));
 *     2 log(alpha); 3, 4 lgamma(n) of gamma's c(i1), c(i2); 5, 6 priors(gamma, c(i1) / c(i2));
 *     7-9 loglikelihood_hamming; 10, 11 logprobgs_phi(gamma, launch, i1 / i2); 12 logprobgs_c_i;
 *     13 logprobgs_phi(gamma_star, merge launch, i2).  size[] = the sizes under terms 0, 3, 4.
 *     log_prior = t0 + t1 - t2 - t3 - t4 - t5 - t6, log_likelihood = t7 - t8 - t9,
 *     log_proposal = t10 + t11 + t12 - t13.
 * Each partial sum starts from 0.0 and adds left to right; log_ratio = log_prior +
 * log_likelihood + log_proposal; the move is accepted when log_u < min(0, log_ratio). */
typedef struct {
    int32_t kind;            /* 0: no completed move yet, 1: split (sm:438-487), 2: merge (sm:489-540) */
    int32_t accepted, i1, i2, nS;
    int32_t size[3];         /* the three cluster sizes whose lgamma enters, in the formula's order */
    double  term[14];        /* the addends as the functions return them, in the reference's source order */
    double  log_prior, log_likelihood, log_proposal;
    double  log_ratio;       /* the sum before min(0, .) */
    double  log_u;           /* log(unif) of sm:591 */
} hdpm_sm_terms;
int hdpm_sm_last_terms(const hdpm_ctx* ctx, hdpm_sm_terms* out);
/* Testing / diagnostics: the bits of hdpm_set_debug's mode.  Same chain with any of them; each
 * selects which path computes it.  Every effect the engine gives a bit is listed with it (a bit
 * that also gates a neighbouring path keeps its number: profiles and A/B records name the values).
 * Changing the mode drops a prepared next sweep. */
/* every point on the exact path (no certainty shortcut: every point listed, no certification by
 * the draw's uniform, no dense listing); the resolver decides each by the exact draw, one by
 * one: no block mode, no fixed-point resolver */
#define HDPM_DBG_EXACT_ALL               (1u << 0)
/* per-phase timings on stderr: host marks of hdpm_iteration, HIP events around every kernel of
 * every launch, the resolvers' own phase clocks, and the general device update_phi's drift
 * tables (read back with blocking copies) */
#define HDPM_DBG_PHASE_TIMES             (1u << 1)
/* the log-likelihood by the per-point kernel (no regrouping into match counts, not the device
 * update_phi's sum); the iteration then commits its tables before it prepares the next sweep */
#define HDPM_DBG_LL_PER_POINT            (1u << 2)
/* no snapshot speculation (the resolver decides every uncertain point itself); no dense listing */
#define HDPM_DBG_NO_SNAPSHOT             (1u << 3)
/* the frequency tables recounted for every update_phi (no incremental move log); hence no
 * update_phi speculated beside the sweep, on the host or the device, and no next sweep prepared */
#define HDPM_DBG_RECOUNT                 (1u << 4)
/* a host timeline of hdpm_iteration accumulated (printed to stderr when the context is
 * destroyed): host marks, the update job's waits and draw counts, and HIP events around every
 * kernel of every launch */
#define HDPM_DBG_TIMELINE                (1u << 5)
/* latent pools by the sequential host generator instead of the device one; also every device
 * update_phi off (the chain's, the one speculated beside the sweep, split-merge's) */
#define HDPM_DBG_HOST_POOL               (1u << 6)
/* no update_phi speculated during the sweep, on the host or beside it on the device, and a
 * speculation already made is not used; hence no next sweep prepared, no early go of a sweep
 * enqueued ahead; split-merge's host update of a wide pair (d >= 128) stays on the one-pass
 * path (cluster by cluster, no host job) */
#define HDPM_DBG_NO_SPEC_PHI             (1u << 7)
/* no next sweep prepared at the end of an iteration */
#define HDPM_DBG_NO_PREPARE              (1u << 8)
/* HIP events around every kernel of every launch (per-kernel times; by default the prepass of
 * every 8th launch only) */
#define HDPM_DBG_KERNEL_EVENTS           (1u << 9)
/* the prepass gathers full bound records for latent picks (no pool-entry heads); hence no latent
 * kept as a head bound by the exact rows */
#define HDPM_DBG_NO_POOL_HEADS           (1u << 10)
/* exact rows one wave per point (no workgroup-per-point LDS staging, no mass kernels); no dense
 * listing */
#define HDPM_DBG_EXACT_WAVE              (1u << 11)
/* no block mode in the resolver (uncertain points decided one by one) and no fixed-point
 * resolver; the host update job takes all of a cluster's logits before its first draw */
#define HDPM_DBG_NO_BLOCK_MODE           (1u << 12)
/* block mode for every resolver launch (not only after a launch that listed kResolveBlkMin
 * points); no fixed-point resolver */
#define HDPM_DBG_BLOCK_MODE_ALWAYS       (1u << 13)
/* wide layouts take the generic prepass (one thread per point) instead of k_prepass_wide */
#define HDPM_DBG_NO_WIDE_PREPASS         (1u << 14)
/* the prepared next sweep is launched before the speculative host update_phi is started */
#define HDPM_DBG_SWEEP_FIRST             (1u << 15)
/* restricted scans of >= 4096 points draw their uniforms on the host (not from the device
 * generator windows); also split-merge's device update_phi off */
#define HDPM_DBG_SM_HOST_DRAWS           (1u << 16)
/* a sweep prepared at the end of hdpm_iterations does not start its prepass on the device */
#define HDPM_DBG_NO_PREPASS_AHEAD        (1u << 17)
/* the prepass certifies "stay" by the margin only (not by the draw's uniform, kernels.hip
 * stay_by_uniform) */
#define HDPM_DBG_MARGIN_ONLY             (1u << 18)
/* update_phi on the host (the job speculated during the sweep) even when the device update is
 * selected (HDPM_OPT_PHI_DEVICE or HDPM_PHI=device; csrc/phi.hip), split-merge's included */
#define HDPM_DBG_PHI_HOST                (1u << 19)
/* no lookahead copy of the next update's stream slice (it is copied when the next sweep's draws
 * are reserved) */
#define HDPM_DBG_NO_LOOKAHEAD            (1u << 20)
/* the iteration commits the new tables and computes the log-likelihood before it prepares the
 * next sweep (by default the next speculative update_phi is started first); hence no next sweep
 * enqueued while the update is drawn */
#define HDPM_DBG_COMMIT_FIRST            (1u << 21)
/* no next sweep enqueued while the iteration's update is drawn (gated on the device,
 * k_pipe_wait) */
#define HDPM_DBG_NO_PIPE                 (1u << 22)
/* the one-wave resolvers (LIST mode, block mode after many exact decisions) instead of the
 * fixed-point resolver k_resolve_fp (which EXACT_ALL, NO_BLOCK_MODE and BLOCK_MODE_ALWAYS also
 * turn off) */
#define HDPM_DBG_ONE_WAVE_RESOLVER       (1u << 23)
/* with the fixed-point resolver too, a launch after one that decided many points itself lists
 * every point (no certification by the draw's uniform), as the one-wave resolvers always do */
#define HDPM_DBG_FP_LIST_ALL_AFTER_EXACT (1u << 24)
/* the fixed-point resolver for every launch it fits (by default a launch after one that listed
 * fewer than 64 points -- a converged chain -- takes the one-wave LIST resolver) */
#define HDPM_DBG_FP_ALWAYS               (1u << 25)
/* the fixed-point resolver's first round starts every point from "stay" instead of its snapshot
 * draw's outcome */
#define HDPM_DBG_FP_FROM_STAY            (1u << 26)
/* the device update_phi resolves its drifts by the per-start-drift walks (k_phi_cwalk) instead
 * of the composition trees (k_phi_tree); its fast path (launch_phi2) is not taken either */
#define HDPM_DBG_PHI_WALKS               (1u << 27)
/* the device pool generator's entry starts by the sequential host walk instead of the segment
 * parse (k_pool_seg*) */
#define HDPM_DBG_POOL_SERIAL_PARSE       (1u << 28)
/* the fixed-point resolver on one workgroup (k_resolve_fp) even after a launch that listed many
 * points (by default those take the device-wide k_resolve_fpg) */
#define HDPM_DBG_FP_ONE_WG               (1u << 29)
/* k_resolve_fpg for every fixed-point launch (testing: also the launches with few listed
 * points) */
#define HDPM_DBG_FPG_ALWAYS              (1u << 30)
int hdpm_set_debug(hdpm_ctx* ctx, int32_t mode);
/* The prepass's pool-entry heads, P entries of wb*Ws + 2 words padded to a power of two
 * (Ws <= 4) or to a multiple of 8 words (wide layouts) (csrc/kernels.hpp "Pool-entry heads",
 * head_stride); HDPM_E_ARG when the data's layout has none (Ws > 32, i.e. d > 2048, or rows
 * of more than 64 words: wb * Ws > 64). */
int hdpm_get_pool_heads(hdpm_ctx* ctx, uint64_t* out, int64_t P);
/* Options.  HDPM_OPT_HIG_LOGSPACE (value != 0): an extension beyond the reference -- the
 * HIG normalising constant's 2F1 series (norm_const2, hg:11-48, and lF_conK2, hg:183-217)
 * is summed with a rescaled partial sum, so clusters of thousands of members get a finite
 * log-density where GSL's double series overflows and the reference throws
 * (HDPM_E_GSL); 10^7 series terms instead of 30000.  Wherever the reference's series stays
 * finite within 30000 terms the values are bit-identical.  Default 0 (reference
 * semantics). */
#define HDPM_OPT_HIG_LOGSPACE 1
/* HDPM_OPT_PHI_DEVICE: where update_phi runs.  0: the host job speculated during the sweep;
 * 1: the device (csrc/phi.hip: center draws, rhig's beta-path sigma draws resolved over
 * acceptance masks by composition tables, tables and bound records; the fast path launch_phi2
 * first when every pick is fixed, else the general kernels); 2: the device's general kernels
 * only; 3 (default): automatic -- the device for the chain's update_phi of at least 4096
 * (cluster, attribute) items, where the host job's serial draws outlast the sweep, the host job
 * otherwise and for split-merge's updates.  Cases the device does not restate fall back to the
 * host.  Same chain either way.  HDPM_PHI=host|device|device-general|auto in the environment
 * sets the default. */
#define HDPM_OPT_PHI_DEVICE 2
/* HDPM_OPT_PIPE_WAIT_US (testing): the limit, in microseconds, after which the wait kernel of
 * a sweep enqueued ahead gives up and gates the sweep off (default 2 s).  A positive value
 * also makes the host refuse a go given after a quarter of the limit; a negative value sets
 * the limit to -value without that check, so the device-side gate-off (and the engine's
 * recovery from it: the sweep re-run ungated, same chain) can be exercised. */
#define HDPM_OPT_PIPE_WAIT_US 3
/* HDPM_OPT_CAPTURE_DELAY_US (testing, default 0): when hdpm_iterations_record has to read a saved
 * iteration's labels from device memory (the host mirror is invalid), the host sleeps this many
 * microseconds (at most 1e6) before it issues that read -- long enough for a sweep that went
 * ahead on the device to have finished, so a test sees whether the read is ordered before it.
 * Host-side only; same chain either way. */
#define HDPM_OPT_CAPTURE_DELAY_US 10
/* HDPM_OPT_FPG_WAIT_US: the limit, in microseconds, after which a grid barrier of the device-wide
 * resolver (k_resolve_fpg) gives up (default 2 s).  A launch that gives up has committed
 * exactly the windows before the barrier; it ends as a restart there and the engine continues
 * with the one-workgroup resolver (same chain; hdpm_stats.fpg_aborts counts these). */
#define HDPM_OPT_FPG_WAIT_US 4
/* HDPM_OPT_FPG_FAIL_AT (testing): workgroup 0 of every k_resolve_fpg launch gives up at its
 * value-th grid barrier (0: never), to exercise that recovery deterministically. */
#define HDPM_OPT_FPG_FAIL_AT 5
/* HDPM_OPT_EXACT_KERNEL (testing): the exact-rows kernel of launches with many listed points:
 * 0 automatic (default), 1 a wave per point (k_exact_rows_mass), 2 a thread per point with
 * compare / select (k_exact_rows_lanes), 3 a thread per point with level-indexed tables
 * (k_exact_rows_lv) -- where the state fits it.  Same chain either way. */
#define HDPM_OPT_EXACT_KERNEL 6
/* HDPM_OPT_LAT_NEGLIGIBLE (testing): the margin (>= 40, default 40) below the best cluster under
 * which a latent entry kept as a head bound by the exact rows counts as probability 0 in a draw;
 * above it the draw computes the latent's exact sum.  A large value sends every such latent to
 * the exact sum (the fallback path).  Same chain either way. */
#define HDPM_OPT_LAT_NEGLIGIBLE 7
/* HDPM_OPT_SM_WIDE_WAIT_US (testing): the grid-barrier limit of the split-merge scan on many CUs
 * (default 50000 us); a scan that gives up writes nothing and is walked on one workgroup
 * (hdpm_stats.sm_wide_fallbacks).  0 gives up at the first barrier, unconditionally; values above
 * 1e9 us are an argument error.  Same chain either way. */
#define HDPM_OPT_SM_WIDE_WAIT_US 8
/* HDPM_OPT_SM_CHAIN: the restricted Gibbs sampler of a split-merge move (sm:163-225, its t scans
 * and update_phi({c1, c2}) calls) as one device chain where it applies (1; also HDPM_SM_CHAIN=1
 * in the environment) or scan by scan with the host between them (0, the default: measured
 * faster at C3 and C4).  Testing:
 * 2 + 3k turns the chain off at scan k (the host continues from there), 3 + 3k / 4 + 3k hand the
 * scan's update of the lower / larger label back.  Same chain either way (hdpm_stats.sm_chain_*). */
#define HDPM_OPT_SM_CHAIN 9
/* HDPM_OPT_PHI_SD_SCALE (testing, default 1): a factor in [0, 1] on the standard-deviation term of
 * the device update_phi's drift windows (csrc/kernels.hpp phi_lo / phi_hi), on the fast path, the
 * composition trees and the walks, split-merge's updates and their wider re-runs included.  Below 1
 * the drift leaves the windows at ordinary sizes, so an update ends with a window status and goes
 * to the host (or, in split-merge, is re-run with a wider window).  Values outside [0, 1] are an
 * argument error.  Same chain either way. */
#define HDPM_OPT_PHI_SD_SCALE 11
int hdpm_set_option(hdpm_ctx* ctx, int32_t option, double value);
/* The current value of an option (the same units as hdpm_set_option; HDPM_OPT_PHI_DEVICE
 * reads 1 when update_phi runs on the device, which may be the default). */
int hdpm_get_option(hdpm_ctx* ctx, int32_t option, double* value);
/* Posterior analysis (realdata_analysis/zoo_simulator.R:193-236, 339-344; mcclust /
 * mcclust.ext).  hdpm_psm_build: the posterior similarity matrix of M saved label vectors
 * c_trace[M x N] (results$c_i, labels 0..254) -- comp.psm(C) -- kept on the device as
 * co-clustering counts (psm = count / M).  hdpm_psm_rows: rows row0 .. row0+nrows-1 of psm
 * (N doubles each).  hdpm_psm_vi_lb: VI.lb(cls, psm) of ncand candidate partitions
 * cls[ncand x N] (the lower bound of the posterior expected variation of information that
 * minVI minimises). */
int hdpm_psm_build(hdpm_ctx* ctx, const int32_t* c_trace, int32_t M, int32_t N);
int hdpm_psm_rows(hdpm_ctx* ctx, int32_t row0, int32_t nrows, double* out);
int hdpm_psm_vi_lb(hdpm_ctx* ctx, const int32_t* cls, int32_t ncand, double* out);
/* The same analysis from the saved labels alone, with no N x N matrix (O(M N) work and bytes
 * per candidate; any N that the labels themselves fit).  With T^m[a][b] = #{j: c_j = a,
 * z_m(j) = b} the contingency table of a candidate c against draw z_m and n^m_b the draw's
 * cluster sizes, the device keeps one byte per saved label and computes T^m per block of
 * candidates.  The trace buffers are separate from the psm ones: a context may hold both.
 *
 * hdpm_trace_build: M saved label vectors c_trace[M x N], labels 0..254 (HDPM_E_ARG
 *   otherwise).  table_budget_bytes bounds the table array of one block of candidates
 *   (M x Ka x Kz x 4 bytes each, Ka / Kz the largest cluster counts of the candidates / the
 *   draws; at least one candidate per block); 0 means the default, 256 MiB.  No result
 *   depends on it.
 * hdpm_trace_terms: all[i] = sum_m n^m[z_m(i)] = M sum_j psm_ij (N values) and same[c][i] =
 *   sum_m T^m[c_i][z_m(i)] = M sum_{j: c_j = c_i} psm_ij (ncand x N) of candidates
 *   cls[ncand x N], exact integers.  Either output may be NULL (all alone runs no table pass).
 * hdpm_trace_losses: per candidate VI.lb(c, psm) (the value of hdpm_psm_vi_lb, from the
 *   integer sums), the posterior expected VI (mcclust.ext VI(cls, cls.draw)) =
 *   (sum_a n_a log2 n_a + (1/M) sum_m (sum_b n^m_b log2 n^m_b - 2 sum_ab T^m log2 T^m)) / N,
 *   and the integers of Binder's loss sum_{i<j} |1(c_i = c_j) - psm_ij| = A + (P - 2 Q) / M:
 *   binder_Q[c] = sum_m sum_ab C2(T^m[a][b]) and *binder_P = sum_m sum_b C2(n^m_b) (one
 *   value), C2(x) = x (x - 1) / 2; A = sum_a C2(n_a) is the caller's.  Any output may be NULL.
 * hdpm_trace_tables (testing and inspection): T^m of every candidate for draws m0 ..
 *   m0 + nm - 1, out[ncand x nm x 256 x 256].
 * Candidate labels are 0..254.  HDPM_E_ARG with a message for labels out of range, for a call
 * before hdpm_trace_build and for m0 + nm > M. */
int hdpm_trace_build(hdpm_ctx* ctx, const int32_t* c_trace, int32_t M, int32_t N, int64_t table_budget_bytes);
int hdpm_trace_terms(hdpm_ctx* ctx, const int32_t* cls, int32_t ncand, uint64_t* all, uint64_t* same);
int hdpm_trace_losses(hdpm_ctx* ctx, const int32_t* cls, int32_t ncand, double* vi_lb, double* vi,
                      uint64_t* binder_Q, uint64_t* binder_P);
int hdpm_trace_tables(hdpm_ctx* ctx, const int32_t* cls, int32_t ncand, int32_t m0, int32_t nm, uint32_t* out);
/* How far an estimate can be trusted (mcclust.ext credibleball and the block structure of the
 * PSM ordered by the estimate's classes), after hdpm_trace_build and with its refusals.
 *
 * hdpm_trace_distances: the distance of every candidate cls[ncand x N] to every saved draw.
 *   vi[c * M + m] = (sum_a n_a log2 n_a + sum_b n^m_b log2 n^m_b - 2 sum_ab T^m log2 T^m) / N,
 *   the variation of information, evaluated as (hc + S_m - 2 l) / N in that order with hc as
 *   in hdpm_trace_losses, so draws with equal labels give bit-equal values; a result that
 *   rounding took below 0 is returned as 0.0.  binder[c * M + m] = A_c + P_m - 2 Q_cm, the
 *   number of pairs i < j on which the two partitions disagree (A_c = sum_a C2(n_a), P_m =
 *   sum_b C2(n^m_b), Q_cm = sum_ab C2(T^m[a][b])): the exact pair count, not mcclust's
 *   scaling of Binder's loss, which is unpinned here.  draw_k[m] = the clusters of draw m.
 *   Any output may be NULL; draw_k alone runs no table pass.
 * hdpm_trace_affinity: one partition cl[N] with labels 0..Ka-1, 1 <= Ka <= 255 (Ka may exceed
 *   the largest label + 1: empty clusters give zero columns and rows; a label >= Ka is
 *   HDPM_E_ARG).  aff[i * Ka + a] = sum_m T^m[a][z_m(i)] = M sum_{j: c_j = a} psm_ij (N x Ka)
 *   and cross[a * Ka + b] = sum_m sum_z T^m[a][z] T^m[b][z] = M sum_{i in a, j in b} psm_ij
 *   (Ka x Ka, symmetric), exact integers.  Either output may be NULL.  cross needs
 *   N^2 M < 2^63 (HDPM_E_ARG otherwise).  aff is produced in blocks of points whose device
 *   staging stays within table_budget_bytes (at least 16 points per block), each copied to
 *   the caller as it completes; no result depends on the budget. */
int hdpm_trace_distances(hdpm_ctx* ctx, const int32_t* cls, int32_t ncand, double* vi, uint64_t* binder,
                         int32_t* draw_k);
int hdpm_trace_affinity(hdpm_ctx* ctx, const int32_t* cl, int32_t Ka, uint64_t* aff, uint64_t* cross);
/* A point estimate refined by single-point moves (the local search of mcclust.ext's greedy and
 * of SALSO, without their splits and restarts; their merges are hdpm_trace_refine_merge's,
 * below: hdpm_trace_refine itself makes none), after hdpm_trace_build and with
 * hdpm_trace_affinity's refusals; an unknown loss or a negative max_rounds is HDPM_E_ARG too.
 * With n_a the class sizes of cl, T^m its table against draw z_m and
 *   h(t) = (t + 1) log2(t + 1) - t log2 t, h(0) = 0, evaluated as
 *          log2(t + 1) + t log1p(1 / t) / ln 2,
 * moving point i alone from a = cl[i] to class b != a changes the loss by
 *   HDPM_LOSS_VI:     gain[i][b] = (M (h(n_b) - h(n_a - 1))
 *                                   - 2 sum_m (h(T^m[b][z_m(i)]) - h(T^m[a][z_m(i)] - 1))) / (M N),
 *                     the change of hdpm_trace_losses' vi;
 *   HDPM_LOSS_BINDER: gain[i][b] = M (n_b - n_a - 1) - 2 (aff[i][b] - aff[i][a]), the change of
 *                     the integer M A + P - 2 Q (M times Binder's loss), exact: accumulated in
 *                     64-bit integers and returned as a double that holds it (|gain| <= 3 M N),
 * and gain[i][a] = 0.  Column b = Ka is a new class of its own (n_b = 0, T[b][.] = 0).  VI's sum
 * over the draws is taken in draw order, per (point, class); no result depends on how the points
 * are cut into blocks.
 *
 * hdpm_trace_move_gains: full[i * (Ka + 1) + b] = gain[i][b] (N x (Ka + 1); testing and
 *   inspection), best[i] the class with the smallest gain and gain[i] that gain (N each, the
 *   only bytes that leave the device without full).  The own class wins a tie, then the lowest
 *   class.  The new class is offered only while Ka < 255: at Ka = 255 its column holds +inf and
 *   is never best.  Any output may be NULL.  The gains are staged on the device in blocks of
 *   points within table_budget_bytes (whole groups of 16 points, at least 16).
 * hdpm_trace_refine: descends from cl (labels 0..254) by rounds of such moves.  One round on the
 *   current partition c with loss L: the candidates are the points with gain < 0; of those whose
 *   best is the new class only the one with the smallest gain stays (the lowest index breaking a
 *   tie): at most one new class per round.  No candidate: stop, converged = 1 (c is a minimum
 *   under single-point moves).  The candidates are ordered by (gain, index) ascending, k their
 *   number.  Trial: the first k moves applied at once, the result relabelled 0..K-1 by first
 *   appearance, its loss evaluated exactly as hdpm_trace_losses does (VI's double, Binder's
 *   integer) and accepted iff strictly below L; a rejected trial with k = 1 stops the run with
 *   converged = 1 (VI only, by rounding), any other is followed by k = ceil(k / 2).  After an
 *   accepted trial the next round starts from the full candidate set; after max_rounds accepted
 *   rounds the run stops with converged = 0 unless no candidate is left.  Simultaneous moves are
 *   no descent by themselves; the strict test makes every accepted round one.
 *   cl_out[N] is the end state (labels 0..K-1 by first appearance: the start relabelled if no
 *   round was accepted); info->rounds the accepted rounds, trials the evaluated trials, moved
 *   the moves of the accepted trials, K the end state's classes, start / value the loss before
 *   and after; history[max_rounds + 1] (may be NULL) the loss at the start and after each
 *   accepted round.  VI values are hdpm_trace_losses' vi; Binder values are the integer
 *   M A + P - 2 Q as a double, and Binder needs N^2 M < 2^63 (HDPM_E_ARG otherwise). */
#define HDPM_LOSS_VI 0
#define HDPM_LOSS_BINDER 1
typedef struct hdpm_refine_info {
  int32_t rounds, trials, converged, K;
  int64_t moved;
  double start, value;
} hdpm_refine_info;
int hdpm_trace_move_gains(hdpm_ctx* ctx, const int32_t* cl, int32_t Ka, int32_t loss, int32_t* best, double* gain,
                          double* full);
int hdpm_trace_refine(hdpm_ctx* ctx, const int32_t* cl, int32_t loss, int32_t max_rounds, int32_t* cl_out,
                      hdpm_refine_info* info, double* history);
/* Merges of two classes as moves: a descent by single-point moves stalls where the draws leave
 * open whether two classes are one (every point is more similar to its own half), and merging
 * the classes lowers the loss.  The gains of all pairs are functions of the tables T^m and the
 * class sizes alone: one table pass, whatever the number of pairs.  After hdpm_trace_build and
 * with hdpm_trace_affinity's refusals (a label >= Ka, Ka outside 1..255); an unknown loss is
 * HDPM_E_ARG, and HDPM_LOSS_BINDER needs N^2 M < 2^63.  With
 *   f(s, t) = (s + t) log2(s + t) - s log2 s - t log2 t for s, t >= 1 and 0 if s = 0 or t = 0,
 *             evaluated as (s log1p(t / s) + t log1p(s / t)) / ln 2,
 * merging the non-empty classes a < b of cl changes the loss by
 *   HDPM_LOSS_VI:     mgain[a][b] = (M f(n_a, n_b) - 2 sum_m sum_z f(T^m[a][z], T^m[b][z])) / (M N),
 *                     the change of hdpm_trace_losses' vi.  The sum runs over 64 slices of the
 *                     draws (m = y, y + 64, ..; M slices if M < 64), within a slice in draw order
 *                     and z ascending, and the slices are added in order: no value depends on
 *                     table_budget_bytes or on Ka;
 *   HDPM_LOSS_BINDER: mgain[a][b] = M n_a n_b - 2 cross[a][b] (hdpm_trace_affinity's cross), the
 *                     exact change of the integer M A + P - 2 Q, formed in 64 bits and returned as
 *                     a double that holds it (|gain| <= 3 M N^2).
 * The matrix is symmetric with a zero diagonal, and a pair with an empty class has gain exactly 0.
 *
 * hdpm_trace_merge_gains: gain[a * Ka + b] = mgain[a][b] (Ka x Ka); best[2] the pair a < b of
 *   non-empty classes with the smallest gain, the lowest a winning a tie and then the lowest b,
 *   and *best_gain its gain; with fewer than two non-empty classes best = {-1, -1} and
 *   *best_gain = 0.  An empty class is never a candidate.  Any output may be NULL.
 * hdpm_trace_merge_path: greedy agglomeration from cl (labels 0..Ka-1 as they stand) down to
 *   k_min classes (k_min >= 1, HDPM_E_ARG otherwise).  *steps = max(0, K0 - k_min) with K0 the
 *   non-empty classes of cl.  Each step merges the best pair (the rule above) of the current
 *   state, whether or not its gain is negative; the merged class keeps the lower label a, and
 *   merge[2 s], merge[2 s + 1] = a, b name the caller's labels.  step_gain[s] is that pair's
 *   gain.  value[0] is the loss of cl and value[s + 1] the loss after step s, evaluated from the
 *   merged tables (row b of every T^m added into row a) and never as the running sum of the
 *   gains: VI as hdpm_trace_losses' vi, Binder's integer M A + P - 2 Q exactly, as a double.
 *   One pass over the points runs at the start; every step works on the tables alone.  merge
 *   holds up to (Ka - 1) x 2 entries, step_gain Ka - 1, value Ka.  Any output may be NULL.
 * hdpm_trace_refine_merge: alternates two phases from cl (labels 0..254).  The descent of
 *   hdpm_trace_refine, with the rounds left of max_rounds, ends at c with loss L; if it ran out
 *   of rounds with candidates left the run stops with converged = 0.  Otherwise the pair gains
 *   of c are taken: no pair with gain < 0 stops the run with converged = 1 (c is a minimum
 *   under single-point moves and pair merges); after max_merges accepted merges a negative pair
 *   stops it with converged = 0.  Else the best pair is tried: the merged partition relabelled
 *   by first appearance, its loss evaluated as every trial of hdpm_trace_refine is, accepted
 *   iff strictly below L.  A rejected merge stops the run with converged = 1 (VI only, by
 *   rounding); an accepted one is followed by the descent again.  Every accepted step lowers the
 *   evaluated loss strictly, so the run ends.  info covers the whole run (trials counts the
 *   evaluated trials of both phases), *merges the accepted merges, and history[max_rounds +
 *   max_merges + 1] (may be NULL) holds the loss at the start and after each accepted round or
 *   merge, info->rounds + *merges + 1 values.  A negative max_rounds or max_merges is HDPM_E_ARG. */
int hdpm_trace_merge_gains(hdpm_ctx* ctx, const int32_t* cl, int32_t Ka, int32_t loss, double* gain, int32_t* best,
                           double* best_gain);
int hdpm_trace_merge_path(hdpm_ctx* ctx, const int32_t* cl, int32_t Ka, int32_t loss, int32_t k_min, int32_t* merge,
                          double* step_gain, double* value, int32_t* steps);
int hdpm_trace_refine_merge(hdpm_ctx* ctx, const int32_t* cl, int32_t loss, int32_t max_rounds, int32_t max_merges,
                            int32_t* cl_out, hdpm_refine_info* info, int32_t* merges, double* history);
/* mcclust.ext minVI(method = "avg") / mcclust minbinder(method = "avgl") =
 * hclust(as.dist(1 - psm), "average") + cutree, from the saved labels alone.  Points whose
 * labels agree in every draw have psm = 1 (distance 0) and any other pair has distance
 * >= 1/M, so average linkage merges each such group completely first; the rest of the tree
 * is average linkage on the U distinct label columns, each weighted by its member count.
 * The calls below are made in this order after hdpm_trace_build (which discards the groups
 * and the tree of an earlier trace); out of order they return HDPM_E_ARG with a message.
 *
 * hdpm_trace_groups: replaces the zero-height part of hclust.  Groups the N points by their
 *   M-label column, exactly (a hash places a column, a byte-for-byte comparison admits it),
 *   and numbers the groups by ascending smallest member; *U = their count.  max_groups: 0
 *   means HDPM_TRACE_GROUPS_DEFAULT, at most HDPM_TRACE_GROUPS_MAX (the host holds U x U
 *   uint64 for the tree); more distinct columns than that stop the device pass and return
 *   HDPM_E_ARG ("too unsettled").  hash_bits: 0 = the full 32-bit hash, 1..32 keep that many
 *   bits (testing: forces collisions); no result depends on it.  HDPM_E_ARG if N^2 M does
 *   not fit 63 bits (the tree's integer sums).
 * hdpm_trace_group_info: first[U] (smallest member), weight[U] (member count), group_of[N],
 *   counts[U x U] = S[u][v] = #{m: the groups' labels agree in draw m} (S[u][u] = M; the sum
 *   of psm over the two groups' points is w_u w_v S_uv / M).  Any output may be NULL.
 * hdpm_trace_avg_tree: replaces hclust(.., "average") above height 0.  With Q_AB =
 *   sum_{u in A, v in B} w_u w_v S_uv (uint64) the merge order is the greedy one, decided in
 *   exact integer arithmetic: among the active pairs with the largest Q_AB / (w_A w_B), the
 *   pair whose smaller `first` is smallest, then whose larger `first` is smallest; the merged
 *   cluster keeps the smaller `first`.  R's hclust tie order is unpinned here (R is absent),
 *   as minVI's other conventions are.  merge[(U - 1) x 2]: the two clusters of each step,
 *   each named by its member group with the smallest `first` (= its smallest group number),
 *   column 0 the name the merged cluster keeps.  height[U - 1] = 1 - Q_AB / (M w_A w_B) as
 *   doubles, for inspection only.  Either output may be NULL.
 * hdpm_trace_cut_losses: replaces cutree + VI.lb / VI / binder of each cut.  The cut into k
 *   clusters is the state after U - k merges; for k = k0 .. k0 + nk - 1 (1 <= k <=
 *   min(U, 255): the trace tables hold at most 255 clusters) vi_lb[nk], vi[nk] and the
 *   integers of Binder's loss A + (P - 2 Q) / M, binder_A[nk] and binder_Q[nk] (P from
 *   hdpm_trace_losses), all from tables over the U weighted groups; every integer equals
 *   what hdpm_trace_terms / hdpm_trace_losses give for the cut expanded to N labels.  Cuts
 *   into more than U clusters split groups and never lower VI.lb.  Blocks of cuts obey
 *   table_budget_bytes.  Any output may be NULL.
 * hdpm_trace_cut_labels: cutree(k) per point, cl[N], labels 0..k-1 in order of first
 *   appearance, 1 <= k <= U. */
#define HDPM_TRACE_GROUPS_DEFAULT 8192
#define HDPM_TRACE_GROUPS_MAX 16384
int hdpm_trace_groups(hdpm_ctx* ctx, int32_t max_groups, int32_t hash_bits, int32_t* U);
int hdpm_trace_group_info(hdpm_ctx* ctx, int32_t* first, int32_t* weight, int32_t* group_of, uint32_t* counts);
int hdpm_trace_avg_tree(hdpm_ctx* ctx, int32_t* merge, double* height);
int hdpm_trace_cut_losses(hdpm_ctx* ctx, int32_t k0, int32_t nk, double* vi_lb, double* vi, uint64_t* binder_A,
                          uint64_t* binder_Q);
int hdpm_trace_cut_labels(hdpm_ctx* ctx, int32_t k, int32_t* cl);
/* The posterior predictive from the recorded draws: where a row the chain never saw belongs,
 * and the pointwise log-likelihood of the training rows for WAIC and LPML.  Saved draw s
 * (0 <= s < M) has K_s clusters of sizes n_k (from the saved labels), centers c_kj and sigmas
 * sg_kj; gamma and attrisize m_j are the chain's; a row y holds codes 1..m_j.  With
 *   ll_k(y) = sum_j dhamming(y_j, c_kj, sg_kj, m_j), added in attribute order (the bits of
 *             hdpm_loglik_matrix on that state),
 *   ll_0 = -sum_j log(m_j), the log prior predictive of any row (a uniform prior center, and
 *          dhamming sums to 1 over the codes for every sigma),
 *   w_k = log n_k + ll_k(y), w_0 = log gamma + ll_0 (the urn given draw s), lse = log sum_{k >= 0}
 *   exp(w_k) and r_k = exp(w_k - lse):
 * the calls below come after hdpm_trace_build of the same saved iterations, whose labels of
 * draw s must be exactly 0..K_s-1 (label k names parameter row k); a later hdpm_trace_build
 * discards the parameters.  Every exp and log is glibc's on host and device; every sum of
 * exps subtracts its maximum.  A row's sums over draws run in draw order and its sums over
 * clusters in cluster order: no result depends on table_budget_bytes, bit for bit.
 *
 * hdpm_predict_build: the parameters of the M draws, total_cls[M] and sum_s K_s rows of d
 *   centers and sigmas in saved-iteration order (what hdpm_record_take returns), kept on the
 *   device as a byte, dhamming's (match, mismatch) pair and the raw sigma per (s, k, j).
 * hdpm_predict_new: ny rows codes[ny x d].  lpd[y] = log((1/M) sum_s exp(lse^s)) - log(N + gamma),
 *   the log posterior predictive density; p_new[y] = (1/M) sum_s r^s_0, the probability of a
 *   cluster of its own; with a partition cl[N] of the training points into classes 0..Ka-1
 *   (1 <= Ka <= 255) and T^s its contingency table against draw s, coclass[y * Ka + a] =
 *   (1 / (M n_a)) sum_s sum_{k >= 1} r^s_k T^s[a][k], the mean over the points i of class a of the
 *   probability that y is clustered with i (0 for an empty class).  Any output may be NULL
 *   and a call computes only what its outputs need: without coclass no table pass runs and cl
 *   is not read.  Rows go through in blocks whose device staging obeys table_budget_bytes
 *   (at least 64 rows per block).
 * hdpm_predict_own: the training rows codes[N x d] themselves; with l_s the ll of row i under
 *   its own cluster z_s(i) in draw s, lppd[i] = log((1/M) sum_s exp(l_s)), logcpo[i] =
 *   -log((1/M) sum_s exp(-l_s)) and var[i] the sample variance of l_s over the draws (ddof 1;
 *   0.0 when M = 1).  WAIC = -2 sum_i (lppd[i] - var[i]) and LPML = sum_i logcpo[i] are the
 *   caller's sums.  Any output may be NULL.
 * hdpm_predict_loglik (testing and inspection): one draw s; ll[ny x K_s] and resp[ny x
 *   (K_s + 1)], slot 0 the new cluster.  Either output may be NULL.
 * HDPM_E_ARG with a message (naming the draw, cluster, row or attribute) for: a call before
 * hdpm_trace_build or hdpm_predict_build; total_cls[s] different from the trace's cluster count
 * of draw s; d or an attrisize outside what hdpm_set_data accepts; a center that is not an
 * integer in 1..m_j; a sigma that is not finite and > 0; gamma <= 0; a code outside 1..m_j;
 * a cl label >= Ka, or Ka outside 1..255; s outside 0..M-1. */
int hdpm_predict_build(hdpm_ctx* ctx, int32_t d, const int32_t* attrisize, double gamma, const int32_t* total_cls,
                       const double* centers, const double* sigmas);
int hdpm_predict_new(hdpm_ctx* ctx, const uint8_t* codes, int32_t ny, const int32_t* cl, int32_t Ka, double* lpd,
                     double* p_new, double* coclass);
int hdpm_predict_own(hdpm_ctx* ctx, const uint8_t* codes, double* lppd, double* var, double* logcpo);
int hdpm_predict_loglik(hdpm_ctx* ctx, int32_t s, const uint8_t* codes, int32_t ny, double* ll, double* resp);
/* Rows with missing attributes: code 0 in a row says "not observed".  Attributes are
 * independent given the cluster and dhamming sums to 1 over an attribute's codes for every
 * sigma, so the marginal of a row over its missing attributes is the same urn with those
 * attributes left out of every sum.  With O(y) the observed attributes of row y:
 *   ll_k(y) = sum_{j in O} dhamming(y_j, c_kj, sg_kj, m_j), in attribute order (a missing
 *             attribute adds nothing, which is adding +0.0),
 *   ll_0(y) = -sum_{j in O} log(m_j), left to right in attribute order, per row,
 *   w_k = log n_k + ll_k(y), w_0 = log gamma + ll_0(y); lse and r_k as above.
 *
 * hdpm_predict_partial: hdpm_predict_new's outputs and rules with these ll_k / ll_0.  A row
 *   without a 0 gets the bytes hdpm_predict_new gives it; a row of all 0 has w_k = log n_k and
 *   w_0 = log gamma (lpd = 0).  hdpm_predict_new itself keeps refusing 0.
 * hdpm_predict_impute: the law of each missing code given the observed codes of its row.
 *   Entries are the 0 codes of codes[ny x d] in row-major order, n_missing of them; entry e is
 *   (row y, attribute j).  For level l = 1..m_j, per draw s:
 *     q_l = r_0 / (double)m_j;  then for k = 1..K_s in cluster order
 *     q_l = q_l + r_k * (l == c_kj ? exp(match_kj) : exp(mismatch_kj)),
 *   the exps glibc's.  Over the draws, in draw order, under the running maximum mx of lse that
 *   lpd's sum keeps (acc = sum_s exp(lse^s - mx)): A_l = q_l at the first draw; at a new
 *   maximum A_l = A_l * exp(mx_old - lse) + q_l; otherwise A_l = A_l + q_l * exp(lse - mx).
 *   pmf[e * ld + l - 1] = A_l / acc = sum_s p(y_O, y_j = l | s) / sum_s p(y_O | s) =
 *   p(y_j = l | y_O, data); slots m_j .. ld-1 are 0.0.  The pmfs of several gaps of one row are
 *   marginals, not their joint law.  lpd[ny] (may be NULL) has hdpm_predict_partial's bytes.
 *   n_missing = 0 is accepted and writes only lpd.
 * No result depends on table_budget_bytes, bit for bit.  HDPM_E_ARG with a message for: a
 * call before hdpm_predict_build; a code above m_j (row and attribute named); n_missing
 * different from the count of 0 codes; ld above 255, or below the m_j of a missing attribute
 * (named); and hdpm_predict_new's refusals for cl and Ka. */
int hdpm_predict_partial(hdpm_ctx* ctx, const uint8_t* codes, int32_t ny, const int32_t* cl, int32_t Ka, double* lpd,
                         double* p_new, double* coclass);
int hdpm_predict_impute(hdpm_ctx* ctx, const uint8_t* codes, int32_t ny, int64_t n_missing, int32_t ld, double* pmf,
                        double* lpd);
/* What each class of a point estimate is: the center code of every attribute with its posterior
 * probability, and the sigma of every attribute with its spread.  After hdpm_trace_build and
 * hdpm_predict_build; cl[N] holds labels 0..Ka-1, 1 <= Ka <= 255, a class may be empty
 * (hdpm_predict_new's rules for cl).  For a point i of class a, draw s says "your center is
 * c^s_{z_s(i)}, your sigma is sg^s_{z_s(i)}"; averaged over the members of a and over the draws
 * this does not depend on how a draw numbers its clusters, so no labels are matched between
 * draws, and the member sums are sums over the contingency table T^s[a][k] of cl against draw s.
 * With n_a the class sizes, c_kj / sg_kj draw s's parameters and em_kj = exp(match_kj), ei_kj =
 * exp(mismatch_kj) (hdpm_predict_impute's values):
 *   center_cnt[(a * d + j) * ld + l - 1] = sum_s sum_k T^s[a][k] [c^s_kj == l], an exact integer;
 *     divided by M n_a it is the posterior probability that the center of a member of a has code
 *     l at attribute j.  Slots m_j .. ld-1 are 0.
 *   sigma_trace[(s * Ka + a) * d + j] = u_s = (sum_k (double)T^s[a][k] * sg^s_kj) / (double)n_a,
 *     k in cluster order, plain multiply and add: the relabelled parameter trace (M x Ka x d).
 *   sigma_mean, sigma_var (Ka x d): Welford's recurrence over u_s in draw order from mean = 0,
 *     m2 = 0: delta = u - mean; mean = mean + delta / (s + 1); m2 = m2 + delta * (u - mean);
 *     sigma_mean is the final mean and sigma_var = m2 / (M - 1), 0.0 when M = 1 (the variance,
 *     not the sd: no device sqrt).
 *   code_pmf[(a * d + j) * ld + l - 1] = (1 / (M n_a)) sum_s sum_k T^s[a][k] (l == c^s_kj ?
 *     em_kj : ei_kj), the model's predictive law of the code of a member of a at attribute j, to
 *     hold against the class's observed code frequencies; slots m_j .. ld-1 are 0.0.  The sums
 *     run over s in draw order, then k in cluster order; the device keeps base = sum T ei and
 *     per level sum_{c = l} T (em - ei) and returns (base + that) / (M n_a), so the value is
 *     within rounding of the definition (M K terms in (0, 1]), not its bits.
 * An empty class gets 0 / 0.0 in every output.  Any output may be NULL and a call computes only
 * what its outputs need.  The level rows are staged in blocks of attributes and sigma_trace in
 * chunks of draws that obey table_budget_bytes (at least one attribute, one draw), each copied
 * out as it completes; no result depends on the budget, bit for bit.  HDPM_E_ARG with a message
 * for: a call before either build; a label >= Ka, or Ka outside 1..255; ld outside 1..255 or
 * below the largest m_j (the attribute is named). */
int hdpm_predict_profile(hdpm_ctx* ctx, const int32_t* cl, int32_t Ka, int32_t ld, uint64_t* center_cnt,
                         double* code_pmf, double* sigma_mean, double* sigma_var, double* sigma_trace);
/* Testing: one draw on the device from log-weights logw[E] (E <= 256) and the uniform rU --
 * the n8:95-102 categorical draw (two_way = 0; *pick = the 0-based index, or -status) or the
 * sm:204-215 two-way draw (two_way = 1, E = 2) -- with the engine's exp, glibc's algorithm
 * (ocml = 0), or the device libm's (ocml = 1: what the engine used before; shows the ulp
 * differences the glibc replica removes). */
int hdpm_debug_draw(hdpm_ctx* ctx, const double* logw, int32_t E, double rU, int32_t two_way, int32_t ocml,
                    int32_t* pick);
/* Testing: exp (fn = 0) or log (fn = 1) of x[n] on the device, glibc's algorithm (ocml = 0)
 * or the device libm's (ocml = 1). */
int hdpm_debug_math(hdpm_ctx* ctx, const double* x, int64_t n, int32_t fn, int32_t ocml, double* out);
/* Testing: what the last launches of this process actually used, from the host's own
 * bookkeeping (no kernel, nothing queued or waited for, a prepared sweep stays prepared).  The
 * HDPM_* environment switches (csrc/switches.hpp) override launch geometry and select paths,
 * and one outside its range, or a group size that does not fit, falls back silently: a test of
 * a switch reads here that its path ran.  -1: no such launch yet.
 *   phi_*: the fast device update_phi (launch_phi2): its group size, groups per cluster, the
 *     threads of k_phi2_group and k_phi2_tree, the waves of k_phi2_values; phi_gs_refused: 1 when
 *     the last plan under HDPM_PHI2_GS found that size not to fit (no fast path then), 0 when
 *     it took it.
 *   wide_*: k_prepass_wide's grid, chunks (16 points each) and claim flag; wide_launches counts
 *     its launches.
 *   mt_*: the stream generator's last window: the workgroups and blocks per workgroup of the
 *     jump tables it holds (0: none built), whether the window ran on them (mt_multi) and its
 *     draws (mt_window, saturating); mt_multi_windows counts the windows that did.
 *   dense_direct, lbound, spec_lv: the last sweep launch's prepass arguments of these names.
 *   mass_static: k_exact_rows_mass's fixed-order flag at its last launch.
 *   dense_direct_launches, lbound_launches: the sweep launches so far with that argument set;
 *     unsettled_margin_launches: those that listed by margins alone behind an unsettled launch
 *     (what HDPM_FP_UNSETTLED_UNIF=0 asks for). */
typedef struct hdpm_launches {
  int32_t phi_gs, phi_G, phi_group_threads, phi_tree_threads, phi_values_waves, phi_gs_refused;
  int32_t wide_grid, wide_chunks, wide_claim, wide_launches;
  int32_t mt_G, mt_bpg, mt_multi, mt_window, mt_multi_windows;
  int32_t dense_direct, lbound, spec_lv, mass_static;
  int32_t dense_direct_launches, lbound_launches, unsettled_margin_launches;
} hdpm_launches;
int hdpm_debug_launches(hdpm_ctx* ctx, hdpm_launches* out);
/* Block until every kernel and copy the context has queued is done, a prepared next
 * sweep's prefix (scratch outputs only) included; the prepared sweep stays prepared. */
int hdpm_synchronize(hdpm_ctx* ctx);
/* Drop a prepared next sweep (the one the last hdpm_iterations / hdpm_iteration call set up:
 * its prepass possibly queued on the device, its speculative update_phi on the host pool):
 * the job is joined and the stream rewound, so the next iteration does all of its own work
 * (bench.py calls it between the warmup and the timed window).  Any other state-changing
 * call does the same implicitly. */
int hdpm_drop_prepared(hdpm_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* HDPM_H */
