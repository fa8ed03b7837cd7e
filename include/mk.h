/* libmk -- MI355X-native meta-kriging hot path (C ABI, no torch / R types).
 *
 * Drop-in boundary for the data-parallel core of MetaKriging_BinaryResponse.R:
 * the per-subset spMvGLM fits + spPredict kriging + 200-level quantile
 * summaries (the `foreach(i=1:n.core) %dopar% partitioned_spMvGLM(...)` at
 * MK.R:108, whose body is MK.R:46-96) and the quantile-average combine
 * (MK.R:119-133).  Conventions are R's: column-major fp64 matrices, int32
 * counts, location-major multivariate vectors (site i, outcome a at i*q + a),
 * caller-allocated outputs.  Every call returns 0 on success or a negative
 * MK_E* code; mk_last_error() gives the thread-local message.
 * See INTEGRATION.md for the R .Call glue that binds these entry points.
 */
#ifndef MK_H
#define MK_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MK_OK 0
#define MK_E_ARG (-1)      /* invalid argument (R: stop()) */
#define MK_E_HIP (-2)      /* HIP runtime failure */
#define MK_E_NOMEM (-3)    /* device allocation failed */
#define MK_E_NODEV (-4)    /* no HIP device */
#define MK_E_INTERRUPT (-5) /* the progress callback asked to stop (R: a user interrupt) */

#define MK_COV_EXPONENTIAL 0
#define MK_COV_MATERN 1
#define MK_LINK_LOGIT 0    /* spMvGLM's binomial family (MK.R:80-84), logistic p(y=1) (MK.R:160) */
#define MK_LINK_PROBIT 1   /* north-star extension: Phi link (no reference parity target)        */
#define MK_N_LEVELS 200    /* quantile(x, probs = seq(0.005, 1, 0.005)), MK.R:88 */

/* Subset data.  Replaces the globals Y*.part / X*.part / coords.part the
 * worker reads (MK.R:67-75) plus coords.test (MK.R:87, 108). */
typedef struct mk_problem {
  int32_t n_subsets;          /* subsets in this call (this GPU's shard)              */
  int32_t subset_base;        /* global index of subset 0 (selects its RNG stream)    */
  int32_t q;                  /* outcomes (MK.R:80: length of the formula list)       */
  int32_t p;                  /* regression coefficients, sum over outcomes           */
  const int32_t* n_part;      /* [n_subsets] sites per subset (MK.R:18)               */
  const double* coords;       /* concatenated per subset: n_s x 2 column-major        */
  const double* y;            /* concatenated per subset: n_s*q responses (counts)    */
  const double* weights;      /* concatenated per subset: n_s*q binomial trials       */
  const double* x;            /* concatenated per subset: (n_s*q) x p column-major    */
  int32_t n_test;             /* held-out sites (coords.test rows)                    */
  const double* coords_test;  /* n_test x 2 column-major                              */
  const double* x_test;       /* (q*n_test) x p column-major, location-major rows: x.test
                                 (MK.R:87 spPredict's pred.covars), or NULL -- without it no
                                 predictive probability (p_predict ...) can be asked for   */
} mk_problem;

/* spMvGLM arguments (MK.R:56-64, 80-85).  Tuning values are proposal
 * VARIANCES (spBayes amcmc semantics); beta_tuning is length p (the diagonal
 * of the t(chol(vcov)) matrix MK.R:55 builds). */
typedef struct mk_config {
  int32_t cov_model;          /* MK_COV_EXPONENTIAL (MK.R:84) or MK_COV_MATERN        */
  int32_t n_batch;            /* MK.R:57 */
  int32_t batch_length;       /* MK.R:58 */
  double accept_rate;         /* MK.R:83 */
  int32_t burn_in;            /* first kept sample, 1-based (MK.R:85-89: start = burn.in) */
  const double* beta_starting;  /* [p]  MK.R:54 */
  const double* beta_tuning;    /* [p]  MK.R:55 (diagonal) */
  const double* phi_starting;   /* [q]  MK.R:60 */
  const double* phi_tuning;     /* [q]  MK.R:61 */
  const double* A_starting;     /* [q(q+1)/2] lower triangle of A, col-major (MK.R:56) */
  const double* A_tuning;       /* [q(q+1)/2] MK.R:61 */
  const double* nu_starting;    /* [q] Matern only, else NULL */
  const double* nu_tuning;      /* [q] Matern only, else NULL */
  double w_starting;            /* MK.R:60 */
  double w_tuning;              /* MK.R:62 */
  const double* phi_unif_a;     /* [q] MK.R:63 */
  const double* phi_unif_b;     /* [q] */
  const double* nu_unif_a;      /* [q] Matern only */
  const double* nu_unif_b;      /* [q] Matern only */
  double K_IW_df;               /* MK.R:64 */
  const double* K_IW_S;         /* [q*q] col-major, MK.R:64 */
  uint64_t seed;                /* Philox stream seed (the R glue draws it from R's RNG) */
  int32_t record_samples;       /* keep p.beta.theta.samples (n_samples x P)            */
  int32_t record_w;             /* keep p.w.samples ((n_s*q) x n_samples)               */
  int32_t device;               /* HIP device ordinal                                    */
  int32_t n_streams;            /* subset groups run on this many HIP streams (0: default 1);
                                   results do not depend on it                          */
  int32_t predict_tile;         /* 0 (or >= n_test): spPredict fused into the kept iterations.
                                   Else the kept chain states are recorded and the kriging
                                   runs after the fit over tiles of this many test sites, so
                                   (q*n_test) x kept draws per subset never coexist (cfg5:
                                   1M sites).  The exact replay gives the fused draws bit for
                                   bit.  Exponential sessions (any q) whose kept window is long
                                   enough for it to save exact evaluations interpolate the
                                   kriging variance in phi per (subset, outcome) pair
                                   (MK_KRIG_CHEB): the draws then agree with the
                                   fused ones to 1e-8 absolute, not bit for bit               */
  int32_t link;                 /* MK_LINK_LOGIT (the reference) or MK_LINK_PROBIT              */
} mk_config;

/* Caller-allocated outputs; any pointer may be NULL to skip it.
 * P = p + q(q+1)/2 + q (+ q for Matern); kept = n_batch*batch_length - burn_in + 1. */
typedef struct mk_outputs {
  double* parameters;   /* [n_subsets] x (200 x P) column-major: obj[[i]]$parameters (MK.R:89)  */
  double* w_predict;    /* [n_subsets] x (200 x q*n_test) column-major: obj[[i]]$w.predict      */
  double* samples;      /* [n_subsets] x (n_samples x P) column-major: m.1$p.beta.theta.samples  */
  double* w_samples;    /* [n_subsets] x ((n_s*q) x n_samples) column-major: m.1$p.w.samples    */
  double* w_pred_samples; /* [n_subsets] x ((q*n_test) x kept): m.s.pred$p.w.predictive.samples */
  double* acceptance;   /* [n_subsets] x (n_batch x (p + n_theta + 1)): per-batch accept rates,
                           last column = mean over the latent w                                  */
  double* w_predict_sum; /* 200 x (q*n_test): w_predict summed over this call's subsets in subset
                           order -- this shard's term of the combine (MK.R:129-132) without the
                           per-subset grids on the host                                          */
  /* spPredict's p.y.predictive.samples for the binomial family: p = linkinv(x(s)'beta + w(s)) of
   * every kept state, beta and w(s) of the same iteration.  They need x_test (MK_E_ARG without). */
  double* p_predict;    /* [n_subsets] x (200 x q*n_test): the 200-level grids of p, as w_predict      */
  double* p_pred_samples; /* [n_subsets] x ((q*n_test) x kept): the p draws, as w_pred_samples          */
  double* p_predict_sum; /* 200 x (q*n_test): p_predict summed in subset order, as w_predict_sum        */
} mk_outputs;

typedef struct mk_session mk_session;

/* ---- batched meta-kriging path (replaces foreach %dopar% at MK.R:108) ---- */
/* Upload the shard to HBM and initialise every chain (no MCMC yet). */
int mk_session_create(const mk_problem* prob, const mk_config* cfg, mk_session** out);
/* Advance every chain by n_iter iterations (returns after the device is idle). */
int mk_session_run(mk_session* s, int32_t n_iter);
/* Iterations done so far. */
int32_t mk_session_iteration(const mk_session* s);
/* Test sites per kriging tile in use (0: fused kriging).  A tiled session takes the configured
 * predict_tile, or the largest tile (halved in 256-site steps) whose kriging buffers fit in HBM;
 * hosts replaying tile by tile (mk_session_tile_grids) step by this value. */
int32_t mk_session_predict_tile(const mk_session* s);
/* One subset's chain state after the iterations done so far, in spMvGLM's MH parameter order:
 * beta [p]; theta [n_theta] (A lower-tri col-major with log diagonal | logit phi | logit nu);
 * w [n_s q] location-major; tune [p + n_theta + n_s q] log proposal sds; accept [same] accept counts
 * of the current amcmc batch.  Any pointer may be NULL.  (Resuming the chain on another host: the CPU
 * baseline of bench.py times the oracle over the window the device timed.) */
int mk_session_chain_state(mk_session* s, int32_t subset, double* beta, double* theta, double* w, double* tune,
                           double* accept);
/* Failure semantics of the factorisations.  mk_session_create
 * returns MK_E_ARG, naming the subset, when a subset has a non-finite coordinate or two sites at the
 * same coordinates, or when a correlation matrix at the starting values meets a pivot that is not
 * > 0.  In the chain a phi / nu candidate whose factorisation meets such a pivot is a rejection;
 * out [n_subsets * q] (subset-major) receives how many each (subset, outcome) pair has had so far. */
int mk_session_notpd_counts(mk_session* s, int64_t* out);
/* Launch schedule (results are the same chain either way): mode 1 = lookahead
 * (the next iteration's phi candidates are factored while this iteration's inverse and latent
 * sweep run; Matern: the nu step follows the phi decision; n_streams <= 1), 0 = sequential, -1 = default (lookahead where
 * eligible; env MK_LOOKAHEAD=0/1 overrides the default).  Before the first mk_session_run only.
 * mk_session_lookahead returns 1 when the lookahead schedule is in use. */
int mk_session_set_lookahead(mk_session* s, int32_t mode);
int32_t mk_session_lookahead(const mk_session* s);
/* Quantile summaries + optional sample copies (requires all iterations done
 * for parameters / w_predict). */
int mk_session_outputs(mk_session* s, mk_outputs* out);
/* spPredict after spMvGLM without refitting (spPredict(m.1, coords.test, ...), MK.R:87): a session
 * created with predict_tile > 0 keeps every kept chain state (burn_in = 1 keeps all of them);
 * mk_session_set_test_sites replaces its test sites (n_test x 2 column-major) and
 * mk_session_set_kept_window(first, last) restricts the kriging replay of the next
 * mk_session_outputs to iterations first..last (1-based, burn_in <= first <= last <= n.samples;
 * spPredict's start / end).  The draws are those a session with burn_in = first would make. */
int mk_session_set_test_sites(mk_session* s, int32_t n_test, const double* coords_test);
/* Covariates of the session's current test sites: x_test (q*n_test) x p column-major (spPredict's
 * pred.covars), copied to HBM; the p_* outputs and the p grids need them.  mk_session_set_test_sites
 * drops them (new sites need their own), and held-out data attached by mk_session_set_validation and
 * maps asked for by mk_session_set_maps with them.  MK_E_ARG when the session has no test sites. */
int mk_session_set_test_covars(mk_session* s, const double* x_test);
int mk_session_set_kept_window(mk_session* s, int32_t first, int32_t last);
/* After all iterations: the shard's 200-level grids, [n_subsets] x (200 x C) column-major -- which 0:
 * obj[[i]]$parameters (C = P), which 1: obj[[i]]$w.predict (C = q*n_test; fused sessions, tiled ones
 * use mk_session_tile_grids), which 2: the p.predict grids (as 1; needs x_test) -- into out: host memory, or HBM of the session's device when
 * device_out != 0 (e.g. the send buffer of a device-resident combine; no host round trip). */
int mk_session_grids(mk_session* s, int32_t which, double* out, int32_t device_out);
/* Tiled sessions (predict_tile > 0), after all iterations: the 200-level w.predict grids of the test
 * sites of tile [t0, t0 + Tc) (Tc = min(predict_tile, n_test - t0), t0 a multiple of predict_tile),
 * every subset: [n_subsets] x (200 x q*Tc) column-major, into out -- host memory, or HBM of the
 * session's device when device_out != 0 (e.g. an RCCL send buffer).  Replays that tile's kriging
 * only (spPredict, MK.R:87-89), so a host can combine tile by tile: at configs[4] the per-subset
 * grids of all 1M sites never coexist. */
int mk_session_tile_grids(mk_session* s, int32_t t0, double* out, int32_t device_out);
/* The same with the tile's p.predict grids: one replay of the tile writes the w grids into out_w and
 * the grids of p = linkinv(x(s)'beta + w(s)) into out_p (same shape; needs x_test).  Either pointer
 * may be NULL.  The next tile overwrites the draws, so both grids come from this one replay. */
int mk_session_tile_grids_wp(mk_session* s, int32_t t0, double* out_w, double* out_p, int32_t device_out);
/* Per-kernel timing (HIP events on the launching streams): launches, total ms and
 * algorithmic flops per kernel kind.  0: the 128-tile column-update launches -- k_chol_update_trsm
 * (column k's update of tiles k+1.. with the panel solve fused in its epilogue, plus the next diagonal
 * tile's update by panels < k; the default schedule) and k_chol_update<128> (unfused and split
 * schedules); 1 diagonal tile k_chol_diag (in the fused schedule it also applies the rank-128
 * diagonal correction by panel k-1, priced here); 2 panel trsm k_chol_trsm (panel 0, and the unfused
 * schedules); 3 latent sweep; 4 R^-1 diagonal tiles; 5 whole iterations; 6 inverse levels
 * k_inv_level (flops per level over the accepted factors, n_s^3/3 per factor with kind 1's diagonal
 * inverses); 7 kind 0's 64/32-sub-tile instances; 8 kinds 0 + 7 with overlapping launches counted
 * once; 9 kriging GEMM k_pred_var; 10 candidate covariance assembly; 11 latent sweeps the
 * multi-workgroup kernel refused admission and its fallback ran -- launches = (subset, iteration)
 * count, no timing; 12 tiles of a tiled session kriged by phi interpolation (exponential, any q) --
 * launches = tiles, flops = exact kriging-variance evaluations, one per (subset, outcome) pair and node
 * or check point, total_ms = the largest per-tile check difference over all pairs and sites (not a
 * time; a fused q = 1 session drawing from phi tables counts its kept iterations here instead); 13
 * tiles whose check failed at any pair and were replayed exactly -- launches, total_ms = the largest
 * failing difference; 14 the chain-diagnostic launches k_chain_diag / k_chain_diag_prob -- launches and ms,
 * timed whether or not profiling is on; 0 launches unless diagnostics were asked for; 15 the
 * model-assessment launches k_crit_accum / k_crit_replay / k_crit_finish / k_crit_total -- launches and
 * ms, always timed, 0 launches unless criteria were asked for; 16 the held-out scoring launches
 * k_score_cols / k_score_finish -- launches and ms, always timed, 0 launches unless validation data were
 * attached; 17 the posterior-map launches k_map_cols -- launches and ms, always timed, 0 launches unless
 * maps were asked for; 18 the cross-outcome launches k_quantiles_pair / k_pair_cols -- launches (one per
 * kernel) and ms, always timed, 0 launches unless pairs were asked for; 19 the areal-prediction launches
 * k_region_cov / k_region_draw per kept state and k_quantiles / k_map_cols per replay (on the interpolated
 * route the node covariances, the check and two launches per chunk of kept states) -- launches (one per
 * kernel) and ms, always timed, 0 launches unless regions were attached; 20 the
 * PSIS-LOO launches -- always timed, 0 launches unless mk_session_loo is called; 21 the state-digest launches
 * k_state_digest / k_digest_reduce of a checkpoint, a restore or mk_session_digest -- launches and ms, always
 * timed, 0 launches unless one of those calls is made).  Flops are algorithmic, not executed: GEMM tiles 2 m n k, the diagonal tile's
 * update as a SYRK, solves and inverse products over their triangles.  mk_session_profile(s, enable)
 * before mk_session_run: enable 0 = off, 1 = every kind, otherwise a mask with bit (1 + kind) per kind
 * bracketed (e.g. 2 << 0 = the panel update only; fewer events, less overhead). */
int mk_session_profile(mk_session* s, int32_t enable);
/* Bracket only the launches of every `every`-th iteration (iteration index % every == 0; default 1:
 * all).  At small shards per-launch events cost measurably (32 subsets: ~4 % of the rate, 250: 0.5 %);
 * a sample keeps the per-launch averages and costs a fraction of that. */
int mk_session_profile_every(mk_session* s, int32_t every);
int mk_session_kernel_stats(const mk_session* s, int32_t which, int64_t* launches, double* total_ms, double* flops);
void mk_session_destroy(mk_session* s);
/* Sessions alive in this process (a failed mk_session_create leaves none behind). */
int32_t mk_session_count(void);

/* One-shot convenience: create, run n_batch*batch_length iterations, outputs, destroy. */
int mk_fit_predict_batched(const mk_problem* prob, const mk_config* cfg, mk_outputs* out);

/* ---- the whole node (replaces makeCluster + foreach %dopar% + the combine, MK.R:100-133) ----
 * The K subsets of prob are cut into n_devices balanced contiguous blocks [floor(rK/G),
 * floor((r+1)K/G)); block r runs as one session on devices[r], one host thread per block, with
 * global subset indices (prob->subset_base + its first subset), so every chain equals the
 * one-device chain.  The chains advance one amcmc batch at a time on every device; between
 * batches the calling thread calls progress (if not NULL) -- spBayes's n.report output and R's
 * interrupt check -- and stops the fit (MK_E_INTERRUPT, every device freed) when it returns
 * nonzero.  cfg->device is ignored.
 * The combine is device to device: every block's 200-level grids stay in HBM; an all-to-all hands
 * device j all K subsets' grids for its block of columns (RCCL send/recv over xGMI when the devices
 * are distinct; device copies when a device is listed more than once -- several shards on one GPU),
 * device j combines them in global subset order -- MK.R:123-133's sequential mean, bit-identical
 * to one device, or the Weiszfeld W2 median -- and its combined columns go to the host.  Tiled
 * kriging (predict_tile) exchanges the grids of one test-site tile at a time, so the configs[4]
 * combine of 1M sites needs K x 200 x q*tile doubles per device, not K x 200 x q*n_test.
 * out (optional, any field NULL): the per-subset outputs of all K subsets as mk_session_outputs
 * lays them out; out->w_predict_sum = the sequential sum of all K w.predict grids.  prob->x_test (shared
 * by every block, as the test sites are) gives out->p_predict / p_pred_samples / p_predict_sum and
 * comb->result3 by the same route. */
#define MK_COMBINE_MEAN 0     /* MK.R:123-133 */
#define MK_COMBINE_MEDIAN 1   /* north-star extension: per column Weiszfeld geometric median in W2 */
typedef struct mk_combined {
  double* result;     /* 200 x P: the combined parameter grid (MK.R:127 result), or NULL            */
  double* result2;    /* 200 x (q*n_test): the combined w.predict grid (MK.R:133 result2), or NULL  */
  int32_t method;     /* MK_COMBINE_MEAN or MK_COMBINE_MEDIAN                                      */
  int32_t max_iter;   /* MEDIAN: Weiszfeld iterations (<= 0: 100)                                   */
  double tol;         /* MEDIAN: convergence tolerance (< 0: 1e-12)                                 */
  int32_t exchange;   /* out: 1 = RCCL, 0 = device copies                                           */
  int32_t comm_ranks; /* out: ranks of the exchange (RCCL: ncclCommCount of the communicators; copies:
                       * the number of device blocks)                                               */
  double* result3;    /* 200 x (q*n_test): the combined p.predict grid (the subsets' grids of
                       * p(y = 1) at the test sites, combined by `method` as result2), or NULL;
                       * needs prob->x_test                                                         */
} mk_combined;
/* Progress between batches: iterations done so far (a multiple of batch_length) of n_samples. */
typedef int (*mk_progress_fn)(void* user, int32_t iterations, int32_t n_samples);
int mk_meta_fit(const mk_problem* prob, const mk_config* cfg, const int32_t* devices, int32_t n_devices,
                mk_progress_fn progress, void* user, mk_outputs* out, mk_combined* comb);

/* ---- chain diagnostics: the numerical counterpart of the trace plots (MK.R:147-149) ----
 * Each chain is one column in time order, x_0 .. x_{n-1} (the kept states).  Per chain, on device:
 *   m = (sum x_i)/n, d_i = x_i - m, c_t = (1/n) sum_{i=0}^{n-1-t} d_i d_{i+t}  (biased autocovariance)
 *   Gamma_k = (c_2k + c_2k+1)/c_0 while 2k+1 <= n-1; Geyer's initial monotone sequence: stop at the
 *   first Gamma_k <= 0 (not added), else Gamma_k <- min(Gamma_k, Gamma_k-1); tau = -1 + 2 sum Gamma_k,
 *   tau <- max(tau, 1/log10(n))
 *   ess = n/tau;  mcse = sqrt(c_0 n/(n-1) / ess)  (Monte Carlo s.e. of the column mean)
 *   split R-hat: h = floor(n/2), a = x[0:h], b = x[n-h:n] (an odd n drops the middle state),
 *   W = (var a + var b)/2 (h-1 denominators), B = h (mean a - mean b)^2 / 2,
 *   rhat = sqrt(((h-1)/h W + B/h) / W).
 * A column that never moved (c_0 = 0) gives (0, 0, +inf); W = 0 with c_0 > 0 gives rhat = +inf; any
 * non-finite value gives three NaN.  4 <= n <= 16384 (the quantile summaries' limit), else MK_E_ARG.
 * "Worst over subsets" is per column: min ess, max mcse, max rhat; a NaN in any subset makes that
 * entry NaN.  The thresholds a reader applies to these numbers are the reader's own. */
#define MK_N_DIAG 3   /* rows: ess, mcse, rhat */
typedef struct mk_diagnostics {        /* caller-allocated, any pointer may be NULL */
  double* parameters;        /* [n_subsets] x (3 x P)         column-major */
  double* w_predict;         /* [n_subsets] x (3 x q*n_test)                */
  double* p_predict;         /* the same of p = linkinv(x'beta + w); needs x_test */
  double* parameters_worst;  /* 3 x P: worst over this call's subsets       */
  double* w_predict_worst;   /* 3 x q*n_test                                */
  double* p_predict_worst;   /* 3 x q*n_test                                */
} mk_diagnostics;
/* After all iterations.  parameters: rows burn_in .. n.samples of the recorded samples, or the kept
 * window when mk_session_set_kept_window set one (sessions made for spPredict run with burn_in = 1,
 * so there the window is the only meaningful range).  w_predict / p_predict: a fused session's
 * kriging draws.  A tiled session's draws exist one tile at a time: asking for them here is MK_E_ARG;
 * attach a sink (mk_session_set_diagnostics) and the tile replays fill it. */
int mk_session_diagnostics(mk_session* s, mk_diagnostics* out);
/* Tiled sessions: while a sink is attached (the struct is copied; NULL detaches), every tile replay
 * -- mk_session_outputs, mk_session_tile_grids, mk_session_tile_grids_wp -- also diagnoses that
 * tile's draws before it returns, from the same replay: columns [t0*q, t0*q + q*Tc) of the sink's
 * w_predict / p_predict arrays (sized for all q*n_test columns) and of their worst rows.  The sink's
 * parameters fields are not written (mk_session_diagnostics gives them).  p fields without x_test:
 * MK_E_ARG.  mk_session_set_test_sites detaches the sink (its arrays were sized for the old sites). */
int mk_session_set_diagnostics(mk_session* s, const mk_diagnostics* sink);
/* mk_meta_fit with the diagnostics of all K subsets (mk_meta_fit is this call with diag = NULL): the
 * per-subset arrays in global subset order, the worst rows over all K (each device block reduces
 * its own on device, the calling thread folds the blocks).  Tiled kriging diagnoses each tile from
 * the replay that makes its grids. */
int mk_meta_fit_diag(const mk_problem* prob, const mk_config* cfg, const int32_t* devices, int32_t n_devices,
                     mk_progress_fn progress, void* user, mk_outputs* out, mk_combined* comb, mk_diagnostics* diag);
/* The diagnostic kernel on caller-given chains: x is n_rows x n_cols column-major, one chain per
 * column (a coda mcmc matrix such as p.beta.theta.samples; t(p.w.samples) for the latent draws);
 * out is 3 x n_cols column-major. */
int mk_chain_diagnostics(const double* x, int32_t n_rows, int64_t n_cols, double* out, int32_t device);

/* ---- model assessment: spDiag's deviance information criterion, and WAIC, per subset ----
 * Per subset, over the window's states k = 1..n and its observations i (site x outcome, location-major,
 * i < n_s q; padding rows are masked):
 *   eta_ik = x_i' beta_k + w_ik, recomputed from X, beta_k and w_k: fused multiply-adds in column order
 *            from zero, then + w (as the predictive probabilities build theirs; not the chain's running
 *            eta, which carries the rounding of its incremental updates)
 *   l_ik   = the chain's likelihood term with the binomial coefficient dropped:
 *            logit y eta - wt log(1 + e^eta); probit y log Phi(eta) + (wt - y) log Phi(-eta)
 *   D_k = -2 sum_i l_ik
 *   bar.D       = (1/n) sum_k D_k
 *   D.bar.Omega = -2 sum_i l(y_i, wt_i, x_i' beta_bar + w_bar_i), beta_bar and w_bar the window means
 *   pD  = bar.D - D.bar.Omega
 *   DIC = bar.D + pD
 *   lppd   = sum_i [log sum_k exp(l_ik) - log n]   (streaming log-sum-exp: running maximum, scaled sum)
 *   p.waic = sum_i M2_i / (n - 1), M2_i = sum_k (l_ik - mean_i)^2 by Welford's update
 *   WAIC   = -2 (lppd - p.waic)
 *   lconst = sum_i [lgamma(wt + 1) - lgamma(y + 1) - lgamma(wt - y + 1)]
 * lconst is the constant the likelihood terms drop (0 for binary data): full-likelihood figures add
 * -2 lconst to bar.D, D.bar.Omega, DIC and WAIC and + lconst to lppd; pD and p.waic do not change.
 * The first four rows are spDiag's for the binomial family as spBayes names them (parity by
 * definition: no spBayes run pins them).  n >= 2 states, else MK_E_ARG.  A likelihood term that is
 * not finite makes the subset's first seven rows NaN (lconst depends on the data alone).  Every sum
 * runs in an order fixed by n and n_pad q alone, and the in-chain and the replayed route perform the
 * same operations in the same order per observation: their results are equal bit for bit. */
#define MK_N_CRIT 8   /* rows: bar.D, D.bar.Omega, pD, DIC, lppd, p.waic, WAIC, lconst */
typedef struct mk_criteria {   /* caller-allocated, any pointer may be NULL */
  double* subsets;     /* [n_subsets] x 8                                                        */
  double* total;       /* 8: sums over this call's subsets in subset order                       */
  double* pointwise;   /* [n_subsets] concatenated (n_s q) x 2 column-major: lppd_i, M2_i/(n-1)  */
} mk_criteria;
/* In-chain accumulation: from the first kept iteration on, one elementwise launch per kept iteration
 * carries the running sums (6 doubles per observation and one partial per 256 observations and kept
 * state of HBM, allocated here and only here).  Before the first mk_session_run only; later is
 * MK_E_ARG.  Sessions that will only replay do not need it. */
int mk_session_set_criteria(mk_session* s, int32_t enable);
/* After all iterations.  With no kept window set, thin = 1 and in-chain accumulation on: closes the
 * in-chain sums (window burn_in .. n.samples).  Otherwise replays states first, first + thin, ... <=
 * last of the window (mk_session_set_kept_window, else burn_in .. n.samples) from the recorded chain:
 * that needs record_samples and record_w, else MK_E_ARG.  For this call mk_session_set_kept_window
 * also serves sessions without predict_tile that recorded both (their outputs are not windowed). */
int mk_session_criteria(mk_session* s, int32_t thin, mk_criteria* out);
/* mk_meta_fit_diag with the criteria of all K subsets (mk_meta_fit and mk_meta_fit_diag are this call
 * with NULLs): every device block accumulates in chain and fills its subsets' rows (and pointwise
 * pairs) at their global offsets; total is the sum of the K rows in global subset order, formed by
 * the calling thread -- the order one session uses, so equal to it bit for bit. */
int mk_meta_fit_ex(const mk_problem* prob, const mk_config* cfg, const int32_t* devices, int32_t n_devices,
                   mk_progress_fn progress, void* user, mk_outputs* out, mk_combined* comb, mk_diagnostics* diag,
                   mk_criteria* crit);

/* ---- leave-one-out: PSIS-LOO elpd and the Pareto shape k-hat per observation ----
 * Pareto-smoothed importance-sampling leave-one-out (Vehtari, Gelman and Gabry 2017; R's loo): the
 * criteria's pointwise likelihood matrix, smoothed importance weights, and per observation a shape
 * estimate k-hat that says whether its term can be trusted (k-hat > 0.7: it cannot).
 * Per subset, over the window's states k = 1..n and its observations i < n_s q (padding rows are
 * masked).  The window is mk_session_set_kept_window's if set, else burn_in .. n.samples, every thin-th
 * state from its first.  l_ik is exactly the criteria's term: crit_eta then loglik_term, the same
 * operands in the same order, the binomial coefficient dropped.
 * MK_LOO_MIN_STATES <= n <= MK_LOO_MAX_STATES, else MK_E_ARG naming n (above the cap: a larger thin);
 * 25 is the smallest n with a tail of 5.
 * For each observation, with r_k = -l_k - max_k(-l_k):
 *   1. M = min(floor(n/5), ceil(3 sqrt(n))).  The tail is the M largest r; cut is the largest r not in
 *      the tail.  Ties are broken by position in the sorted row: tied states have equal l, so no output
 *      depends on it.
 *   2. If the tail's largest value equals its smallest, nothing is smoothed and k-hat = +inf.
 *   3. Otherwise the generalised-Pareto fit of Zhang and Stephens (2009) as loo applies it, with
 *      x_j = exp(r_(j)) - exp(cut) over the tail in ascending order, j = 1..M:
 *        G = 30 + floor(sqrt(M)),  x* = x_floor(M/4 + 0.5)
 *        theta_g = 1/x_M + (1 - sqrt(G/(g - 1/2)))/(3 x*),  g = 1..G
 *        k_g = (1/M) sum_j log1p(-theta_g x_j)
 *        L_g = M (log(-theta_g/k_g) - k_g - 1)
 *        omega_g = 1/sum_h exp(L_h - L_g)
 *        theta = sum_g theta_g omega_g
 *        k = (1/M) sum_j log1p(-theta x_j),  sigma = -k/theta
 *        k-hat = (k M + 5)/(M + 10)
 *   4. If k-hat is finite, the j-th smallest tail value is replaced by
 *        min(log(sigma expm1(-k-hat log1p(-p_j))/k-hat + exp(cut)), 0),  p_j = (j - 1/2)/M;
 *      if it is not, nothing is replaced.
 *   5. lw_k = r_k - logsumexp(r);  elpd_loo_i = logsumexp_k(l_k + lw_k);
 *      lppd_i = logsumexp_k(l_k) - log n.
 * Relative efficiency is taken as 1: the chain's autocorrelation is not used to lengthen the tail.
 * Rows per subset, N = n_s q:
 *   elpd_loo     sum_i elpd_loo_i
 *   p_loo        lppd - elpd_loo
 *   looic        -2 elpd_loo
 *   se_elpd_loo  sqrt(N var_i elpd_loo_i): two-pass variance, denominator N - 1, NaN when N = 1
 *   lppd         sum_i lppd_i
 *   k_max        the largest k-hat of the subset
 *   n_k_bad      the count of k-hat > 0.7, as a double; +inf counts
 *   lconst       as in the criteria
 * pointwise per subset is (n_s q) x 3 column-major: elpd_loo_i, k-hat_i, lppd_i.  total: sums in subset
 * order for elpd_loo, p_loo, looic, lppd, n_k_bad and lconst; the maximum for k_max; the root of the
 * summed squares for se_elpd_loo.  A non-finite l in an observation's window makes its triple NaN and
 * the subset's first seven rows NaN (the criteria's rule).
 * Every sum runs in an order fixed by n, M and n_pad q alone (the row sorted; thread stride, then a
 * fixed tree): two calls return the same bytes, and so do any two chunkings of the subsets. */
#define MK_N_LOO 8               /* rows: elpd_loo, p_loo, looic, se_elpd_loo, lppd, k_max, n_k_bad, lconst */
#define MK_LOO_MIN_STATES 25
#define MK_LOO_MAX_STATES 8192   /* one observation's row is sorted in 64 KB of LDS */
typedef struct mk_loo {          /* caller-allocated, any pointer may be NULL */
  double* subsets;     /* [n_subsets] x 8                                                       */
  double* total;       /* 8                                                                     */
  double* pointwise;   /* [n_subsets] concatenated (n_s q) x 3 column-major                     */
} mk_loo;
/* After all iterations.  Always replays the recorded chain: that needs record_samples and record_w,
 * else MK_E_ARG.  Window and thin are exactly mk_session_criteria's, including sessions without
 * predict_tile that recorded both, and imported sessions.  The terms of a chunk of subsets are scratch
 * (Np n doubles per subset, 1 GiB at a time; MK_LOO_CHUNK=<subsets> overrides), freed on return; a
 * chunk that does not fit is MK_E_NOMEM.  Nothing is launched or allocated unless this is called. */
int mk_session_loo(mk_session* s, int32_t thin, mk_loo* out);
/* The same kernel on a caller's log-likelihood matrix on the host: ell is n_states x n_obs column-major,
 * one observation per column.  pointwise (n_obs x 3 column-major) and row (8, lconst 0) may be NULL.
 * Columns are uploaded in chunks (bounded in bytes; MK_LOO_CHUNK=<columns> overrides); the triples of
 * all columns stay in one device buffer and the row is reduced once, so nothing depends on the chunk. */
int mk_loo_matrix(const double* ell, int64_t n_obs, int32_t n_states, double* pointwise, double* row, int32_t device);

/* ---- held-out validation: log score, Brier score and error rate at the test sites ----
 * The out-of-sample companion of the model assessment above.  Held-out data are y_test and wt_test,
 * q*n_test each, location-major like x_test: y successes of wt trials; a column with wt = 0 is "not
 * observed here".  Per subset, over the kept states k = 1..n of the window and per test column c:
 *   eta_kc = x_c' beta_k + w_kc and p_kc = linkinv(eta_kc): the predictive probabilities' own
 *            expressions (p_pred_samples holds these p, bit for bit)
 *   l_kc   = the chain's likelihood term of (y_c, wt_c) at eta_kc, the binomial coefficient dropped
 *   pmean_c = (sum_k p_kc) / n, summed in time order from zero
 *   lpd_c   = log((1/n) sum_k exp(l_kc)), by the streaming log-sum-exp (running maximum, scaled sum);
 *             0 by itself where wt_c = 0
 * and a row of MK_N_SCORE values:
 *   n      columns with wt > 0
 *   lpd    sum_c lpd_c
 *   brier  (1/n) sum over wt_c > 0 of (pmean_c - y_c/wt_c)^2
 *   err    the share of held-out trials the rule yhat_c = [pmean_c >= 0.5] gets wrong:
 *          sum_c (yhat_c ? wt_c - y_c : y_c) / sum_c wt_c
 *   lconst sum_c [lgamma(wt + 1) - lgamma(y + 1) - lgamma(wt - y + 1)]: what the likelihood terms
 *          drop (0 for binary data); full-likelihood log scores add it, as with the criteria
 * One thread owns a column and consumes its states in time order, so nothing in a column's pair depends
 * on the tile, the stream group or the device block it ran in.  Sums over columns run in an order fixed
 * by q*n_test alone (thread stride, then a fixed tree); the closing formulas use no contraction.  A
 * non-finite draw makes that column's pair NaN and the subset's lpd, brier and err NaN; -inf is a
 * legitimate lpd (an outcome the predictor gave probability 0); brier is NaN when n = 0 and err when
 * no trial was held out.  Pointwise output per subset: (q*n_test) x 2 column-major, pmean_c and lpd_c;
 * pmean is also the posterior mean map of p(y = 1).
 * The combined posterior is a grid of levels (comb->result3, 200 of them): it is scored by the same
 * formulas with the grid's n_rows levels as equally weighted states and p read, not computed:
 *   l = y log p + (wt - y) log1p(-p), a term whose multiplier is 0 contributing 0. */
#define MK_N_SCORE 5   /* rows: n, lpd, brier, err, lconst */
typedef struct mk_validation { const double* y_test; const double* wt_test; } mk_validation;   /* q*n_test each */
typedef struct mk_scores {            /* caller-allocated, any pointer may be NULL */
  double* subsets;             /* [n_subsets] x 5 */
  double* pointwise;           /* [n_subsets] x ((q*n_test) x 2) */
  double* combined;            /* 5: the combined p grid's row (node call only) */
  double* combined_pointwise;  /* (q*n_test) x 2 */
} mk_scores;
/* Attach held-out data to the session's current test sites (copied to HBM; NULL detaches and frees).
 * Needs test sites and x_test, else MK_E_ARG; every entry must be finite with wt >= 0 and 0 <= y <= wt,
 * else MK_E_ARG naming the first bad index.  A tiled session also gets its score buffer here and only
 * here: 16 bytes per (subset, test column); MK_E_NOMEM names the remedies.  While data are attached,
 * every tile replay of a tiled session -- mk_session_outputs, mk_session_tile_grids,
 * mk_session_tile_grids_wp -- also scores that tile's columns into the buffer, from the same replay and
 * over its kept window.  mk_session_set_test_sites detaches (the data belonged to the sites that go).
 * Nothing is launched or allocated for scoring unless data are attached. */
int mk_session_set_validation(mk_session* s, const mk_validation* val);
/* After all iterations.  A fused session scores its kriging draws (all kept states) now.  A tiled
 * session closes the rows from its buffer: MK_E_ARG, naming the first missing tile, if some tile has
 * not been replayed over the current kept window since the data were attached.  combined and
 * combined_pointwise are not written here. */
int mk_session_scores(mk_session* s, mk_scores* out);
/* The same scores of a grid of probabilities on the host: p is n_rows x n_cols column-major (e.g.
 * comb->result3 with n_rows = 200), y and wt n_cols each (checked as above).  pointwise (n_cols x 2
 * column-major) and row (5) may be NULL.  Columns are uploaded in chunks (bounded in bytes;
 * MK_SCORE_CHUNK=<columns> overrides); the pairs of all columns stay in one device buffer and the row
 * is reduced once, so nothing depends on the chunk. */
int mk_score_grid(const double* p, int32_t n_rows, int64_t n_cols, const double* y, const double* wt,
                  double* pointwise, double* row, int32_t device);
/* mk_meta_fit_ex with held-out validation (mk_meta_fit_ex is this call with two NULLs): every block
 * attaches the shared data and fills its subsets' rows and pairs at their global offsets;
 * scores->combined / combined_pointwise come from mk_score_grid on comb->result3 (MK_E_ARG when that
 * is not asked for).  Nothing is added to the exchange. */
int mk_meta_fit_val(const mk_problem* prob, const mk_config* cfg, const int32_t* devices, int32_t n_devices,
                    mk_progress_fn progress, void* user, mk_outputs* out, mk_combined* comb, mk_diagnostics* diag,
                    mk_criteria* crit, const mk_validation* val, mk_scores* scores);

/* ---- posterior maps: mean, sd and exceedance probabilities of p(y = 1) at the test sites ----
 * The map a binary spatial model is drawn as: per test column the posterior mean and standard deviation
 * of the latent w and of p(y = 1), and the posterior probability that p exceeds each of J policy
 * thresholds ("prevalence above 20 %").  Thresholds u_1..u_J are on the probability scale,
 * 0 <= J <= MK_MAP_MAXT, every u_j finite.
 * Each subset on its own; k = 1..n the kept states of the window in time order, c a test column (site x
 * outcome, location-major like x_test):
 *   eta_kc, p_kc  exactly pred_eta and pred_linkinv: p is the p of p_pred_samples bit for bit, as in the
 *                 held-out scores
 *   mean of v (v = w or p)  (sum_k v_k) / n, summed in time order from zero: pmean's own expression --
 *                 with validation data attached the p_mean plane equals the scores' pmean bit for bit
 *   sd of v       Welford's recurrence in time order: m = 0, M2 = 0; per state d = v - m, m = m + d/k,
 *                 M2 = M2 + d (v - m); sd = sqrt(M2 / (n - 1)), NaN when n = 1.  Plain operations, no
 *                 contraction
 *   exc_j         #{k : p_kc > u_j} / n; the inequality is strict
 * A non-finite draw or eta makes every plane of that column NaN.
 * Planes per subset: MK_N_MAP_BASE + J, in the order w_mean, w_sd, p_mean, p_sd, exc_1..exc_J; output
 * per subset (q*n_test) x (4 + J) column-major.  One thread owns one column and walks its states
 * serially, so nothing in a column depends on the tile, the stream group, the workgroup or the device
 * block it ran in.
 * The combined posterior is a grid of levels; as with mk_score_grid its n_rows levels are equally
 * weighted states, read and not computed: mk_map_grid gives n_cols x (2 + J): mean, sd, exc_1..J of the
 * grid it is handed, and the node call fills the combined planes in the 4 + J order -- w_mean and w_sd
 * from comb->result2; p_mean, p_sd and exc from comb->result3 -- for the mean combine and the Weiszfeld
 * median alike. */
#define MK_MAP_MAXT 8     /* thresholds at most */
#define MK_N_MAP_BASE 4   /* planes before the exceedances: w_mean, w_sd, p_mean, p_sd */
typedef struct mk_map_spec { const double* thresholds; int32_t n_thresholds; } mk_map_spec;
typedef struct mk_maps {              /* caller-allocated, either pointer may be NULL */
  double* subsets;             /* [n_subsets] x ((q*n_test) x (4 + J)) */
  double* combined;            /* (q*n_test) x (4 + J): the combined grids' planes (node call only) */
} mk_maps;
/* Ask the session for the maps of its current test sites (NULL detaches and frees).  Needs test sites,
 * x_test and recorded samples, else MK_E_ARG; the thresholds are checked before any device is touched: a
 * non-finite value or n_thresholds outside 0 .. MK_MAP_MAXT is MK_E_ARG naming the index.  A tiled
 * session takes its plane buffer here and only here: 8 (4 + J) bytes per (subset, test column);
 * MK_E_NOMEM names the remedies.  While attached, every tile replay of a tiled session --
 * mk_session_outputs, mk_session_tile_grids, mk_session_tile_grids_wp -- also fills that tile's columns
 * of the planes, from the same replay and over its kept window.  mk_session_set_test_sites detaches.
 * Nothing is launched or allocated for the maps unless they were asked for. */
int mk_session_set_maps(mk_session* s, const mk_map_spec* spec);
/* After all iterations.  A fused session makes the planes from its kriging draws (all kept states) now,
 * in scratch held for the call.  A tiled session copies its buffer out: MK_E_ARG, naming the first such
 * tile, if some tile has not been replayed over the current kept window since the maps were attached.
 * combined is not written here. */
int mk_session_maps(mk_session* s, mk_maps* out);
/* mean, sd and exceedances of a grid on the host: grid is n_rows x n_cols column-major (e.g.
 * comb->result3 with n_rows = 200), out n_cols x (2 + n_thresholds) column-major.  Columns are uploaded
 * in chunks (bounded in bytes; MK_MAP_CHUNK=<columns> overrides); a column is one thread's work, so
 * nothing depends on the chunk. */
int mk_map_grid(const double* grid, int32_t n_rows, int64_t n_cols, const double* thresholds, int32_t n_thresholds,
                double* out, int32_t device);
/* mk_meta_fit_val with posterior maps (mk_meta_fit_val is this call with two NULLs): every block
 * attaches the spec and writes its subsets' planes at their global offsets; maps->combined comes from
 * mk_map_grid on the host copies of comb->result2 and comb->result3 (MK_E_ARG when either is not asked
 * for).  Nothing is added to the exchange. */
int mk_meta_fit_maps(const mk_problem* prob, const mk_config* cfg, const int32_t* devices, int32_t n_devices,
                     mk_progress_fn progress, void* user, mk_outputs* out, mk_combined* comb, mk_diagnostics* diag,
                     mk_criteria* crit, const mk_validation* val, mk_scores* scores, const mk_map_spec* spec,
                     mk_maps* maps);

/* ---- cross-outcome prediction (q >= 2): co-occurrence and contrast of two outcomes at a test site ----
 * A kept state's kriging draws at a site are joint across the q outcomes (w* = A (m + diag(sd) z)), so
 * functionals of two outcomes at ONE site have a posterior the per-column outputs cannot give.  (Across
 * sites the draws are marginal by design: nothing here aggregates over sites.)
 * Pairs (a, b), a < b, are numbered r = 0 .. n_pairs - 1 in the order
 *   for a in 0 .. q-2: for b in a+1 .. q-1
 * so n_pairs = q (q - 1) / 2 (at most 6).  Pair column e = t n_pairs + r for test site t (site-major, as
 * the columns are location-major); C2 = n_pairs n_test.
 * Each subset on its own; k = 1..n the kept states of the window in time order; p_a,k and p_b,k are
 * pred_prob's values of columns t q + a and t q + b: the p_pred_samples bit for bit.
 *   both_k = p_a,k * p_b,k   P(y_a = 1, y_b = 1 | state) -- the outcomes are conditionally independent given
 *                            eta.  One fp64 multiplication, never contracted into a neighbouring add, so
 *                            the planes and the grids see the same numbers
 *   diff_k = p_a,k - p_b,k
 * Grids: both_predict and diff_predict, each 200 x C2 column-major per subset: the type-7 quantiles of the
 * draws above at the 200 levels, laid out as p_predict is.
 * Planes per subset: MK_N_PAIR_BASE + J, C2 x (6 + J) column-major, in the order
 *   both_mean, both_sd, diff_mean, diff_sd, corr, a_gt_b, joint_1..joint_J
 *   means    (sum_k v_k) / n, summed in time order from zero
 *   sds      the maps' Welford recurrence; NaN when n = 1
 *   corr     the posterior correlation of (p_a, p_b): beside the two marginal Welford pairs (m, M2) the
 *            co-moment C = C + (p_a - m_a,old) (p_b - m_b,new); corr = C / (sqrt(M2_a) sqrt(M2_b)), NaN when
 *            either M2 is 0 or n < 2
 *   a_gt_b   #{k : p_a,k > p_b,k} / n, strict
 *   joint_j  #{k : p_a,k > u_j and p_b,k > u_j} / n, strict ("both above 20 %"); the thresholds are checked as
 *            the maps' are: finite, J <= MK_MAP_MAXT
 * A non-finite draw or eta in either column makes every plane of the pair NaN.
 * The combined grids combined_both / combined_diff (200 x C2) are the K subsets' grids combined by
 * mk_combined.method (mean or median; the mean when comb is NULL).  Their planes are mk_map_grid's: of
 * combined_both with the thresholds, of combined_diff with the one threshold 0, whose exceedance column
 * P(diff > 0) is the combined counterpart of a_gt_b.  A combined corr and a combined joint_j do not exist:
 * the grids do not carry them. */
#define MK_N_PAIR_BASE 6  /* planes before joint_1..J */
typedef struct mk_pair_spec { int32_t n_thresholds; const double* thresholds; } mk_pair_spec;
typedef struct mk_pairs {             /* caller-allocated, any pointer may be NULL */
  double* both_predict;        /* [n_subsets] x (200 x C2) */
  double* diff_predict;        /* [n_subsets] x (200 x C2) */
  double* planes;              /* [n_subsets] x (C2 x (6 + J)) */
  double* combined_both;       /* 200 x C2 (node call only) */
  double* combined_diff;       /* 200 x C2 (node call only) */
} mk_pairs;
/* Ask the session for the pair outputs at its current test sites (NULL detaches and frees).  MK_E_ARG for
 * q = 1, no test sites, no x_test or no recorded samples, and for a bad threshold (as mk_session_set_maps),
 * all before any device is touched.  A tiled session takes its buffers here and only here: 3200 bytes of
 * grids and 8 (6 + J) bytes of planes per (subset, pair column); MK_E_NOMEM names the remedies.  While
 * attached, every tile replay of a tiled session also fills that tile's pair columns, from the same
 * replay and over its kept window.  mk_session_set_test_sites detaches.  Nothing is launched or allocated
 * for the pairs unless they were asked for. */
int mk_session_set_pairs(mk_session* s, const mk_pair_spec* spec);
/* After all iterations.  A fused session makes what is asked for from its kriging draws (all kept states)
 * now, in scratch held for the call.  A tiled session copies its buffers out: MK_E_ARG, naming the first
 * such tile, if some tile has not been replayed over the current kept window since the pairs were
 * attached.  combined_both / combined_diff are not written here. */
int mk_session_pairs(mk_session* s, mk_pairs* out);
/* mk_meta_fit_maps with the pair outputs (mk_meta_fit_maps is this call with two NULLs): every block
 * attaches the spec and writes its subsets' grids and planes at their global offsets into the caller's
 * arrays (into a host scratch when only a combined grid is asked for); the calling thread then combines the
 * host copies with mk_combine / mk_combine_median.  Nothing is added to the exchange; the host holds
 * K 200 C2 8 bytes per functional (0.27 GB at 56 subsets x 3 pairs x 1,000 sites). */
int mk_meta_fit_pairs(const mk_problem* prob, const mk_config* cfg, const int32_t* devices, int32_t n_devices,
                      mk_progress_fn progress, void* user, mk_outputs* out, mk_combined* comb, mk_diagnostics* diag,
                      mk_criteria* crit, const mk_validation* val, mk_scores* scores, const mk_map_spec* spec,
                      mk_maps* maps, const mk_pair_spec* pair_spec, mk_pairs* pairs);

/* ---- areal prediction: the prevalence of a region from joint kriging draws ----
 * The prevalence of a district is the (population-weighted) mean of p(y = 1) over the test sites inside it.
 * The per-site draws above are marginal across sites: averaging them gives the right mean and too small a
 * spread, because kriging errors at neighbouring sites are strongly correlated.  Here the draws of a region's
 * sites are joint, per kept state, and only their weighted mean -- one scalar per (state, region, outcome) --
 * leaves the replay.
 * A region spec partitions the session's current test sites, in their order, into G contiguous runs:
 * offsets[0 .. G] with offsets[0] = 0, offsets[G] = n_test, strictly increasing; m_g = offsets[g+1] -
 * offsets[g] <= MK_REGION_MAXM; one weight per test site (NULL: all 1), finite and >= 0 with a positive sum in
 * every region; up to MK_MAP_MAXT thresholds.  The host normalises the weights once, omega_i = weight_i / (the
 * sum of the region's weights, added in index order); the device only sees omega.
 * For subset s, kept state k of the window (iteration it), outcome h and region g with sites t_1 < .. < t_m
 * (global test-site indices):
 *   mean_i,h = X_h,t_i . z_h over rows < n_s                                  (k_pred_draw's mean)
 *   S_h      = R_h(g,g) - X_g' X_g, lower triangle, rows < n_s of X only; R_h(g,g) the model's own
 *              correlation (exponential or Matern, at the state's phi_h, nu_h) between the region's sites,
 *              unit diagonal
 *   L_h      = the Cholesky factor of S_h in site order; a pivot that is not > MK_REGION_PIVOT_TOL zeroes
 *              that column of L (the site is conditionally determined by the data and the sites before it)
 *              and flags the factor
 *   zeta_i,h = predict_normal(key_s, t_i q + h, it): the Philox word of the marginal draw of that site,
 *              outcome and state
 *   v_i,h    = mean_i,h + sum_{j <= i} L_h[i,j] zeta_j,h, j ascending
 *   w*_i,a   = sum_h v_i,h A[a,h]                                              (k_pred_draw's order)
 *   p_i,a    = pred_prob of column t_i q + a                                   (the p draws' expression)
 *   r_g,a    = sum_i omega_i p_i,a, i ascending: one draw of the regional prevalence
 * Region column c = g q + a; C3 = G q.  A region of one site reproduces that site's p_pred_samples (to the
 * summation order of its kriging variance); the first site of every region keeps its marginal law.  The
 * draws depend only on (seed, global subset index, test-site index): not on sharding or stream groups.
 * Outputs per subset:
 *   region_samples  C3 x kept column-major, like p_pred_samples
 *   region_predict  200 x C3: the type-7 quantiles of the draws (the p grids' kernel)
 *   planes          C3 x (2 + J): mean, sd, exc_1..J -- the maps' formulas on the draws, in time order, the
 *                   exceedance strict; a non-finite draw makes the column's planes NaN
 *   singular        int32 [C3]: the kept states of the window whose factor for (region g, outcome a) was
 *                   flagged, at column g q + a
 * The regions need a session created with predict_tile > 0 whose tile holds every test site: the joint
 * covariance is formed from X = W P^T, which the tiled replay has in HBM.  Two routes serve them.
 * MK_REGIONS_EXACT (the default): the exact tiled replay forms and factors S_h at every kept state whose phi_h
 * changed; while regions are attached on this route the phi-interpolated replay is not used, so the tile's
 * other outputs (grids, draws, maps, pairs, scores) are the exact replay's: they agree with the interpolated
 * ones to the documented 1e-8, not bit for bit.
 * MK_REGIONS_INTERP (mk_session_set_regions_route): the tile replay interpolates wherever it would without
 * regions (exponential models, MK_KRIG_CHEB's auto rule or its forcing, the checks passed).  S_h depends on
 * phi_h alone and is analytic in it like s(t; phi): its lower triangle is formed exactly at the replay's
 * Chebyshev nodes and check slots (the node-count rule's d_max then also covers the largest distance inside a
 * region), interpolated with the same barycentric weights (a node hit returns the node's value) at every
 * distinct phi_h of the window, and factored with the same pivot rule.  The interpolant's largest |difference|
 * from the exact S at the check slots joins the replay's own check: above MK_KRIG_CHEB_TOL the whole tile
 * runs exactly, as does a tile whose node, means or factor buffers do not fit in HBM.  The means are the
 * interpolated replay's m_k,h(t); the normals, the summation orders, the A mix, pred_prob, the weighted sum
 * and the flagged-factor count are those above.  The draws agree with the exact route's to about
 * cond(S_h) x the check, and the tile's other outputs are, bit for bit, those of the interpolated replay
 * without regions.  The kept window is processed in chunks of consecutive states (as many as a factor scratch
 * of 1 GiB holds; MK_REGIONS_CHUNK overrides); the results do not depend on the chunk length.
 * The fused (in-chain) route, the node call, regions above MK_REGION_MAXM sites or across tiles, a Matern
 * interpolation and a thinned replay are not covered. */
#define MK_REGION_MAXM 128          /* sites per region at most */
#define MK_REGION_PIVOT_TOL 1e-12   /* a pivot of S_h that is not above this zeroes its column */
#define MK_REGIONS_EXACT 0          /* routes of the areal prediction: the exact tiled replay */
#define MK_REGIONS_INTERP 1         /* the phi-interpolated replay wherever it would run without regions */
typedef struct mk_region_spec {
  int32_t n_regions;           /* G */
  const int32_t* offsets;      /* [G + 1] */
  const double* weights;       /* [n_test], or NULL: every site weighs 1 */
  int32_t n_thresholds;        /* J */
  const double* thresholds;
} mk_region_spec;
typedef struct mk_regions {           /* caller-allocated, any pointer may be NULL */
  double* region_predict;      /* [n_subsets] x (200 x C3) */
  double* planes;              /* [n_subsets] x (C3 x (2 + J)) */
  double* region_samples;      /* [n_subsets] x (C3 x kept) */
  int32_t* singular;           /* [n_subsets] x C3 */
  double* timing_ms;           /* [3]: the region launches' time since the attach -- covariance and factor
                                  (on the interpolated route the node covariances, the check and the
                                  interpolate-and-factor launches), draws, grids and planes (HIP events;
                                  kernel kind 19 holds their sum) */
} mk_regions;
/* Attach a region spec to the session's current test sites (NULL detaches and frees).  Everything is checked
 * on the host before any device is touched, each failure MK_E_ARG naming the offending index: bad offsets, a
 * region above MK_REGION_MAXM, a bad weight or threshold, two sites of one region at identical coordinates;
 * no test sites, no x_test or no recorded samples; a session that was not created with predict_tile > 0 (the
 * message names the remedy); more test sites than the session's tile (mk_session_predict_tile).  The session
 * takes its buffers here and only here: per (subset, outcome) sum_g m_g^2 doubles of factors, per subset C3
 * doubles per kept state, and the grids and planes; MK_E_NOMEM names the remedies.  While attached, every
 * tile replay also makes the regional draws, from the same replay and over its kept window.
 * mk_session_set_test_sites detaches.  Nothing is launched or allocated for the regions unless they were
 * attached. */
int mk_session_set_regions(mk_session* s, const mk_region_spec* spec);
/* The route of the attached regions (MK_REGIONS_EXACT or MK_REGIONS_INTERP; anything else, or no attached
 * spec, is MK_E_ARG).  Called after mk_session_set_regions: attaching or detaching a spec resets the route to
 * MK_REGIONS_EXACT.  Nothing is allocated here: the interpolated route takes its buffers inside a tile replay
 * and frees them before it returns. */
int mk_session_set_regions_route(mk_session* s, int32_t route);
/* asked: the route set; ran: the route the last tile replay took (MK_REGIONS_EXACT before any); check: that
 * replay's largest |interpolant - exact| over the entries of S_h at the check slots, 0 when the exact route
 * ran.  Any pointer may be NULL.  MK_E_ARG without an attached spec. */
int mk_session_regions_route(mk_session* s, int32_t* asked, int32_t* ran, double* check);
/* After all iterations: copies the buffers out.  MK_E_ARG if the tile has not been replayed over the current
 * kept window since the regions were attached. */
int mk_session_regions(mk_session* s, mk_regions* out);

/* ---- combine (MK.R:123-133): out = (grid_1 + ... + grid_K) / K, sequential order ---- */
int mk_combine(const double* grids, int32_t K, int64_t grid_len, double* out, int32_t device);

/* The sum only (no 1/K): one shard's term of the combine, or the rank-ordered sum of shard terms. */
int mk_combine_sum(const double* grids, int32_t K, int64_t grid_len, double* out, int32_t device);
/* Device-resident form for the multi-GPU combine (grids already in HBM, e.g. RCCL receive
 * buffers): d_out[e] = sum_k d_grids[k*grid_len + e] in k order, divided by K when mean != 0.
 * stream: a hipStream_t (NULL = the legacy default stream); returns after the kernel is queued. */
int mk_combine_device(const double* d_grids, int32_t K, int64_t grid_len, double* d_out, int32_t mean,
                      int32_t device, void* stream);

/* ---- combine extension (north star; not in the reference, which averages at MK.R:123-133):
 * per column, the Weiszfeld geometric median of the K subset quantile functions in the
 * Wasserstein-2 metric, started from the mean.  grids: K x (n_levels x n_cols) column-major;
 * out: n_levels x n_cols; iters (optional): [n_cols] iterations used.  n_levels <= 256. ---- */
int mk_combine_median(const double* grids, int32_t K, int32_t n_levels, int64_t n_cols, int32_t max_iter,
                      double tol, double* out, int32_t* iters, int32_t device);
/* Device-resident form (grids, out, iters in HBM; stream as in mk_combine_device). */
int mk_combine_median_device(const double* d_grids, int32_t K, int32_t n_levels, int64_t n_cols, int32_t max_iter,
                             double tol, double* d_out, int32_t* d_iters, int32_t device, void* stream);

/* ---- post-combine steps (MK.R:136-165) ---- */
typedef struct mk_summary {
  double* sample_par;    /* samplesize x P   SamplePar  (MK.R:145)                 */
  double* sample_w;      /* samplesize x C   Samplew    (MK.R:146)                 */
  double* p_sample;      /* samplesize x C   p.sample   (MK.R:156-161)             */
  double* w_quant;       /* 3 x C            w.quant    (MK.R:164)                 */
  double* param_quant;   /* 3 x P            param.quant (MK.R:165)                */
  double* p_quant;       /* 3 x C            quantiles of p.sample (extension)     */
  int32_t* index;        /* samplesize       sampleparIndex - 1 (MK.R:141)         */
} mk_summary;
/* result: 200 x P combined parameter grid (betas first, MK.R:159); result2: 200 x C combined
 * w.predict grid; x_test: C x p (p <= P).  Any output pointer may be NULL. */
int mk_posterior_summary(const double* result, int32_t P, const double* result2, int64_t C,
                         const double* x_test, int32_t p, int32_t samplesize, uint64_t seed,
                         mk_summary* out, int32_t device);
/* As mk_posterior_summary, plus: index (optional, [samplesize], 1-based) is sampleparIndex drawn
 * by the caller -- the R glue passes R's own sample(seq(1, length(Xout), 1), samplesize,
 * replace=TRUE) (MK.R:141), so the draws follow R's RNG stream; NULL draws it from Philox(seed).
 * link: MK_LINK_LOGIT (MK.R:160) or MK_LINK_PROBIT for p.sample. */
int mk_posterior_summary_ex(const double* result, int32_t P, const double* result2, int64_t C,
                            const double* x_test, int32_t p, int32_t samplesize, uint64_t seed,
                            const int32_t* index, int32_t link, mk_summary* out, int32_t device);

/* ---- glm start values (MK.R:53-55), once on the full data: binomial-logit IRLS with
 * glm.fit's rules (mustart init, |dev - devold|/(|dev| + 0.1) < epsilon, maxit).
 * y: counts, weights: trials (n each), x: n x p column-major (p <= 8).
 * coef: [p]; vcov: p x p (dispersion 1); iters (optional). ---- */
int mk_glm_binomial(const double* y, const double* weights, const double* x, int64_t n, int32_t p,
                    double epsilon, int32_t maxit, double* coef, double* vcov, int32_t* iters,
                    int32_t device);
/* binomial(link = "probit") too: R's make.link("probit") (eta clamped to +-qnorm(eps) in linkinv,
 * mu.eta = max(dnorm(eta), eps), linkfun = qnorm). link = MK_LINK_LOGIT is mk_glm_binomial. */
int mk_glm_binomial_link(const double* y, const double* weights, const double* x, int64_t n, int32_t p,
                         int32_t link, double epsilon, int32_t maxit, double* coef, double* vcov,
                         int32_t* iters, int32_t device);

/* ---- empirical variogram: all pairs of n sites, before the fit (the phi prior) and after it (misfit) ----
 * The reference chooses phi's start and prior by hand (MK.R:60-63: an effective range of 0.5 on the unit
 * square, Unif(3/0.75, 3/0.25)); the variogram of the start-value glm's residuals is what such a choice is
 * read from, and the variogram of held-out residuals is what is left of spatial structure after a fit.  For
 * q >= 2 the cross-variograms are the empirical counterpart of K = A A'.  Every pair is visited: nothing
 * is subsampled.
 * coords is n x 2 column-major, z location-major (site i, outcome a at i q + a).  The T = q (q + 1) / 2
 * outcome pairs (a >= b) come in the lower-triangle column-major order of A and K: (0,0), (1,0), ..,
 * (q-1,0), (1,1), ..; the diagonal entries are the direct semivariograms, the others the cross-variograms.
 *   s = n_bins / max_dist, divided once on the host
 *   for each unordered pair i < j:  d = sqrt(dx dx + dy dy) with dx = x_i - x_j, dy = y_i - y_j (dist2d's
 *     expression, no contraction), k = floor(d s); the pair is counted iff k < n_bins, so the bins are
 *     half-open, [k/s, (k+1)/s); coincident sites (d = 0) fall in bin 0; a site is never paired with itself
 *     and each unordered pair is counted once
 *   count[k]    = N_k
 *   dist[k]     = (sum of d) / N_k
 *   gamma_ab[k] = (sum of (z_a(i) - z_a(j)) (z_b(i) - z_b(j))) / (2 N_k), Matheron's estimator
 * An empty bin has count 0 and NaN in dist and gamma.  The sums are fp64 in a fixed order -- a lane's pairs
 * in (tile, column) order, the lanes of a workgroup in lane order, the workgroups in index order, the tiles
 * dealt to a number of workgroups fixed by n alone -- and the counts are integers, so two calls with the
 * same arguments return the same bytes on any placement; there are no floating-point atomics.
 * MK_E_ARG, before any device is touched and with the message in mk_last_error: a null pointer, n < 2 (or
 * above 2^24), q outside 1 .. MK_VG_MAXQ, n_bins outside 1 .. MK_VG_MAXBINS, max_dist not finite or not > 0,
 * a coordinate or z value that is not finite (the message names the first such index). */
#define MK_VG_MAXBINS 64
#define MK_VG_MAXQ 4
#define MK_VG_EDGE 256    /* tile edge of the pair kernel (mk_variogram_tile_edge) */
typedef struct mk_variogram {
  int64_t* count;   /* [n_bins]      pairs in the bin                                   */
  double*  dist;    /* [n_bins]      mean distance of the bin's pairs, NaN if empty     */
  double*  gamma;   /* [T][n_bins]   T = q(q+1)/2, NaN if empty                         */
  double   ms;      /* out: device time of the launches, by one event pair             */
} mk_variogram;
int mk_variogram_compute(const double* coords, int64_t n, const double* z, int32_t q, int32_t n_bins,
                         double max_dist, mk_variogram* out, int32_t device);
int32_t mk_variogram_tile_edge(void);

/* ---- partition (MK.R:15-41) with R's own RNG stream, host side ----
 * After `set.seed(seed)` under R >= 3.6.0 defaults (Mersenne-Twister, Rejection sampling),
 * the reference's loop `index.part[[i]] <- sample(a, n.part[i]); a <- setdiff(a, ...)`.
 * n_part: [n_core] out (MK.R:17-18); index_out: [n] out, subset i's 1-based indices at offset
 * n_part[0] + ... + n_part[i-1], in R's draw order.  Replaces nothing on the R side (R keeps
 * its own partition); it lets a non-R host fit exactly the subsets an R session fits. */
int mk_partition_r(int32_t n, int32_t n_core, int32_t seed, int32_t* n_part, int32_t* index_out);
/* sample.int(n, size) (without replacement, 1-based) right after set.seed(seed). */
int mk_r_sample(int32_t seed, int32_t n, int32_t size, int32_t* out);
/* sample.int(n, size, replace = TRUE) right after set.seed(seed): MK.R:141's sampleparIndex
 * (n = length(Xout) = 996) as an R session that set the seed just before would draw it. */
int mk_r_sample_replace(int32_t seed, int32_t n, int32_t size, int32_t* out);

/* ---- exposed kernels for parity tests ---- */
/* R_k = correlation(coords_k) (n x n column-major) for S point sets of n sites, computed by
 * the sampler's own candidate kernel (k_cov_candidate: exponential, or Matern with the binned
 * Temme/CF2 Bessel-K evaluation) -- the covariance-assembly arithmetic the chains use. */
int mk_correlation_batched(const double* coords, int32_t S, int32_t n, const double* phi, const double* nu,
                           int32_t cov_model, double* R_out, int32_t device);
/* The same, on both routes and both Matern table configurations.  R_out ([S][n][n] column-major, or NULL):
 * the candidate route, as above.  PT_out ([S][n][n_test], row k the observed site, or NULL): the kriging
 * route, P^T = correlation(coords_k, coords_test_k) by k_pred_PT_matern (Matern) or k_pred_PT
 * (exponential); coords_test: [S][2][n_test], every point set with its own test sites (x then y, as
 * coords: [S][2][n]).  stored_tables (Matern): 1 the configuration of a session -- the Chebyshev tables
 * cover [0.5, phi x span], span the sites' bounding-box diagonal (R) or the bound on the site-to-test-site
 * distances (P^T) by the expressions the sessions use, stored by k_matern_table / k_matern_table_list and
 * loaded by the tile workgroups; 0 the kernels build unbounded tables themselves.
 * mk_correlation_batched is this call with stored_tables = 0 and R only. */
int mk_correlation_cross_batched(const double* coords, int32_t S, int32_t n, const double* coords_test,
                                 int32_t n_test, const double* phi, const double* nu, int32_t cov_model,
                                 int32_t stored_tables, double* R_out, double* PT_out, int32_t device);
/* Cholesky (lower) + log-determinant (+ optional inverse) of S SPD n x n matrices.  MK_E_ARG when a
 * factorisation meets a pivot that is not > 0 (negative, zero or NaN); mk_last_error then reads
 * "matrix <i> is not positive definite", i the lowest index of such a matrix. */
int mk_cholesky_batched(const double* A, int32_t S, int32_t n, double* L_out, double* logdet_out,
                        double* inv_out, int32_t device);

/* The block -> job map of the inverse levels' launches (k_inv_level), evaluated on the host by the
 * kernel's own code; no GPU work.  One launch: level sz (tiles per block: 1, 2, 4, ... < nt), phase 0
 * or 1, `count` listed factors of nt 128-tiles on a grid sized for max_entries, sub = 1, 4 or 16
 * sub-tiles per 128-tile.  map 1: the cut over the XCDs by work, longest K ranges first (MK_INV_MAP's
 * default); 0: the equal-count cut.  Returns the launch's grid; when out is not NULL, block b < min(grid,
 * cap) gets out[5 b ..] = entry, pair, tile row i, tile column j, sub-tile, or five times -1 when it
 * has no job. */
int mk_inv_map_jobs(int32_t map, int32_t count, int32_t max_entries, int32_t nt, int32_t sz, int32_t phase,
                    int32_t sub, int32_t* out, int32_t cap);

/* Hardware queues the process's HIP runtime was started with (GPU_MAX_HW_QUEUES when HIP first
 * initialised; HIP's default is 4).  The lookahead schedule adds a kriging stream and a CU-masked
 * main stream only when there are >= 8 (streams beyond the queue count share queues and serialise,
 * DESIGN.md 4.2).  A host that knows HIP started before its own setting took effect (e.g. torch
 * first) passes the real count; n < 0 restores the default: GPU_MAX_HW_QUEUES from the environment. */
int mk_set_hw_queues(int32_t n);

/* Whether this process's HIP runtime has already started (the process holds /dev/kfd open), without
 * starting it: a host that sets GPU_MAX_HW_QUEUES first checks whether the setting can still take
 * effect (the R package's .onLoad; libmk itself has not touched HIP when this is called). */
int mk_hip_initialized(void);

/* Drains and destroys libmk's idle pooled HIP streams (CU-masked and priority queues included) while
 * the runtime is alive; streams of sessions still open are destroyed with them.  libmk registers it
 * with atexit after its first stream; hosts call it from their own exit hooks too (Python atexit,
 * R .onUnload).  Idempotent; libmk stays usable afterwards (new streams are no longer pooled). */
void mk_shutdown(void);

/* Stall watchdog: when seconds > 0 every launch is followed by a progress-word store into pinned host
 * memory, and a C-ABI call still running after `seconds` prints (stderr, and MK_WATCHDOG_LOG=<path>
 * if set) every stream with work outstanding and the kernel it is on.  0 = off (default; the
 * environment variable MK_WATCHDOG=<seconds> sets it at load). */
int mk_set_watchdog(int32_t seconds);

/* ---- sessions from a recorded chain ----
 * Everything the kriging replay and the result sinks read of a fit is what a fit reports: samples
 * (beta | lower-tri K | phi | nu per iteration) and w_samples (w = A u).  mk_session_import_chain rebuilds the
 * kept-state record from them -- per kept state A = chol(K) with a positive diagonal, theta (A's lower triangle
 * with log diagonal | logit phi | logit nu), u_i = A^-1 w_i per site and z_h = L_h^-1 u_h with L_h the Cholesky
 * factor of R(phi_h, nu_h) -- so a chain saved by an earlier process, or made elsewhere (the CPU oracle, another
 * machine), is replayed at any test sites and through every sink without running it again.
 *
 * Valid on a session as mk_session_create left it (no iteration run, nothing imported, not poisoned) that keeps
 * chain states: predict_tile > 0, and no test sites or more test sites than the tile.  The checks run on the
 * host before the device is touched, and each refusal (MK_E_ARG) names the global subset index, the 1-based
 * iteration and the column or row: a null pointer, n_w out of range, a value that is not finite, a kept phi (nu
 * under Matern) that is not strictly inside its prior, a kept K that is not positive definite.  A kept state
 * whose R(phi_h, nu_h) meets a pivot that is not > 0 on the device is MK_E_ARG naming subset, outcome and
 * iteration, and the session is left as created.  Out of memory is MK_E_NOMEM; every buffer of the import other
 * than the record is freed before the call returns.
 *
 * Afterwards the session is one whose chain is complete: mk_session_iteration returns n.samples, and the
 * outputs, grids, tile grids, test sites, covariates, kept windows and every sink work as after mk_session_run
 * (the criteria by their replay route, which needs record_w; in-chain criteria are refused).  samples and, with
 * record_w, w_samples come back from mk_session_outputs as the bytes that went in; mk_session_notpd_counts
 * returns zeros.  The imported z is computed from w, the live chain's is updated incrementally: the two sessions
 * agree to rounding.  mk_session_run, mk_session_chain_state and mk_session_set_lookahead on an imported
 * session are MK_E_ARG, and so is asking for acceptance when none was imported. */
typedef struct mk_chain {
  const double* samples;     /* [n_subsets] x (n_samples x P) column-major, the layout of mk_outputs.samples   */
  const double* w_samples;   /* [n_subsets] x ((n_s q) x n_w) column-major: the LAST n_w iterations' w           */
  int32_t n_w;               /* kept <= n_w <= n_samples; must be n_samples when cfg.record_w                    */
  const double* acceptance;  /* optional, the layout of mk_outputs.acceptance; NULL: none recorded               */
} mk_chain;
int mk_session_import_chain(mk_session* s, const mk_chain* c);
int32_t mk_session_imported(const mk_session* s);          /* 1 after a successful import */
/* What the import cost: the (subset, outcome) factorisations it made (one per run of consecutive kept states
 * with the same (phi_h, nu_h), summed over the pairs), the milliseconds of the factor refreshes (candidate,
 * Cholesky, inverse) and of the z = W u launches (k_import_z), by device events.  Any pointer may be NULL;
 * MK_E_ARG unless the session was imported. */
int mk_session_import_stats(const mk_session* s, int64_t* factorisations, double* ms_factor, double* ms_z);

/* ---- checkpoints: continue a chain in a later process ----
 * The chain is deterministic given its state (the Philox streams are keyed by seed, global subset and iteration
 * and carry none), so a chain stopped after any iteration, written out, read by a fresh process and continued
 * reports the bytes of the chain that never stopped.  mk_session_checkpoint copies that state to the host,
 * mk_session_restore puts it into a session made over the same data and configuration.
 *
 * The state is MK_CKPT_NFIELDS fields of 8-byte words (doubles but for notpd, int64), each [count] x words[f],
 * subset-major, in the session's padded device layout (n_pad = the largest subset + 1 rounded up to 128,
 * Np = n_pad q, nmh = p + n_theta + Np), as raw bytes:
 *    0 beta [p]           1 theta [n_theta]     2 w [Np]             3 eta [Np] (padding zeroed)
 *    4 tune [nmh]         5 acc [nmh]           6 u [q n_pad]        7 z [q n_pad]
 *    8 Z [q q n_pad]      9 logdetR [q]        10 quad [q]          11 A_full [q q]
 *   12 Ainv [q q]        13 notpd [q] int64
 *   14 crit_acc [6 Np]   15 crit_part [k nb]   16 crit_sbeta [p]    in-chain criteria (else 0 words; 14 and
 *                                                                   16 once a kept iteration ran; padding zeroed)
 *   17 samples [it P]    18 w_samples [it Np] (record_w)            19 acc_hist [it / batch.length][P + 1]
 *   20 kz [k q n_pad]    21 kth [k n_theta]    22 kA [k q q]        a tiled session's kept-state record
 *   23 w_pred [k q n_test]                                          a fused session's kriging draws
 * with it the iterations done and k = max(0, it - burn_in + 1) the kept ones: only the rows that exist are
 * moved.  mk_session_checkpoint_layout writes the words per subset of every field at `iteration` (-1: the
 * iterations done so far) into words[MK_CKPT_NFIELDS]; the caller allocates count x words[f] x 8 bytes per field
 * and count q MK_CKPT_NDIGEST uint64 for the digests.
 *
 * The factors (L, Winv, W, QB of the accepted slots) and a fused session's kriging buffers are not part of the
 * state: the restore re-derives them from the restored theta with the session's own candidate, Cholesky and
 * inverse kernels, then refreshes the kriging buffers of every pair.  The carried schedule state (queued
 * lookahead candidates, the early assembly, pending table draws) is dropped; the schedules re-prime themselves.
 * So that "re-derived, hence the same bits" is checked and not assumed, a checkpoint carries per (subset,
 * outcome) pair a 64-bit digest of each factor buffer over the region later iterations read -- columns and rows
 * below n_s; the bordered row and scratch are outside -- and the restore compares the digests of what it
 * re-derived: a mismatch is MK_E_HIP naming the pair and the buffer, and the session is left poisoned.
 *
 * The digest of words x_0 .. x_{m-1} (a double's bit pattern) is
 *    D = sum_i mix(x_i + (i + 1) * 0x9E3779B97F4A7C15) mod 2^64,
 * mix the splitmix64 finaliser (x ^= x >> 30, x *= 0xBF58476D1CE4E5B9, x ^= x >> 27, x *= 0x94D049BB133111EB,
 * x ^= x >> 31).  The regions' enumeration: MK_DIGEST_L and MK_DIGEST_W the lower triangle of the leading n_s x
 * n_s block, column-major (column c: rows c .. n_s - 1); MK_DIGEST_WINV per 128-tile k, m_k = min(128, n_s -
 * 128 k) > 0, the lower triangle of its leading m_k x m_k block, column-major, tile after tile; MK_DIGEST_QB per
 * tile its two diagonal 64 x 64 quadrants (the sweeps read, and the library computes, no other part of a tile),
 * of each the leading block below n_s, column-major, quadrant 0 then 1 (0 for a session whose sweep keeps no QB).
 *
 * mk_session_checkpoint: subsets [first, first + count); MK_E_ARG on an imported session (it holds no sampler
 * state; the fit file is the tool there) or a poisoned one.  mk_session_restore: the session must be as
 * mk_session_create left it (no iteration run, nothing imported, not poisoned); `words` are the caller's sizes
 * per subset of every field, and all the session's subsets are restored -- a subset range of a checkpoint goes
 * into a session made over those subsets with subset_base moved by `first`, which must have the same n_pad.
 * Refused on the host before any device work (MK_E_ARG, naming subset, field, expected and given size):
 * iteration outside 0 .. n.samples, a size that differs from the layout, a missing field, a non-finite theta,
 * tune or w, an accept count that is negative or not integral.  A restored theta whose R(phi, nu) meets a pivot
 * that is not > 0 is MK_E_ARG naming the pair, and the session is left as created.  Afterwards
 * mk_session_iteration returns `iteration`, mk_session_run continues the chain, and once iteration = n.samples
 * every output and sink behaves as on the session that ran.  The state does not depend on n_streams or on how
 * the session that wrote it was launched, with one exception: the lookahead and the sequential schedule make the
 * same decisions but round z differently (a forward solve against the bordered factor row; mk_session_set_lookahead),
 * so a chain written under one and continued under the other would agree with neither to the last bit.  The
 * schedule is therefore part of what a started chain is ("before the first mk_session_run only" above): the
 * checkpoint records it, and a restore at 0 < iteration < n.samples puts the session on the schedule that wrote
 * the state, whatever it was made with (mk_session_lookahead reports it; at iteration 0 and n.samples the
 * session keeps its own).  A session of several stream groups cannot run the lookahead schedule: a state
 * written mid-chain under it is MK_E_ARG there, by name -- a different chain is never continued.
 * mk_session_digest: the digests of the session's factors now, [n_subsets q][MK_CKPT_NDIGEST].
 * mk_digest: the digest of n_words caller-given host words on `device` (uploaded in chunks; MK_DIGEST_CHUNK
 * words per chunk, default 2^25), by the kernel the sessions use (k_state_digest).
 * Kernel-stat kind 21: the digest launches -- launches and ms, always timed, 0 launches unless a checkpoint,
 * restore or digest call is made. */
#define MK_CKPT_NFIELDS 24
#define MK_CKPT_NDIGEST 4
#define MK_DIGEST_L 0
#define MK_DIGEST_WINV 1
#define MK_DIGEST_W 2
#define MK_DIGEST_QB 3
typedef struct mk_checkpoint {
  void* field[MK_CKPT_NFIELDS]; /* field f: [count] x words[f] 8-byte words; NULL only where words[f] = 0 */
  uint64_t* digests;            /* [count q][MK_CKPT_NDIGEST]                                             */
  int32_t lookahead;            /* the schedule that wrote the state: mk_session_lookahead (set by checkpoint) */
} mk_checkpoint;
int mk_session_checkpoint_layout(const mk_session* s, int32_t iteration, int64_t* words);
int mk_session_checkpoint(mk_session* s, int32_t first, int32_t count, mk_checkpoint* out);
int mk_session_restore(mk_session* s, int32_t iteration, const int64_t* words, const mk_checkpoint* in);
int mk_session_digest(mk_session* s, uint64_t* out);
int mk_digest(const void* words, int64_t n_words, int32_t device, uint64_t* out);
/* What the last restore cost, by device events: the re-derivation (candidates, Cholesky, inverse, kriging
 * refresh), the digests, and the uploads (host clock).  MK_E_ARG unless the session was restored. */
int mk_session_restore_stats(const mk_session* s, double* ms_derive, double* ms_digest, double* ms_upload);

const char* mk_last_error(void);
int mk_device_count(void);
/* Free and total HBM of a device (hipMemGetInfo), e.g. to size shards or check for leaks. */
int mk_device_memory(int32_t device, int64_t* free_bytes, int64_t* total_bytes);

#ifdef __cplusplus
}
#endif
#endif /* MK_H */
