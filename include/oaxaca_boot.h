/*
 * oaxaca_boot.h -- C ABI of the MI355X bootstrap-inference engine for Oaxaca-Blinder.
 *
 * Drop-in boundary for the bootstrap driver of `OaxacaBuilder::run()` in
 * dot-comma-hyphen/oaxaca-blinder-rs (paths below are relative to oaxaca_blinder/src/).
 * Plain C types only: no torch, no HIP types (a hipStream_t is passed as void*).
 * INTEGRATION.md shows the Rust `extern "C"` block and the edited run() a maintainer adds.
 *
 * Layering:
 *   1. hot path   ob_panel_* / ob_point_estimate / ob_boot_run*   replaces builder.rs:808-847
 *   2. inference  ob_bootstrap_stats / ob_rif                      inference.rs:4-34, math/rif.rs:14-88
 *   3. builder    ob_builder_* / ob_prepared_* / ob_results_*      OaxacaBuilder (builder.rs:37-983)
 *                 for hosts without a Rust toolchain (the Python front end binds these).
 *
 * All calls are blocking unless named *_device. One ob_ctx per thread, or external locking.
 * Errors: return code (OB_OK = 0) + thread-local message from ob_last_error().
 */
#ifndef OAXACA_BOOT_H
#define OAXACA_BOOT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- errors: one code per OaxacaError variant (error.rs:6-19) plus engine codes ---------- */
#define OB_OK 0
#define OB_E_POLARS 1        /* OaxacaError::PolarsError: dtype / frame errors */
#define OB_E_COLUMN 2        /* OaxacaError::ColumnNotFound */
#define OB_E_GROUP 3         /* OaxacaError::InvalidGroupVariable (also negative weights, ols.rs:60-66) */
#define OB_E_LINALG 4        /* OaxacaError::NalgebraError (Cholesky failure, ols.rs:107-111) */
#define OB_E_DIAG 5          /* OaxacaError::DiagnosticError */
#define OB_E_INSUFFICIENT 6  /* OaxacaError::InsufficientData (n <= k, ols.rs:98-105) */
#define OB_E_HIP 7           /* HIP runtime failure / no GPU: the engine never falls back to the CPU */
#define OB_E_INVALID 8       /* bad argument */
#define OB_E_UNSUPPORTED 9   /* outside the engine's scope (Heckman selection, sizes over limits) */
#define OB_E_OVERFLOW 10     /* a resample count exceeded the Gram's range in one row: 127 on the default i8
                                path (probability ~1e-215 per row and replicate), 255 on the f64 path */
#define OB_E_RCCL 11         /* RCCL missing or a collective failed (multi-GPU entry points) */
#define OB_E_CONVERGENCE 12  /* AkmError::ConvergenceFailed (akm.rs:11): an AKM loop ran out of iterations, or
                                the OLS of the demeaned controls is singular */

const char* ob_last_error(void);
const char* ob_version(void);

/* ---- ReferenceCoefficients (decomposition.rs:5-20) ---------------------------------------- */
#define OB_REF_GROUP_A 0
#define OB_REF_GROUP_B 1
#define OB_REF_POOLED 2   /* == Neumark */
#define OB_REF_WEIGHTED 3 /* == Cotton  */
#define OB_REF_COTTON 4
#define OB_REF_NEUMARK 5

/* ---- per-replicate row layout (Kd = K + n_base, K = p + 1 incl. the intercept) ------------ */
#define OB_ROW_EXPLAINED 0
#define OB_ROW_UNEXPLAINED 1
#define OB_ROW_ENDOWMENTS 2
#define OB_ROW_COEFFICIENTS 3
#define OB_ROW_INTERACTION 4
#define OB_ROW_TOTAL_GAP 5
#define OB_ROW_DETAILED 6 /* [6, 6+Kd) explained, [6+Kd, 6+2Kd) unexplained, then
                             beta_a[K], beta_b[K], xa_mean[K], xb_mean[K], beta_star[K] */

/* ---- device context ---------------------------------------------------------------------- */
typedef struct ob_ctx ob_ctx;
int ob_device_count(int* n);
int ob_ctx_create(int device, ob_ctx** out);
void ob_ctx_destroy(ob_ctx* ctx);

/* ---- hot path: the two groups' design, resident in HBM -------------------------------------
 * Replaces the per-replicate polars resample + prepare_data + OlsEstimator of builder.rs:816-839.
 * The caller builds X as in prepare_data (builder.rs:294-378) WITHOUT the intercept column:
 * column-major n x p, predictors then dummy columns (builder.rs:325-327). */
typedef struct {
  int64_t n;       /* rows (df_a.height() / df_b.height()) */
  const double* x; /* column-major, ldx >= n */
  int64_t ldx;
  const double* y; /* outcome */
  const double* w; /* weights or NULL */
} ob_group_desc;

typedef struct {
  int32_t p;        /* predictor columns (numeric + dummies); K = p + 1 */
  int32_t n_num;    /* numeric predictors: the pooled group indicator is inserted at 1 + n_num
                       (builder.rs:560-564 -> prepare_data extra_predictors) */
  int32_t weighted; /* 1 if .weights() was set */
  ob_group_desc a;  /* advantaged group A */
  ob_group_desc b;  /* reference group B */
  /* categorical normalization (estimation.rs:76-91, normalization.rs:5-51, builder.rs:634-674);
     n_norm = 0 disables it. Column indices count the intercept as column 0. */
  int32_t n_norm;
  const int32_t* norm_start;   /* n_norm + 1 offsets into norm_idx */
  const int32_t* norm_idx;     /* columns named "{var}_*" (normalization.rs:11-16) */
  const int32_t* norm_m;       /* category_counts[var], or -1 for a non-categorical var
                                  (then matches + 1, normalization.rs:28-31) */
  const int32_t* pooled_start; /* the same on the pooled predictor list (indicator inserted) */
  const int32_t* pooled_idx;
  const int32_t* has_base;     /* 1 if var has a base category (adds a detailed term) */
  /* outcomes (RIF multi-tau): 0 or 1 = one outcome; n_y > 1: each group's
     y is an n x n_y column-major block with leading dimension ldx, and every replicate yields
     n_y rows (one per outcome) from one Gram pass. */
  int32_t n_y;
  /* Heckman two-step (builder .heckman_selection; estimation.rs:114-260, heckman.rs:38-108):
     heckman = 1 runs a probit of s on [1, z] (math/probit.rs:25-170) and the outcome OLS on the
     rows with s = 1 augmented by the inverse Mills ratio. z: n x n_zsel column-major with
     leading dimension ldx (intercept implicit, n_zsel <= OB_HECKMAN_MAX_ZSEL = 31, else
     OB_E_UNSUPPORTED; up to 7 run register-resident kernels, more the f64 MFMA kernels of
     csrc/ob_heckman.hip); s: the 0/1 selection outcome.
     With heckman = 1 the group w (if weighted) only feeds the total gap and the Cotton weights
     (the Heckman OLS is unweighted), n_norm must be 0, n_y 1, and rows carry K' = K + 1
     coefficients (IMR last) then 1 + n_zsel selection components (OB_ROW_* with K'). */
  int32_t heckman;
  int32_t n_zsel;
  const double* za;
  const double* zb;
  const double* sa;
  const double* sb;
} ob_panel_desc;

typedef struct ob_panel ob_panel;

/* Copies the design into HBM (the caller keeps ownership of its buffers). Fails with
   OB_E_GROUP on negative weights (ols.rs:60-66) and OB_E_HIP without a GPU. */
int ob_panel_create(ob_ctx* ctx, const ob_panel_desc* desc, ob_panel** out);
void ob_panel_destroy(ob_panel* panel);
int ob_panel_row_len(const ob_panel* panel);
int ob_panel_k(const ob_panel* panel);
int ob_panel_n_base(const ob_panel* panel);
int ob_panel_n_y(const ob_panel* panel);

/* Point estimate: run_single_pass on the unresampled data (builder.rs:810-811).
   resid_b (n_b entries, may be NULL) receives y_B - X_B beta_B (OaxacaResults::residuals).
   With n_y outcomes: row holds n_y x row_len, resid_b n_y x n_b (outcome-major). */
int ob_point_estimate(ob_panel* panel, int ref_mode, double* row, double* resid_b);

/* Bootstrap replicates [first_rep, first_rep + n_reps) of the OBRS-3 stream keyed by seed.
   rows: n_reps x ob_panel_row_len(); ok[r] = 0 marks a replicate the reference would drop
   (filter_map + .ok(), builder.rs:816-839): Cholesky failure or zero total weight. Results are
   a pure function of (seed, replicate id): identical on 1 or 8 GPUs. With n_y outcomes rows
   holds n_y x n_reps x row_len and ok n_y x n_reps (outcome-major blocks); each outcome's block
   is bitwise the rows a one-outcome panel of that y gives. */
int ob_boot_run(ob_panel* panel, uint64_t seed, uint64_t first_rep, uint64_t n_reps, int ref_mode,
                double* rows, uint8_t* ok);
/* Same, rows/ok in device memory, enqueued on hip_stream (hipStream_t; NULL = engine stream).
   Returns after enqueueing; synchronize the stream before reading. */
int ob_boot_run_device(ob_panel* panel, uint64_t seed, uint64_t first_rep, uint64_t n_reps,
                       int ref_mode, double* d_rows, uint8_t* d_ok, void* hip_stream);

/* HIP-event timings of the last boot run (ms summed over its launches; 0 if not run). */
typedef struct {
  double level1_ms; /* level-1 tile counts */
  double gram_ms;   /* X^T diag(c w) X MFMA kernel over the count images (the dominant kernel) */
  double reduce_ms;
  double solve_ms;  /* Cholesky solves + OB algebra */
  int32_t gram_launches;
  int32_t chunks;
  int32_t blocks;
  double counts_ms; /* level-2 count images (ob_count_kernel) */
  double heckman_ms; /* Heckman panels: probit iterations + IMR sums + two-step solve (in solve_ms too) */
  int32_t probit_iterations; /* Heckman panels: probit iterations of the last segment */
  double mm_assemble_ms;     /* ob_mm_run: mm_assemble kernel time (HIP events), summed */
  double mm_fit_rows;        /* ob_mm_run: live (fit, row) pairs those launches processed */
  int32_t mm_iterations;     /* ob_mm_run: most IPM iterations of a batch */
  double mm_ms;              /* ob_mm_run: whole call, host clock */
  double gather_ms;          /* sharded runs: the RCCL all-gather of the per-replicate rows (HIP events) */
  int32_t gram_path;         /* last boot run: 1 = f64 MFMA Gram, 2 = exact integer-sliced i8 MFMA Gram */
  double probit_ms;          /* Heckman panels: ob_probit_kernel time (HIP events), summed over iterations */
  int32_t probit_launches;   /* Heckman panels: ob_probit_kernel launches in those ms */
  double heck_sums_ms;       /* Heckman panels: ob_heck_sums_kernel (IMR sums) time */
  int32_t mm_reduced;        /* ob_mm_run: 1 if the row reduction ran (subsample, bands, reduced LPs) */
  int64_t mm_retried;        /* ob_mm_run: fits the reduction solved again on all rows (phase 3) */
  double prep_ms;            /* i8 Gram: building the panel's digit images + exception rows (HIP events;
                                nonzero only on the boot run that built them, the first of a panel) */
  int32_t oz_exceptions;     /* i8 Gram: exception rows, summed in f64 beside the integer Gram */
  int32_t oz_bits;           /* i8 Gram: a row is an exception when some |v_c| >= 2^oz_bits x its chunk's
                                scale for column c (geometric mean over nonzero rows), or not finite */
  int32_t oz_tiles6;         /* i8 Gram: (chunk, 32-pair column tile) blocks that run 6 of the 7 digit
                                slices (pairs of narrow magnitude range) */
  int32_t oz_tiles;          /* i8 Gram: all (chunk, column tile) blocks */
  int32_t oz_wide;           /* i8 Gram, last launch: 1 = the wide-tile kernel (4 waves, 256 replicates x 64
                                pairs per block), 2 = the wide tile with each chunk split over two blocks,
                                0 = the 8-wave kernel (32 pairs); option gram_tile */
} ob_timing;
int ob_panel_last_timing(const ob_panel* panel, ob_timing* out);
/* Synchronize the stream used by the last *_device call and collect its timings. */
int ob_panel_sync(ob_panel* panel);

/* ---- multi-GPU: replicates sharded over GPUs, one RCCL all-gather ----------
 * Replaces the Rayon into_par_iter of builder.rs:816-839 across devices. Replicates are
 * independent and a replicate's row is a pure function of (seed, replicate id), so the rows are
 * bitwise the same on 1, 2, 4 or 8 GPUs. Shard of rank r of W over [first_rep, first_rep + n):
 * per = ceil(n / W) replicates starting at first_rep + r * per (the last shard may be short or
 * empty). The per-replicate rows of every rank are then all-gathered over RCCL (xGMI), so every
 * rank ends with all n rows in replicate order; the caller aggregates them (ob_aggregate /
 * ob_prepared_finish) on one rank.
 *
 * One process per GPU (the torchrun / MPI shape): rank 0 calls ob_get_unique_id, sends the 128
 * bytes to every rank out of band, and each rank calls ob_ctx_create_rank with its GPU. Panels
 * created in a rank context run sharded through ob_boot_run_sharded[_device]. A plain ob_ctx acts
 * as rank 0 of 1 (no collective). */
typedef struct {
  char internal[128]; /* ncclUniqueId */
} ob_unique_id;
int ob_get_unique_id(ob_unique_id* id);
int ob_ctx_create_rank(int device, int rank, int world, const ob_unique_id* id, ob_ctx** out);
int ob_ctx_rank(const ob_ctx* ctx, int* rank, int* world);
/* This rank's shard + the all-gather; rows/ok (host) receive all n_reps rows on every rank
   (n_y outcome-major blocks as in ob_boot_run). Collective: every rank of the context calls it
   with the same seed, first_rep, n_reps and ref_mode. */
int ob_boot_run_sharded(ob_panel* panel, uint64_t seed, uint64_t first_rep, uint64_t n_reps, int ref_mode,
                        double* rows, uint8_t* ok);
/* Same into device buffers (n_reps x row_len doubles, n_reps bytes; x n_y) enqueued on hip_stream
   (NULL = engine stream); ob_panel_sync waits and fills ob_timing.gather_ms. */
int ob_boot_run_sharded_device(ob_panel* panel, uint64_t seed, uint64_t first_rep, uint64_t n_reps, int ref_mode,
                               double* d_rows, uint8_t* d_ok, void* hip_stream);
/* One process driving several GPUs: panels[i] (the same design, each created in an ob_ctx on a
   distinct device) takes shard i of n_panels; the shards are all-gathered over an RCCL clique of
   those devices (ncclCommInitAll, cached per device list) and rows/ok (host) receive all n_reps
   rows. */
int ob_boot_run_multi(ob_panel* const* panels, int n_panels, uint64_t seed, uint64_t first_rep, uint64_t n_reps,
                      int ref_mode, double* rows, uint8_t* ok);

/* The row columns the sharded entry points move over RCCL (ascending offsets into a row; n = 0 or
   every column: whole rows, the default). Aggregation reads only the component columns (two-fold,
   three-fold, total gap, detailed: [0, 6 + 2 Kd), plus the selection terms of a Heckman row), so a
   caller that only aggregates gathers those: 48 of 153 f64 per replicate at K = 21. Delivered rows
   then hold the other columns for this rank's own replicates only (NaN for the other ranks'). */
int ob_panel_set_gather_columns(ob_panel* panel, const int32_t* cols, int32_t n);
/* Test hook: a sharded run of `world` ranks simulated on this panel's one GPU -- each rank's shard
   computed and packed in turn and copied to where ncclAllGather would place it -- then delivered to
   host rows/ok as rank self_rank would receive them (the layout arithmetic of ob_shard_layout.h and
   the pack / unpack kernels of the real path, without the collective). */
int ob_debug_shard_sim(ob_panel* panel, int world, int self_rank, uint64_t seed, uint64_t first_rep, uint64_t n_reps,
                       int ref_mode, double* rows, uint8_t* ok);

/* ---- test hook: the OBRS-3 resample counts themselves (bitwise parity, builder.rs:822-827) ----
 * For replicates [first_rep, first_rep + n_reps) of `group` (0 = A, 1 = B): level1 receives
 * n_reps x ceil(n_g / 256) tile counts and row_counts n_reps x n_g per-row draw counts, exactly
 * as the Gram kernel consumes them. Either output may be NULL. */
int ob_debug_counts(ob_panel* panel, uint64_t seed, uint64_t first_rep, uint32_t n_reps, int group,
                    uint32_t* level1, uint8_t* row_counts);
/* Test hook: the reduced extended Grams G_r = sum_i c_ri v_i v_i^T (upper triangle, row-major pairs,
   e_pad per group) of replicates [first_rep, first_rep + n_reps <= 16384), gram: n_reps x 2 x e_pad,
   computed by path 1 (f64 MFMA) or 2 (exact integer-sliced i8 MFMA); 0 = the default choice. */
int ob_debug_gram(ob_panel* panel, int path, uint64_t seed, uint64_t first_rep, uint32_t n_reps, double* gram);
/* Test hook: the i8 Gram's exception rows once the panel's digit images exist:
   *bits = the threshold B, *n_exc = the number of exception rows, rows[0 .. min(cap, n_exc)) =
   (group << 31 | row) ascending. */
int ob_debug_gram_exceptions(ob_panel* panel, int32_t* bits, int32_t* n_exc, uint32_t* rows, int32_t cap);
/* Test hook: the panel's row chunking (a function of the panel only): *n_chunks chunks, and
   table[3 c .. 3 c + 2] = (group, first 256-row tile, end tile) for c < min(cap, *n_chunks).
   Host only; the Gram kernels, the exception rule and the reduce all use this table. */
int ob_debug_chunks(const ob_panel* panel, uint32_t* table, int32_t cap, int32_t* n_chunks);
/* Test hook: one Machado-Mata pass of replicate `rep` (0xFFFFFFFF: the point pass on the
   unresampled panel) and the coefficients of its quantile regressions: betas[(g S + s) K + k] for
   group g, simulation s < S = simulations (tau_s of MM-1), NaN where the fit failed; done[g S + s] = 1
   where it converged. For checks of LP optimality (objective, residual signs) on degenerate data. */
int ob_debug_mm_betas(ob_panel* panel, uint64_t seed, int32_t simulations, uint64_t rep, double* betas,
                      uint8_t* done);
/* Process-wide engine options (no reference counterpart: test and A/B switches). The library reads
   no environment variable; a caller sets these explicitly. value NaN restores the default.
     "gram_path"   1: f64 MFMA Gram, 2: i8 Gram (OB_E_UNSUPPORTED if its images do not fit)
     "gram_digits" 7: seven digit slices on every i8 column tile
     "hk_erfc"     0: library erfc in the Heckman probit/IMR kernels (default: npdf_ncdf)
     "mm_reduce"   0: no Machado-Mata row reduction, 1: always (default: both groups >= 2^16 rows)
     "mm_trace"    nonzero: Machado-Mata per-iteration trace on stderr
     "mm_state_gb", "mm_delta1", "mm_delta2", "mm_tol1", "mm_fit_stride", "mm_kappa", "mm_band0":
                   Machado-Mata tuning (the verification keeps results exact)
     "gram_diag", "l1_diag": timing ablations, tuning builds only (OB_E_UNSUPPORTED otherwise)
     "gram_tile"   1: the 8-wave i8 Gram kernel, 2: the wide-tile one, 3: the wide tile split (default: whichever the launch's
                   block count favours; their Grams are bitwise equal)
     "debug_count_overflow" nonzero: the resample's count-overflow word is raised after every
                   count kernel of a Machado-Mata run or ob_debug_counts (tests the OB_E_OVERFLOW path)
     "rs_double"   1: two level-1 / count-image buffers per panel, so each boot segment's resample
                   runs under the previous segment's Gram (rows bitwise unchanged; twice the image HBM),
                   0: one buffer (default: the engine's rule)
     "akm_poll"    n >= 1: the AKM loops read their device-side done flags every n iterations (default 8;
                   results and iteration counts bitwise unchanged)
     "hk_batch"    n >= 1: Heckman panels with more than 7 selection predictors run each boot segment in
                   batches of at most n 64-replicate blocks (default: as many as keep the chunk partials
                   within 1 GiB; rows bitwise unchanged)
   Unknown names are OB_E_INVALID. ob_get_option reads back what ob_set_option stored (NaN: unset). ob_tuning_build() is 1 in a -DOB_TUNING=1 build (`make tuning`),
   which also reads OB_<NAME> from the environment for options nobody set. */
int ob_set_option(const char* name, double value);
int ob_get_option(const char* name, double* value);
/* Test hook: the Heckman kernels' normal pdf and cdf (npdf_ncdf: W. J. Cody's rational erfc with
   the pdf's exponential shared, ob_heckman.hip) on the device at z[0 .. n). */
int ob_debug_normal(int device, const double* z, int64_t n, double* pdf, double* cdf);
int ob_tuning_build(void);

/* ---- inference (host) --------------------------------------------------------------------- */
/* inference.rs:4-34: out = {std_err, p_value, ci_lower, ci_upper}; n = 0 gives NaNs. */
int ob_bootstrap_stats(const double* estimates, int64_t n, double point_estimate, double out[4]);
/* process_component over replicate rows (builder.rs:849-865): bootstrap_stats of row column
   cols[c] over the rows with ok != 0, in replicate order; out: n_cols x {std_err, p_value,
   ci_lower, ci_upper}. Multithreaded on the host. */
int ob_aggregate(const double* rows, const uint8_t* ok, uint64_t n_reps, int32_t row_len, const int32_t* cols,
                 int32_t n_cols, double* out);
/* math/rif.rs:14-88 (R type-7 quantile, Silverman bandwidth, Gaussian KDE). */
int ob_rif(const double* y, int64_t n, double tau, double* out);

/* ---- builder: OaxacaBuilder over a column frame ------------------------------------------- */
#define OB_COL_F64 0
#define OB_COL_I64 1
#define OB_COL_STR 2

typedef struct {
  const char* name;
  int32_t kind;
  const double* f64;       /* OB_COL_F64 */
  const int64_t* i64;      /* OB_COL_I64 */
  const char* const* str;  /* OB_COL_STR; a NULL entry is a null */
  const uint8_t* valid;    /* numeric kinds: 1 = valid, 0 = null; NULL = all valid */
} ob_column;

/* ---- CSV front end (the reference CLI's LazyCsvReader, main.rs:161-165) ------------------
 * Header row; dtypes from the first 100 rows (i64, else f64, else str); empty field = null;
 * RFC 4180 quotes. ob_csv_column views stay valid until ob_csv_free. */
typedef struct ob_csv ob_csv;
int ob_csv_read(const char* path, ob_csv** out);
int ob_csv_dims(const ob_csv* csv, int64_t* nrows, int32_t* ncols);
int ob_csv_column(const ob_csv* csv, int32_t i, ob_column* out);
void ob_csv_free(ob_csv* csv);

typedef struct {
  const char* outcome;
  const char* group;
  const char* reference_group;
  const char* const* predictors;
  int32_t n_predictors;
  const char* const* categorical;
  int32_t n_categorical;
  const char* const* normalize;
  int32_t n_normalize;
  const char* weights;           /* NULL: unweighted */
  const char* selection_outcome; /* Heckman two-step (builder .heckman_selection): the 0/1 outcome */
  uint64_t bootstrap_reps;       /* builder default 20 (builder.rs:122) */
  int32_t reference_coeffs;      /* builder default OB_REF_GROUP_A (builder.rs:123) */
  int32_t has_seed;              /* 0: fresh entropy per run, like the unseeded reference */
  uint64_t seed;
  const char* const* selection_predictors; /* Heckman: z (intercept implicit), at most OB_HECKMAN_MAX_ZSEL */
  int32_t n_selection_predictors;
} ob_builder_config;

typedef struct ob_prepared ob_prepared;
typedef struct ob_results ob_results;
typedef struct ob_matrices ob_matrices;

/* clean_dataframe -> dummies -> split_groups -> prepare_data -> HBM upload -> point estimate
   (builder.rs:787-814). */
int ob_builder_prepare(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                       const ob_builder_config* cfg, ob_prepared** out);
int ob_prepared_row_len(const ob_prepared* prep);
int ob_prepared_n_y(const ob_prepared* prep);
uint64_t ob_prepared_seed(const ob_prepared* prep);
ob_panel* ob_prepared_panel(ob_prepared* prep);
int ob_prepared_boot(ob_prepared* prep, uint64_t first_rep, uint64_t n_reps, double* rows, uint8_t* ok);
/* ob_boot_run_sharded over the prepared panel (its seed and reference coefficients): with a rank
   context (ob_ctx_create_rank) each rank runs its shard and every rank receives all rows. Only the
   columns ob_prepared_finish aggregates travel (ob_panel_set_gather_columns): the coefficient and
   mean columns of the other ranks' replicates arrive as NaN. */
int ob_prepared_boot_sharded(ob_prepared* prep, uint64_t first_rep, uint64_t n_reps, double* rows, uint8_t* ok);
int ob_prepared_boot_device(ob_prepared* prep, uint64_t first_rep, uint64_t n_reps, double* d_rows,
                            uint8_t* d_ok, void* hip_stream);
/* Aggregation of builder.rs:841-950 over the successful rows (ok != 0), in replicate order. */
int ob_prepared_finish(ob_prepared* prep, const double* rows, const uint8_t* ok, uint64_t n_reps,
                       ob_results** out);
void ob_prepared_destroy(ob_prepared* prep);

/* prepare + all replicates + finish: OaxacaBuilder::run() (builder.rs:787). */
int ob_builder_run(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                   const ob_builder_config* cfg, ob_results** out);
/* OaxacaBuilder::decompose_quantile (builder.rs:711-757). */
int ob_builder_decompose_quantile(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                                  const ob_builder_config* cfg, double quantile, ob_results** out);
/* Several quantiles in one run: out[t] = decompose_quantile(taus[t]),
   bitwise, from one panel whose outcomes are the n_taus RIF columns, so one Gram pass and one
   resample per replicate serve every tau. out must hold n_taus slots. */
int ob_builder_decompose_quantiles(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                                   const ob_builder_config* cfg, const double* taus, int32_t n_taus,
                                   ob_results** out);
/* OaxacaBuilder::get_data_matrices (builder.rs:252-291). Host only: needs no GPU. */
int ob_builder_data_matrices(const ob_column* cols, int32_t n_cols, int64_t n_rows,
                             const ob_builder_config* cfg, ob_matrices** out);

/* ---- results (types.rs:8-47,160-180) ------------------------------------------------------ */
#define OB_TABLE_TWO_FOLD 0            /* two_fold.aggregate: explained, unexplained */
#define OB_TABLE_DETAILED_EXPLAINED 1
#define OB_TABLE_DETAILED_UNEXPLAINED 2
#define OB_TABLE_DETAILED_SELECTION 3  /* Heckman only: intercept + selection predictors */
#define OB_TABLE_THREE_FOLD 4          /* endowments, coefficients, interaction */

typedef struct {
  const char* name; /* valid until ob_results_free */
  double estimate, std_err, t_stat, p_value, ci_lower, ci_upper;
} ob_component;

#define OB_VEC_RESIDUALS 0 /* point-estimate residuals of group B */
#define OB_VEC_XA_MEAN 1
#define OB_VEC_XB_MEAN 2
#define OB_VEC_BETA_STAR 3

double ob_results_total_gap(const ob_results* r);
int64_t ob_results_n_a(const ob_results* r);
int64_t ob_results_n_b(const ob_results* r);
int64_t ob_results_n_failed(const ob_results* r); /* dropped replicates (builder.rs:841-847) */
int ob_results_count(const ob_results* r, int32_t table);
int ob_results_component(const ob_results* r, int32_t table, int32_t i, ob_component* out);
int ob_results_vector(const ob_results* r, int32_t which, const double** data, int64_t* len);
void ob_results_free(ob_results* r);

/* get_data_matrices: X column-major n x K including the intercept column. */
int ob_matrices_dims(const ob_matrices* m, int64_t* n_a, int64_t* n_b, int32_t* k);
int ob_matrices_get(const ob_matrices* m, const double** x_a, const double** y_a, const double** x_b,
                    const double** y_b);
const char* ob_matrices_name(const ob_matrices* m, int32_t i);
void ob_matrices_free(ob_matrices* m);

/* ---- Machado-Mata (QuantileDecompositionBuilder, quantile_decomposition.rs:21-445) ---------
 * A pass (run_single_pass, :173-279): `simulations` quantile regressions per group at the MM-1
 * quantiles (csrc/ob_spec.h; the reference draws from an unseeded thread_rng), one MM-1 row pick
 * per group per successful simulation, predictions x_A b_A, x_B b_B, x_A b_B, and empirical
 * quantiles. Each QR (math/quantile_regression.rs:22-129, Clarabel LP) is solved on the GPU by an
 * interior-point method on its dual LP; the replicates are OBRS-3 resamples. */

/* Runs the point pass (every row once; with_point != 0) then one pass per replicate of
   [first_rep, first_rep + n_reps). rows: (with_point + n_reps) x 3 n_quantiles host doubles,
   [gap, characteristics, coefficients] per quantile; ok[r] = 0 where the pass failed (fewer than
   simulations / 2 successful fits in a group, :231-236). panel: unweighted, one outcome, at most
   31 predictor columns. Replaces run_single_pass + the bootstrap loop (:173-354). */
int ob_mm_run(ob_panel* panel, uint64_t seed, int32_t simulations, const double* quantiles,
              int32_t n_quantiles, uint64_t first_rep, uint64_t n_reps, int32_t with_point, double* rows,
              uint8_t* ok);
/* Test hook: make chosen quantile-regression fits count as failed, as Clarabel's non-Solved statuses
   do in the reference (quantile_regression.rs:120-128), to pin the pass's failure semantics
   (quantile_decomposition.rs:221-259): each group drops its failed fits independently, the
   survivors pair by index, and a pass with fewer than simulations / 2 successes in a group fails.
   mask: 2 x sims bytes [group][simulation]; fit (g, s) of pass rep fails when bit (rep & 7) of
   mask[g * sims + s] is set (the point pass has rep = 2^32 - 1, bit 7). sims = 0 clears it. */
int ob_debug_mm_fail(ob_panel* panel, const uint8_t* mask, int32_t sims);

typedef struct {
  const char* outcome;
  const char* group;
  const char* reference_group;
  const char* const* predictors;
  int32_t n_predictors;
  const char* const* categorical;
  int32_t n_categorical;
  const double* quantiles; /* NULL: the builder default {0.1, 0.25, 0.5, 0.75, 0.9} */
  int32_t n_quantiles;
  int32_t simulations;     /* builder default 200 */
  uint64_t bootstrap_reps; /* builder default 20 */
  int32_t has_seed;        /* 0: fresh entropy per run, like the reference's thread_rng */
  uint64_t seed;
} ob_qd_config;

typedef struct ob_qd_results ob_qd_results;
/* QuantileDecompositionBuilder::run over a column frame (quantile_decomposition.rs:281-445). */
int ob_quantile_decomposition_run(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                                  const ob_qd_config* cfg, ob_qd_results** out);
/* results_by_quantile: n entries keyed "q{floor(100 tau)}" (a repeated key keeps the later
   quantile, as the reference's HashMap does), in first-appearance order of the keys. */
int ob_qd_results_dims(const ob_qd_results* r, int32_t* n_entries, int64_t* n_a, int64_t* n_b);
/* comps[0..2] = Total Gap, Characteristics, Coefficients (QuantileDecompositionDetail). */
int ob_qd_results_get(const ob_qd_results* r, int32_t i, const char** key, ob_component* comps);
int64_t ob_qd_results_n_failed(const ob_qd_results* r);
void ob_qd_results_free(ob_qd_results* r);

/* ---- DFL reweighting (dfl.rs:34-195, math/logit.rs:31-118, math/kde.rs:20-59) ----------------
 * The distributional companion of the mean decomposition: a logit propensity score of group
 * membership reweights group B to group A's characteristics, then Gaussian kernel densities of the
 * outcome are evaluated on a grid for A, B and B's counterfactual. The n x K Newton passes and the
 * density sums run on the GPU; sums are f64 with a fixed reduction order (no atomics), so a call
 * repeated on the same input returns the same bytes. */

/* logit(): Newton-Raphson from beta = 0. x: column-major n x k with the intercept column supplied
   by the caller, ldx >= n; y: 0/1. p = sigmoid(x beta) clamped to [1e-10, 1 - 1e-10]; each step
   solves X^T diag(p (1 - p)) X step = X^T (y - p) by Cholesky; converged when ||step||_2 < tol.
   beta[k]; probs[n] (may be NULL) are the probabilities at the START of the last iteration when
   converged (the reference does not recompute them with the final beta) and those at the final
   beta after max_iter unconverged iterations. A Cholesky failure is OB_E_LINALG "Failed to solve
   Information Matrix in Logit. Perfect separation?". k <= OB_LOGIT_MAX_K, else OB_E_UNSUPPORTED
   before any work. */
#define OB_LOGIT_MAX_K 64
int ob_logit(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, int64_t n, int32_t k, int32_t max_iter,
             double tol, double* beta, double* probs, int32_t* converged, int32_t* iterations);
/* probit(): math/probit.rs::probit, Fisher scoring from beta = 0 on unresampled rows. x: column-major
   n x k, ldx >= n, with the caller's intercept as column 0 (all ones: the device kernels take z_0 = 1
   as given, anything else is OB_E_UNSUPPORTED); y: the 0/1 outcome. Phi is clamped to [1e-10,
   1 - 1e-10]; each step solves (sum w z z' + 1e-9 I) step = sum lambda z by Cholesky, LU with partial
   pivoting if that fails, and a step neither can solve is OB_E_LINALG "Failed to solve Hessian system
   in Probit". converged: ||step||_2 < tol within max_iter iterations (running out is not an error);
   *iterations: the steps taken. It runs the Heckman kernels as a one-replicate segment (register-
   resident for k <= 8, f64 MFMA above). k <= 32 (1 + OB_HECKMAN_MAX_ZSEL), else OB_E_UNSUPPORTED before
   any device work, as are the argument checks (OB_E_INVALID: null pointers, n <= 0, k < 1, ldx < n). */
#define OB_HECKMAN_MAX_ZSEL 31
int ob_probit(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, int64_t n, int32_t k, int32_t max_iter,
              double tol, double* beta, int32_t* converged, int32_t* iterations);
/* kde(): density[g] = sum_i w_i phi((grid[g] - data[i]) / bandwidth) / bandwidth with phi the
   standard normal pdf and w the weights over their sum (weights NULL: 1 / n). A grid point whose
   every term underflows gets exactly 0. */
int ob_kde(ob_ctx* ctx, const double* data, const double* weights, int64_t n, const double* grid, int64_t n_grid,
           double bandwidth, double* density);
/* silverman_bandwidth() of math/kde.rs:44-59 (not the RIF one): 0.9 min(sd, iqr / 1.34) n^-0.2 with
   the (n - 1) variance and quartiles sorted[(size_t)(n 0.25)], sorted[(size_t)(n 0.75)]. Host only. */
int ob_silverman_bandwidth(const double* data, int64_t n, double* out);

typedef struct {
  const char* outcome;
  const char* group;
  const char* reference_group;
  const char* const* predictors;
  int32_t n_predictors;
  int32_t grid_size; /* 0: the reference's 100 */
} ob_dfl_config;

typedef struct ob_dfl_results ob_dfl_results;
/* run_dfl over a column frame. Group A is the first sorted unique value of the group column that
   is not the reference; the logit target is 1 on A's rows and 0 on EVERY other row (a null group
   reads as ""), while n_b counts the reference's rows only. OB_COL_STR predictors become dummies
   "{col}_{val}" over the sorted levels without the first; numeric ones are cast to f64. No rows are
   dropped (no clean_dataframe). logit(y, X, 100, 1e-6); B's rows get psi = p / (1 - p) * (n_b / n) /
   (n_a / n) with p clamped to [1e-4, 0.9999]; grid[i] = min + i (max - min) / grid_size for
   i < grid_size; Silverman bandwidths of A's and of the non-A outcomes (the counterfactual uses the
   latter). Errors: a missing column, a non-string group column or a non-f64 outcome is OB_E_POLARS;
   a null outcome is OB_E_GROUP "Null outcome encountered in DFL".
   Stricter than the reference (which would carry NaNs or panic): an empty group A or an empty
   reference group is OB_E_GROUP, a null in a predictor column is OB_E_POLARS. */
int ob_dfl_run(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_dfl_config* cfg,
               ob_dfl_results** out);
/* DflResult (dfl.rs:10-19): *n_grid points; the arrays stay valid until ob_dfl_results_free. */
int ob_dfl_results_get(const ob_dfl_results* r, int64_t* n_grid, const double** grid, const double** density_a,
                       const double** density_b, const double** density_b_counterfactual);
typedef struct {
  int64_t n_a, n_b;          /* rows equal to A / to the reference */
  int32_t logit_iterations;
  int32_t logit_converged;
  double bandwidth_a, bandwidth_b;
  const char* group_a;       /* valid until ob_dfl_results_free */
  double logit_ms;           /* HIP-event ms of the Newton-pass launches, summed */
  double kde_ms;             /* HIP-event ms of the three KDE launches, summed */
} ob_dfl_info;
int ob_dfl_results_info(const ob_dfl_results* r, ob_dfl_info* out);
void ob_dfl_results_free(ob_dfl_results* r);

/* ---- Matching (matching/engine.rs, matching/distance.rs, matching/logistic.rs) -----------------
 * Nearest-neighbour matching with replacement on raw covariates, on Mahalanobis-transformed ones or
 * on a propensity score. The all-pairs distance pass, the control covariance, the transform and the
 * logistic's n x K sums run on the GPU; counts are integer atomics and every f64 sum has a fixed
 * order, so a call repeated on the same input returns the same bytes.
 *
 * The one deliberate difference from the reference: among exactly equidistant controls its choice
 * depends on the shape of its k-d tree. Here the k nearest are the k smallest by the lexicographic
 * key (squared distance, control position), whatever the launch shape. */

#define OB_MATCH_MAX_DIM 64 /* covariates */
#define OB_MATCH_MAX_K 16   /* neighbours */
/* The min(k, n_c) nearest controls of each query. queries: column-major n_q x dim, ldq >= n_q;
   controls: column-major n_c x dim, ldc >= n_c (entries past n_q / n_c of a column are never read).
   The squared distance is 0 + t_0 t_0 + t_1 t_1 + ... with t_j = q_j - c_j in covariate order, each
   product and sum rounded on its own (no FMA), which is the kdtree crate's squared_euclidean bit
   for bit. idx[n_q][k] (control positions) and dist2[n_q][k] are ascending by (dist2, position);
   entries past min(k, n_c) hold -1 / +inf. dim > OB_MATCH_MAX_DIM or k > OB_MATCH_MAX_K is
   OB_E_UNSUPPORTED before any device work; a non-finite coordinate is OB_E_DIAG. */
int ob_knn(ob_ctx* ctx, const double* queries, int64_t ldq, int64_t n_q, const double* controls, int64_t ldc,
           int64_t n_c, int32_t dim, int32_t k, int64_t* idx, double* dist2);
/* LogisticRegression::fit + predict_proba of matching/logistic.rs (not math/logit.rs, which
   ob_logit restates): Newton-Raphson from beta = 0 with p = 1 / (1 + e^-x beta) unclamped, 1e-6
   added to the Hessian's diagonal, an LU solve with partial pivoting (a zero pivot is OB_E_DIAG
   "Hessian is singular"), beta += delta, stop when ||delta||_2 < tol; running out of iterations is
   not an error. x: column-major n x k with the intercept supplied by the caller, ldx >= n; y: the
   target as given. beta[k]; probs[n] (may be NULL) are the scores at the final beta. *converged:
   whether the last step was under tol; *iterations: the steps taken. k <= OB_LOGIT_MAX_K. */
int ob_match_logistic(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, int64_t n, int32_t k,
                      int32_t max_iter, double tol, double* beta, double* probs, int32_t* converged,
                      int32_t* iterations);

enum { OB_MATCH_EUCLIDEAN = 0, OB_MATCH_MAHALANOBIS = 1, OB_MATCH_PSM = 2 };
typedef struct {
  const char* treatment;
  const char* outcome; /* read by OB_MATCH_PSM only; the other methods never look at it */
  const char* const* covariates;
  int32_t n_covariates;
  int32_t k;
  int32_t method; /* OB_MATCH_* */
} ob_match_config;

typedef struct ob_match_results ob_match_results;
/* run_matching(k, use_mahalanobis) / match_psm(k) over a column frame.
   Groups: treated rows have a treatment value equal to 1, controls one equal to 0 (any numeric
   column); every other row, a null included, is in neither and gets weight 0. A string treatment
   column is OB_E_POLARS. Covariates are cast to f64.
   Mahalanobis: S is the covariance of the CONTROL rows (centred, n - 1 divisor; fewer than 2 controls
   is OB_E_DIAG "Not enough data points to calculate covariance"), S^-1 a general inverse (adjugate
   up to dimension 4, LU with partial pivoting beyond; OB_E_DIAG "Covariance matrix is singular and
   cannot be inverted"), L its lower Cholesky factor (OB_E_DIAG "Cholesky decomposition failed"),
   and both groups become X L.
   Each treated row takes its min(k, n_c) nearest controls (ob_knn's distance and key); k = 0 or no
   controls selects nothing. A treated row's weight is 1; a control matched m times gets 0.0 with the
   f64 value 1.0 / k added m times in sequence (not m / k).
   PSM first makes prepare_data's checks: an empty treated or control group is OB_E_GROUP "One group
   is empty", a missing or non-f64 outcome OB_E_POLARS, a null outcome in a treated or control row
   OB_E_GROUP "Null values in outcomes"; a non-f64 treatment column is OB_E_POLARS here. The design
   is an intercept and the covariates of ALL rows, the target the raw treatment value (null: 0.0),
   fitted by ob_match_logistic(.., 100, 1e-6); the scores are then the single covariate of a
   Euclidean match.
   Stricter than the reference (which would carry NaNs into its tree): a null in a covariate column
   is OB_E_POLARS, a non-finite coordinate of a treated or control row after the transform is
   OB_E_DIAG. n_covariates > OB_MATCH_MAX_DIM or k > OB_MATCH_MAX_K is OB_E_UNSUPPORTED. */
int ob_match_run(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_match_config* cfg,
                 ob_match_results** out);
/* weights[*n_rows]: the reference's return value. An extension: treated_rows[*n_treated] are the
   treated rows' frame positions, and neighbor_rows / neighbor_dist2 [*n_treated][*k_out] their
   neighbours' frame positions and squared distances in ob_knn's order (-1 / +inf past
   min(k, n_control)). Any out pointer may be NULL; the arrays live until ob_match_results_free. */
int ob_match_results_get(const ob_match_results* r, int64_t* n_rows, const double** weights, int64_t* n_treated,
                         int32_t* k_out, const int64_t** treated_rows, const int64_t** neighbor_rows,
                         const double** neighbor_dist2);
typedef struct {
  int64_t n_treated, n_control;
  int32_t logistic_iterations; /* OB_MATCH_PSM, else 0 */
  int32_t logistic_converged;
  double knn_ms;  /* HIP-event ms of the distance pass and its merge */
  double prep_ms; /* HIP-event ms of everything else on the device: covariance, transform, logistic, packing */
} ob_match_info;
int ob_match_results_info(const ob_match_results* r, ob_match_info* out);
void ob_match_results_free(ob_match_results* r);

/* ---- AKM two-way fixed effects (akm.rs:47-621) -------------------------------------------------
 * y = x beta + alpha[worker] + psi[firm] + e on the largest connected set of the worker-firm graph:
 * the outcome and every control are demeaned by alternating worker and firm means until a fixed
 * point (demean_vector), beta is the OLS of the demeaned outcome on the demeaned controls, and the
 * effects come from alternating means of the residual (recover_fe). The group means, the Gram and
 * the R^2 sums run on the GPU as segmented reductions over the rows grouped by worker and by firm;
 * every sum is f64 in a fixed order that depends only on the input's sizes and group layout (no
 * floating atomics), so a call repeated on the same input returns the same bytes, and a column gives
 * the same bytes and iteration count demeaned alone or in any batch.
 *
 * The one deliberate difference from the reference: among components with equally many nodes its
 * choice follows HashMap iteration order. Here the component holding the smallest sorted worker id
 * wins. */
#define OB_AKM_MAX_CONTROLS 64

typedef struct ob_akm_set ob_akm_set;
/* find_largest_connected_set (akm.rs:151-234) and the dense indices of solve_akm (akm.rs:246-303).
   Host only: needs no GPU. Id columns are OB_COL_STR or OB_COL_I64 (cast to decimal strings, so they
   sort as strings: "10" < "9"); an OB_COL_F64 id column is OB_E_UNSUPPORTED. Nodes are the distinct
   non-null worker and firm ids, edges the rows with both ids non-null; the component with the most
   nodes (workers + firms, not rows) is kept. Rows outside it or with a null id are dropped; no kept
   row is OB_E_INSUFFICIENT "No connected set found". A missing column is OB_E_COLUMN. */
int ob_akm_connected_set(const ob_column* cols, int32_t n_cols, int64_t n_rows, const char* worker_col,
                         const char* firm_col, ob_akm_set** out);
/* keep[*n_rows]: 1 for a kept row; worker_idx / firm_idx[*n_kept]: the dense index of each kept row, in
   row order, over the kept ids in sorted string order; *n_components counts every component of the
   graph. Any out pointer may be NULL; the arrays live until ob_akm_set_free. */
int ob_akm_set_get(const ob_akm_set* s, int64_t* n_rows, const uint8_t** keep, int64_t* n_kept,
                   const int32_t** worker_idx, const int32_t** firm_idx, int64_t* n_workers, int64_t* n_firms,
                   int64_t* n_components);
/* The i-th sorted kept id: which = 0 worker, 1 firm. NULL when out of range. */
const char* ob_akm_set_id(const ob_akm_set* s, int32_t which, int64_t i);
void ob_akm_set_free(ob_akm_set* s);

/* demean_vector (akm.rs:452-527) of n_cols columns in one batch. v and out: column-major n x n_cols
   with leading dimension ldv >= n (entries past n of a column are never read or written). Each
   iteration subtracts every worker's mean, then every firm's mean of the result, and a column stops
   at the first iteration whose change ||v - prev||_2 is not above tol, or after max_iters; the rule is
   evaluated on the device per column and a stopped column is frozen. iterations[n_cols]; converged[c]
   = iterations[c] < max_iters, the reference's own test, so a column that converges in its last
   allowed iteration, or max_iters = 0, reads as not converged. That is reported, not an error.
   worker_idx / firm_idx: n dense indices in [0, n_workers) / [0, n_firms), else OB_E_INVALID. */
int ob_akm_demean(ob_ctx* ctx, const double* v, int64_t ldv, int64_t n, int32_t n_cols, const int32_t* worker_idx,
                  const int32_t* firm_idx, int64_t n_workers, int64_t n_firms, double tol, int64_t max_iters,
                  double* out, int32_t* iterations, int32_t* converged);
/* recover_fe (akm.rs:530-621): from alpha = psi = 0, alpha_w = mean(r - psi[firm] | w), then psi_f =
   mean(r - alpha[worker] | f) with the new alpha, until the 2-norm of the change of (alpha, psi) is
   not above tol; then psi[0] is subtracted from every psi and added to every alpha (skipped when not
   converged, where the reference returns nothing). The same converged rule as ob_akm_demean. */
int ob_akm_recover_fe(ob_ctx* ctx, const double* r, int64_t n, const int32_t* worker_idx, const int32_t* firm_idx,
                      int64_t n_workers, int64_t n_firms, double tol, int64_t max_iters, double* alpha, double* psi,
                      int32_t* iterations, int32_t* converged);

typedef struct {
  const char* outcome;
  const char* worker_col;
  const char* firm_col;
  const char* const* controls;
  int32_t n_controls;
  double tolerance;  /* 0: the reference's 1e-8 */
  int64_t max_iters; /* negative: the reference's 1000 (0 stays 0, which fails at once as there) */
} ob_akm_config;

typedef struct ob_akm_results ob_akm_results;
/* AkmBuilder::run over a column frame. The outcome and the controls must be OB_COL_F64 (else
   OB_E_POLARS); a null outcome in a kept row is OB_E_INSUFFICIENT "Null outcome encountered", a null
   control reads as 0.0. A loop that ends with iterations >= max_iters is OB_E_CONVERGENCE
   "demean_vector failed to converge within N iterations" / "recover_fe failed ...", a failed Cholesky
   of X'X OB_E_CONVERGENCE "OLS design matrix is singular". More than OB_AKM_MAX_CONTROLS controls, or
   2^31 or more rows or nodes, is OB_E_UNSUPPORTED before any device work. r2 = 1 - rss / tss. */
int ob_akm_run(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_akm_config* cfg,
               ob_akm_results** out);
/* AkmResult (akm.rs:39-44): beta[*n_controls]; the sorted worker ids and their effects, the sorted firm
   ids and theirs. Any out pointer may be NULL; everything lives until ob_akm_results_free. */
int ob_akm_results_get(const ob_akm_results* r, int32_t* n_controls, const double** beta, int64_t* n_workers,
                       const char* const** worker_ids, const double** worker_effects, int64_t* n_firms,
                       const char* const** firm_ids, const double** firm_effects, double* r2);
typedef struct {
  int64_t n_rows_kept, n_workers, n_firms, n_components;
  const int32_t* demean_iterations; /* 1 + n_controls entries: the outcome, then the controls */
  int32_t n_demean;
  int32_t recover_iterations;
  int32_t launches_per_iteration; /* kernel launches of one demean iteration */
  double demean_ms;  /* HIP-event ms of the demean loop */
  double ols_ms;     /* the Gram, the residual and the R^2 sums */
  double recover_ms; /* the recover_fe loop and the normalisation */
} ob_akm_info;
int ob_akm_results_info(const ob_akm_results* r, ob_akm_info* out);
void ob_akm_results_free(ob_akm_results* r);

/* ---- VIF collinearity diagnostic (math/diagnostics.rs:29-109 over math/ols.rs:44-144) -----------
 * calculate_vif: for predictors x_0..x_{k-1}, in the order given, regress x_j on [the others in that
 * order, then the intercept LAST] and score 1 / (1 - r2). The reference runs k fits of n rows; here
 * all of them read one extended Gram G = Xe^T Xe, Xe = [x_0..x_{k-1}, 1], formed on the GPU, the k
 * Cholesky solves run on the host in nalgebra's operation order, and one more GPU pass over the rows
 * gives every fit's residual and total sums of squares from explicit residuals (never from
 * G_jj - b^T beta, which cancels as r2 -> 1). Sums are f64 in a fixed order that depends on the shape
 * only (no floating atomics), so a call repeated on the same input returns the same bytes.
 *
 * Errors, in this order and before any device work: k < 2 is OB_E_DIAG "VIF calculation requires at
 * least two predictors."; k > OB_VIF_MAX_K is OB_E_UNSUPPORTED; n <= k is OB_E_INSUFFICIENT
 * "Insufficient data for OLS calculation: n_obs (n) must be strictly greater than k (k)". A Cholesky
 * failure of ANY fit is OB_E_LINALG "Failed to perform Cholesky decomposition. Matrix may be singular
 * or not positive definite due to multicollinearity." and fails the whole call, as in the reference
 * (whose INFINITY arm matches a message ols never produces). A NaN or infinite value ends there too.
 *
 * The one deliberate difference from the reference: a null in a named column of ob_vif_run is
 * OB_E_INVALID naming the column. The reference reads a null regressand as 0.0 while the regressors
 * keep it as missing. */
#define OB_VIF_MAX_K 120
/* x: column-major n x k, ldx >= n (entries past n of a column are never read). gram: (k + 1)^2
   column-major, both triangles filled; row and column k are the intercept's (gram[k][k] = n). */
int ob_vif_gram(ob_ctx* ctx, const double* x, int64_t ldx, int64_t n, int32_t k, double* gram);
/* The k auxiliary fits from one Gram. Host only: takes no ctx and needs no GPU. coef: (k + 1) x k
   column-major; column j holds fit j's coefficients at the positions of Xe (row k: the intercept),
   with coef[j][j] = 0. */
int ob_vif_solve(const double* gram, int64_t n, int32_t k, double* coef);
/* ss_res[j] = sum_i (x_ij - xe_i . coef_j)^2 and ss_tot[j] = sum_i (x_ij - means[j])^2, j < k.
   means[k]: ob_vif uses gram[j][k] / n. */
int ob_vif_sums(ob_ctx* ctx, const double* x, int64_t ldx, int64_t n, int32_t k, const double* coef,
                const double* means, double* ss_res, double* ss_tot);
/* The three above over one upload of x. vif[k]: +inf where ss_tot == 0 or |1 - r2| < 1e-9 with
   r2 = 1 - ss_res / ss_tot, else 1 / (1 - r2). */
int ob_vif(ob_ctx* ctx, const double* x, int64_t ldx, int64_t n, int32_t k, double* vif);
/* The calling thread's last ob_vif or ob_vif_run: HIP-event ms of the Gram pass and of the residual
   pass (each with its reduce), host ms of the k solves. Any out pointer may be NULL. */
int ob_vif_last_timing(double* gram_ms, double* solve_ms, double* sums_ms);
/* calculate_vif over a column frame: vif[n_names] in the order of names. A missing column is
   OB_E_COLUMN, an OB_COL_STR column OB_E_POLARS, OB_COL_I64 is cast to f64, a name given twice is
   OB_E_INVALID (before any device work, with the shape errors above). */
int ob_vif_run(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const char* const* names,
               int32_t n_names, double* vif);

/* ---- Pay-equity remediation: fair-wage scoring and budget allocation (engine/src/analysis.rs:309-869,
 * optimize_inner) over arrays. The engine's "A" is the reference group, "B" the target. The design is
 * [1, features]: k columns, the intercept FIRST and implicit (x holds the k - 1 features), rows stacked
 * with A's n_a rows first. The chain: the Gram of [features, y] (ob_vif_gram, over A's rows and, for the
 * Pooled target, over all rows) -> ob_remedy_solve (host) -> ob_remedy_score (one GPU pass: fair wage,
 * leverage, A's residual sum) -> ob_remedy_allocate (GPU: classify, stable descending sort, running
 * budget in closed form, output ordered by original index).
 *
 * Deliberate differences from the reference: beta comes from the Cholesky solve of the normal
 * equations in nalgebra's operation order, not from an SVD (the reference needs X'X invertible two
 * lines later anyway); greedy pay is clamp(budget - P_c, 0, diff_c) with P_c the exclusive prefix sum of
 * the eligible diffs before candidate c in sorted order, which agrees with the reference's sequential
 * current_spend to rounding. P_c's order: an inclusive Kogge-Stone scan (offsets 1, 2, .. 128) within
 * each tile of 256 sorted candidates, plus the totals of the tiles before it added one by one in tile
 * order; it depends on the candidate count alone. Every sum is f64 in a fixed order (no floating
 * atomics), so a repeated call returns the same bytes. */
#define OB_REMEDY_MAX_K 120 /* design columns, the intercept included: at most 119 beside it */
enum { OB_REMEDY_TARGET_REFERENCE = 0, OB_REMEDY_TARGET_POOLED = 1 };
enum { OB_REMEDY_GREEDY = 0, OB_REMEDY_EQUITABLE = 1 };
enum { OB_REMEDY_MIDPOINT = 0, OB_REMEDY_LOWER = 1, OB_REMEDY_UPPER = 2 };
typedef struct {
  double budget;              /* > 0, else the auto budget total_need * 1.00001 (analysis.rs:697-703) */
  double min_gap_pct;         /* a row is eligible when diff / actual >= this */
  double confidence_level;    /* clamped to [0.50, 0.999]; 0.95 when NaN */
  int32_t strategy;           /* OB_REMEDY_GREEDY | OB_REMEDY_EQUITABLE */
  int32_t range_target;       /* OB_REMEDY_MIDPOINT | _LOWER | _UPPER: group B's target wage */
  int32_t forensic_mode;      /* also return the ineligible and non-positive rows, with pay 0 */
  int32_t adjust_both_groups; /* group A's positive gaps are eligible too (always against the midpoint) */
} ob_remedy_request;
typedef struct ob_remedy_results ob_remedy_results;
typedef struct {
  int64_t n_a, n_b, n_adjustments;
  double total_cost, required_budget, effective_budget, net_residual_sum_b;
  double original_unexplained_gap, new_unexplained_gap; /* analysis.rs:847-857 */
  double z_score, sigma_squared;
  double classify_ms, order_ms, allocate_ms; /* HIP-event ms */
  double original_gap, new_gap;              /* ob_remedy_run only (analysis.rs:836-845), else 0 */
  double gram_ms, score_ms;                  /* ob_remedy_run only: HIP-event ms of the Gram and score passes */
} ob_remedy_info;
/* statrs Normal(0, 1)::inverse_cdf(p) = -sqrt(2) erfc_inv(2 p), term by term (its erf_inv_impl
   rational approximations in its evaluation order). NaN outside [0, 1]. Host only. */
double ob_normal_inverse_cdf(double p);
/* beta[k] and cov[k * k] (column-major, (X_A'X_A)^-1 by nalgebra's try_inverse) in DESIGN order
   (intercept first) from Grams in ob_vif_gram's layout over [features(k - 1), y]: (k + 1)^2, the
   columns being the features, then y, then the ones. gram_fit: the fit rows' Gram, or NULL to fit on
   A (OptimizationTarget::Reference). Host only. k < 2 or NULL is OB_E_INVALID, k > OB_REMEDY_MAX_K
   OB_E_UNSUPPORTED, a singular matrix OB_E_LINALG "Covariance matrix is singular, likely due to perfect
   multicollinearity." */
int ob_remedy_solve(const double* gram_a, const double* gram_fit, int32_t k, double* beta, double* cov);
/* One pass over n stacked rows: fair[i] = xe_i . beta, leverage[i] = xe_i' cov xe_i (T = Xe cov on the
   f64 matrix units, then a row dot with xe_i), *rss = sum over the FIRST n_rss rows of (y_i - fair_i)^2
   from explicit residuals, and on request contrib[i + j * n] = xe_ij beta_j. x: column-major
   n x (k - 1), ldx >= n. y (n_rss entries read), rss and contrib may be NULL. */
int ob_remedy_score(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, int64_t n, int64_t n_rss,
                    int32_t k, const double* beta, const double* cov, double* fair, double* leverage,
                    double* rss, double* contrib);
/* analysis.rs:516-834 over the stacked rows (A's n_a first, then B's n_b): intervals from sigma_squared
   and the request's confidence, classification, allocation. index[n_a + n_b]: each row's original
   index, or NULL for its stacked position. Returns one entry per adjustment, ordered by index. A
   non-finite y, fair or leverage is OB_E_INVALID: the reference's partial_cmp(..).unwrap_or(Equal) gives
   a NaN gap an order that depends on its sort's internals. */
int ob_remedy_allocate(ob_ctx* ctx, const double* y, const double* fair, const double* leverage, int64_t n_a,
                       int64_t n_b, const int64_t* index, double sigma_squared, const ob_remedy_request* request,
                       ob_remedy_results** out);
int ob_remedy_results_info(const ob_remedy_results* r, ob_remedy_info* out);
/* Arrays of n_adjustments entries, owned by r; any out pointer may be NULL. group: 0 = A, 1 = B;
   row: the stacked row. */
int ob_remedy_results_get(const ob_remedy_results* r, const int64_t** index, const double** adjustment,
                          const double** current_wage, const double** new_wage, const double** fair_wage,
                          const double** lower, const double** upper, const int32_t** group, const int64_t** row);
void ob_remedy_results_free(ob_remedy_results* r);
/* optimize_inner over a column frame (ob_remedy_run only): the design's k column names (the intercept
   first) with the fair-wage coefficients, and, when contributions were asked for, n_adjustments x k
   row-major values xe_ij beta_j (else NULL). Owned by r. */
int ob_remedy_results_model(const ob_remedy_results* r, int32_t* k, const char* const** names, const double** beta,
                            const double** contributions);
/* optimize_inner (analysis.rs:309-869) over a column frame and a builder configuration: the builder's
   design (intercept and dummies included), Pooled reference coefficients and the existing point estimate
   for original_gap, one upload of the stacked rows, then the Gram, the solve, the score pass and the
   allocation above. target: OB_REMEDY_TARGET_REFERENCE | _POOLED (A's and B's Grams are formed separately
   and added on the host). As in the reference, whose optimize_inner calls run() first, a group with no more
   rows than design columns is OB_E_INSUFFICIENT from the point estimate; the dof <= 0 rule (sigma_squared
   = 0) is therefore reachable only through the array pieces.
   Errors, before any device work and in this order: a bad request or target is OB_E_INVALID; a named
   column that is missing is OB_E_COLUMN "Column '<name>' not found in dataset."; a null in a named
   column is OB_E_INVALID (deliberate: the reference indexes the uncleaned frame with rows of the cleaned
   one); a non-finite outcome is OB_E_INVALID (a NaN gap has no place in the order); a group column that is
   not a string column is OB_E_POLARS, as the reference's `.str()` fails; anything but exactly two group
   values with the reference group among them is OB_E_UNSUPPORTED (deliberate: with more, the reference's
   indices and matrices disagree); more than OB_REMEDY_MAX_K design columns is OB_E_UNSUPPORTED. */
int ob_remedy_run(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                  const ob_remedy_request* request, int32_t target, int32_t contributions, ob_remedy_results** out);

/* calculate_efficient_frontier_inner (analysis.rs:871-1153): ob_remedy_run with budget 0, Reference target,
   Greedy and Midpoint gives the gaps; max_budget (NaN: 1.1 x total need; below 1e-9: 1000) is cut into `steps`
   slices, and for each of the steps + 1 budgets b_s = s * max_budget / steps the wages y + pay_s, pay_s[i] =
   clamp(b_s - P_i, 0, gap_i) (P_i: the gaps before i in descending order, ties by original index, added one by
   one on the host), are regressed on the pooled design [1, group dummy (A = 0, B = 1), features]. Two GPU
   passes serve all budgets at once: X_p'Y on the f64 matrix units with Y never stored, then rss_s from explicit
   residuals; the steps + 1 solves use nalgebra's try_inverse of X_p'X_p on the host ("Singular matrix in Pooled
   OLS" is OB_E_LINALG). Deliberate difference: beta_s = (X_p'X_p)^-1 (X_p'Y_s), not the reference's dense K x n
   projector times Y_s. Per point: t = beta_group / sqrt(sigma2 (X_p'X_p)^-1[1][1]), p = 2 Phi(-|t|), significant
   when p < 0.05; (0, 1, 0) when n - (k + 1) <= 0. The arrays hold steps + 1 entries. steps < 1 is OB_E_INVALID,
   steps > OB_REMEDY_MAX_STEPS OB_E_UNSUPPORTED. ms (may be NULL): HIP-event ms of the two passes. */
#define OB_REMEDY_MAX_STEPS 127
int ob_remedy_frontier(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                       int32_t steps, double max_budget, double* budget, double* t_statistic, double* p_value,
                       int32_t* is_significant, double* ms);

/* ---- Defensibility and verification of edited raises (engine/src/defensibility.rs, check_defensibility_inner;
 * analysis.rs:40-96, verify_inner). check_defensibility scores every proposed raise against the reference
 * group's fair-wage interval and reports the gaps before and after; verify applies the raises to the wages and
 * runs the decomposition again.
 *
 * The reference finds a row's adjustment by walking the whole result list and stopping at the first hit
 * (defensibility.rs:292-301, :343-349): O(n m). Here first[row] = min { j : row_j = row } by a 32-bit integer
 * atomicMin (order-free, so deterministic) and one streamed pass over the rows: the FIRST adjustment of a row in
 * request order decides its new wage in every sum, while every adjustment, duplicates included, is returned.
 * Sums are f64 in a fixed order that depends on the sizes only (wave butterfly, waves in order, the ordered sum
 * of the block partials; no floating atomics), so a repeated call returns the same bytes. The reference adds
 * group B's terms in HashMap iteration order, so there is no order of its own to copy. */
typedef struct {
  int64_t n_a, n_b, n_adjustments; /* n_adjustments: the kept ones, as returned */
  int64_t n_skipped;               /* ob_remedy_defend: adjustments whose index is outside the frame */
  double total_cost;               /* the values of the kept adjustments, request order (:279-282) */
  double original_gap, new_gap;    /* mean_A - mean_B of the wages before and after (:316-330) */
  double original_unexplained_gap, new_unexplained_gap; /* sum_B (fair - wage) / n_b (:332-365) */
  double required_budget;          /* sum_B (fair - y) over fair > y (:266-276) */
  double z_score, sigma_squared;
  double gram_ms, score_ms;        /* ob_remedy_defend only: HIP-event ms of the Gram and score passes */
  double defend_ms;                /* HIP-event ms of the three passes below together */
  double scatter_ms, adjust_ms, rows_ms; /* the first-wins map, the per-adjustment pass, the row pass */
  double sums[7]; /* sum_A y, sum_A new, sum_B y, sum_B new, sum_B (fair - y), sum_B (fair - new), required_budget */
} ob_defend_info;
/* defensibility.rs:199-365 over stacked arrays as ob_remedy_allocate takes them (A's n_a rows first). rows[m],
   values[m]: the proposed adjustments as (stacked row, raise) in request order. Per adjustment: current =
   y[row], new = current + value (one add), fair, lower / upper = fair -+ z sqrt(sigma_squared (1 + h)) with z
   from confidence_level as in ob_remedy_request (the reference hard-wires 0.95), both equal to fair when
   sigma_squared <= 1e-9, and is_defensible = new >= lower - 1.0. Results through ob_remedy_results_get (index =
   row), ob_remedy_results_defensible and ob_remedy_results_defend_info.
   Errors, before any device work and in this order: negative n_a, n_b or m is OB_E_INVALID; n_a + n_b >= 2^31 -
   257 or m >= 2^31 - 1 is OB_E_UNSUPPORTED; a NULL array is OB_E_INVALID; a non-finite y, fair or leverage
   (deliberate, as ob_remedy_allocate) or a NaN sigma_squared is OB_E_INVALID; then, adjustment by adjustment, a
   row outside [0, n_a + n_b) or a non-finite value is OB_E_INVALID; a NULL ctx or out comes last. */
int ob_remedy_defend_rows(ob_ctx* ctx, const double* y, const double* fair, const double* leverage, int64_t n_a,
                          int64_t n_b, const int64_t* rows, const double* values, int64_t m, double sigma_squared,
                          double confidence_level, ob_remedy_results** out);
/* check_defensibility_inner over a column frame and a builder configuration. index[m], value[m]: the proposed
   adjustments by ORIGINAL row index, request order. Predictor overrides are a flat list of n_overrides entries
   (override_adjustment[i]: a position in the adjustments array; override_name[i]; override_value[i]), resolved
   by ob_remedy_resolve_overrides and applied to copies of the touched columns before the design is built. An
   override of a reference-group row therefore changes beta, cov and sigma_squared for everyone: that is the
   reference's behaviour (defensibility.rs:32-73 runs before the model is fit). Then, as ob_remedy_run with the
   Reference target: the builder's design, one upload of the stacked rows, the Gram over A, ob_remedy_solve, the
   score pass, sigma_squared = rss_A / (n_A - K) (0 when n_A = K), and ob_remedy_defend_rows' passes. No point
   estimate is run: original_gap is the difference of the group means, as in the reference.
   An adjustment whose index is outside [0, n_rows) is skipped and counted in n_skipped, not an error (:200, the
   map lookup fails); the handle holds one entry per kept adjustment in request order, with the model behind
   ob_remedy_results_model (contributions on request).
   Errors before any device work, in this order: NULL cfg or arrays and negative counts are OB_E_INVALID; m >=
   2^31 - 1 OB_E_UNSUPPORTED; ob_remedy_run's frame checks in its order (missing column, null, non-finite outcome,
   group dtype, two groups, column count); a non-finite value or override value, or an override position outside
   [0, m), is OB_E_INVALID; a NULL ctx or out comes last. A null in a named column stays OB_E_INVALID even where
   an override would fill it (the reference would take the override). */
int ob_remedy_defend(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                     const int64_t* index, const double* value, int64_t m, const int64_t* override_adjustment,
                     const char* const* override_name, const double* override_value, int64_t n_overrides,
                     double confidence_level, int32_t contributions, ob_remedy_results** out);
/* defensibility.rs:32-73 on the host (needs no GPU): per original index the LAST adjustment that carries any
   override replaces every earlier set for that index as a whole (HashMap::insert of the row's map; within one
   set a name given twice keeps its last value); then only names among predictors[n_predictors] and indices below
   n_rows take effect. Writes the cells to change, predictor by predictor and by ascending row: out_row,
   out_predictor (a position in predictors) and out_value hold up to n_overrides entries, *n_out of them filled. */
int ob_remedy_resolve_overrides(const int64_t* index, int64_t m, const int64_t* override_adjustment,
                                const char* const* override_name, const double* override_value, int64_t n_overrides,
                                const char* const* predictors, int32_t n_predictors, int64_t n_rows, int64_t* out_row,
                                int32_t* out_predictor, double* out_value, int64_t* n_out);
/* is_defensible per returned adjustment (1 / 0), owned by r; NULL for a handle of ob_remedy_run or _allocate. */
int ob_remedy_results_defensible(const ob_remedy_results* r, const int32_t** is_defensible);
/* OB_E_INVALID for a handle that is not ob_remedy_defend's or ob_remedy_defend_rows'. */
int ob_remedy_results_defend_info(const ob_remedy_results* r, ob_defend_info* out);
/* analysis.rs:76-88 on the host (needs no GPU): out[n_rows] = wage with out[index[j]] += value[j] applied one by
   one in request order, so two raises of one row give (w + a1) + a2. valid (may be NULL): 0 marks a null wage,
   which no raise touches. An index outside [0, n_rows) is OB_E_INVALID "Adjustment index <i> is out of bounds
   (dataset has <n> rows)", a non-finite value OB_E_INVALID, whichever comes first in request order. */
int ob_remedy_apply_adjustments(const double* wage, const uint8_t* valid, int64_t n_rows, const int64_t* index,
                                const double* value, int64_t m, double* out);
/* verify_inner: ob_remedy_apply_adjustments on a copy of the outcome column (OB_COL_I64 is cast to f64, a string
   column is OB_E_POLARS, a missing one OB_E_COLUMN "Column '<name>' not found in dataset."), then ob_builder_run
   with the caller's configuration as it stands (reference coefficients, replicates, seed, weights,
   normalisation) and its ordinary handle. The argument errors come before any device work; a NULL ctx or out is
   OB_E_INVALID after them. The reference's `quantile` switch (Machado-Mata) is not built. */
int ob_remedy_verify(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                     const int64_t* index, const double* value, int64_t m, ob_results** out);

/* ---- Jackknife influence pass and BCa bootstrap intervals (no reference counterpart: inference.rs:21-31 has
 * floor-index percentile intervals only) ----------------------------------------------------------------
 * The bias-corrected and accelerated interval needs the leave-one-out value theta_(i) of every component for
 * every row. In closed form (Sherman-Morrison on the group's Gram) that is one streaming pass over the panel in
 * HBM: per row of group g, t = G_g^-1 x on the f64 matrix units, h = w x't, e = y - x'beta_g, beta_g(i) =
 * beta_g - t w e / (1 - h), the means (S_g - w x) / (W_g - w) (w = 1, W_g = n_g without weights), for Pooled /
 * Neumark the same update of the pooled fit on [x, 1[g = A]] and for Weighted / Cotton the weights from W_g - w;
 * the other group stays at its point estimate. The C = 6 + 2 K components are the first C columns of a
 * replicate row (OB_ROW_EXPLAINED .. OB_ROW_TOTAL_GAP, detailed explained, detailed unexplained).
 * A row is DROPPED, and counted per group, when the fit without it has no solution: 1 - h <= 2^-40 (for Pooled
 * also 1 - h^P <= 2^-40) or W_g - w <= 0; this mirrors the reference dropping a replicate whose Cholesky fails.
 * Sums are f64 in a fixed order (per-wave slots, ob_ordered_sum; no floating atomics), so a repeated call
 * returns the same bytes.
 * Limits, each OB_E_UNSUPPORTED before any device work: Heckman panels, n_norm > 0, n_y > 1, K >
 * OB_JACK_MAX_K, the rows output above 2^24 rows. A group with n_g <= K + 1 is OB_E_INSUFFICIENT; a Cholesky
 * failure of the point fit OB_E_LINALG. */
#define OB_JACK_MAX_K 119 /* design columns, the intercept included: the pooled design's 120 fits the LDS shape */
/* The limits above on their own (host only, needs no GPU): k design columns with the intercept; want_rows: the
   rows output is asked for. Every jackknife entry point makes exactly these checks first. */
int ob_jackknife_check_shape(int32_t k, int64_t n_a, int64_t n_b, int32_t n_norm, int32_t n_y, int32_t heckman,
                             int32_t want_rows);
typedef struct {
  int32_t capacity;     /* in: components the caller's arrays hold; at least 6 + 2 ob_panel_k(panel) */
  int32_t n_components; /* out: C */
  int64_t n_used[2];    /* out: kept rows of A and of B */
  int64_t n_dropped[2];
  double* point;        /* caller's, [C]: the point estimate's components */
  double* sums;         /* caller's, [2][C][3]: sum d, sum d^2, sum d^3 of d = theta_(i) - theta_hat per group */
  double* stats;        /* caller's, [C][3]: accel, jack_se, jack_bias (ob_jackknife_finish) */
} ob_jackknife_out;
/* The production path: the power sums and the statistics; nothing of size n x C is stored. */
int ob_jackknife(ob_panel* panel, int ref_mode, ob_jackknife_out* out);
/* For tests and small panels: theta[(n_a + n_b) x C] row-major, A's rows first, and kept[n_a + n_b] (a dropped
   row's theta is NaN). n_dropped[2] may be NULL. */
int ob_jackknife_rows(ob_panel* panel, int ref_mode, double* theta, uint8_t* kept, int64_t* n_dropped);
/* The calling thread's last ob_jackknife / ob_jackknife_rows (or a builder entry that ran one): HIP-event ms of
   the pass with its reduce. */
int ob_jackknife_last_timing(double* pass_ms);
/* Host only. With m_g the kept rows of group g, dbar_g = sum d / m_g, U2_g = sum d^2 - m_g dbar_g^2 and U3_g =
   -(sum d^3 - 3 dbar_g sum d^2 + 2 m_g dbar_g^3) (the power sums of u_gi = thetabar_g - theta_g(i)):
   stats[c] = {accel = sum_g U3_g / (6 (sum_g U2_g)^1.5) or 0 where the denominator is 0,
               jack_se = sqrt(sum_g (m_g - 1) / m_g U2_g), jack_bias = sum_g (m_g - 1) dbar_g}.
   sums: [2][n_components][3]; a group with m_g = 0 adds nothing. */
int ob_jackknife_finish(const double* sums, const int64_t* n_used, int32_t n_components, double* stats);
/* The BCa interval of n replicate values. p0 = (#{v < point} + #{v = point} / 2) / n, z0 =
   ob_normal_inverse_cdf(p0); for alpha in {(1 - level) / 2, 1 - (1 - level) / 2}: q = z0 +
   ob_normal_inverse_cdf(alpha), alpha' = Phi(z0 + q / (1 - accel q)) with Phi(z) = erfc(-z / sqrt 2) / 2, endpoint
   sorted[min(floor(alpha' n), n - 1)] (the index convention of inference.rs:25-31). out = {ci_lower, ci_upper,
   z0, alpha'_lo, alpha'_hi, flag}; flag != 0 with NaN endpoints when n = 0 (1), p0 is 0 or 1 (2), accel is not
   finite (3) or 1 - accel q <= 0 (4). level outside (0, 1) is OB_E_INVALID. Host only. */
int ob_bca_stats(const double* estimates, int64_t n, double point_estimate, double accel, double level, double out[6]);
/* ob_aggregate with one point estimate and one accel per column: out is n_cols x the six values above. */
int ob_aggregate_bca(const double* rows, const uint8_t* ok, uint64_t n_reps, int32_t row_len, const int32_t* cols,
                     int32_t n_cols, const double* point, const double* accel, double level, double* out);
/* ob_jackknife on the prepared panel with its reference coefficients; the result is kept in the handle. */
int ob_prepared_jackknife(ob_prepared* prep, ob_jackknife_out* out);
/* ob_prepared_finish with ci_lower / ci_upper of every component replaced by the BCa endpoints at `level`
   (estimate, std_err, t_stat and p_value are untouched). Runs ob_prepared_jackknife if the handle has none yet.
   It reads only the aggregated columns, so rows of any boot serve, sharded ones included. A component that
   pools several row columns (a repeated name) takes the accel of its own column. */
int ob_prepared_finish_bca(ob_prepared* prep, const double* rows, const uint8_t* ok, uint64_t n_reps, double level,
                           ob_results** out);
/* ob_builder_run with BCa intervals: prepare + every replicate + the jackknife pass + ob_prepared_finish_bca. */
int ob_builder_run_bca(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                       const ob_builder_config* cfg, double level, ob_results** out);
/* out[5] = {accel, jack_se, jack_bias, z0, flag} of component i of a table of such a result. OB_E_INVALID on a
   result without a jackknife (ob_prepared_finish, ob_builder_run) or for OB_TABLE_DETAILED_SELECTION. */
int ob_results_jackknife(const ob_results* r, int32_t table, int32_t i, double* out);

/* ---- Cluster bootstrap (no reference counterpart: builder.rs:822-827 resamples rows) -------------------
 * The row bootstrap assumes independent rows within a group. For panels whose rows are nested in clusters
 * (workers with repeated observations, employees in firms) a replicate resamples whole clusters instead, the
 * counterpart of Stata's `bootstrap, cluster()`. The extended Gram is linear in the cluster counts,
 *     G_r[g] = sum_c k[r][c] Q[c][g],   Q[c][g] = sum over the rows i of cluster c in group g of v_i v_i',
 * with v_i the engine's row vector (sqrt(w) [1, x, y] weighted, [1, x, y] otherwise). One pass forms Q
 * (ob_cluster_gram), an exact multinomial draws k (ob_cluster_counts, the OBRC-1 stream of ob_spec.h) and an
 * f64 GEMM forms counts x Q (ob_cluster_apply) in the [rep][2][e_pad] layout the solve reads, together with
 * each replicate's row count per group; beta, beta*, normalization, the row layout, ob_prepared_finish and
 * ob_aggregate are the row bootstrap's. The point estimate does not change. A replicate in which a group
 * has rows <= K is dropped (ok = 0, the reference's InsufficientData).
 * Cluster ids: after clean_dataframe (a null in the cluster column drops the row) and the group split, the
 * column's values over the rows of groups A and B become dense ids 0 .. C-1 in order of first appearance.
 * The column is a string or an integer column; a float column is OB_E_INVALID.
 * Modes: joint (stratified = 0): one multinomial of C draws over all C clusters, shared by both groups.
 * stratified: C_A draws over A's clusters and C_B over B's, independently; every cluster must lie in exactly
 * one group (OB_E_INVALID naming the first that does not) and A's clusters are renumbered to [0, C_A).
 * Every sum is f64 in a fixed order that depends on the cluster sizes and on C alone: a replicate's row has
 * the same bytes alone, in any batch and at any first_rep.
 * Limits, each before any device work: C < 2 OB_E_INSUFFICIENT; C >= 2^24, or Q above 8 GiB
 * (C * 2 * (e_pad + 1) doubles): OB_E_UNSUPPORTED; Heckman selection, ob_prepared_boot_sharded,
 * ob_prepared_jackknife, ob_prepared_finish_bca on a clustered handle: OB_E_UNSUPPORTED (delete-one-row is
 * the wrong jackknife under clustering; ob_prepared_cluster_jackknife, ob_prepared_finish_cluster_bca and
 * ob_builder_run_clustered_bca below are the delete-one-cluster forms). Machado-Mata has no clustered entry point. */
typedef struct {
  const char* column; /* the cluster id column */
  int32_t stratified; /* 0: joint, 1: stratified */
} ob_cluster_config;
typedef struct {
  int64_t n_clusters, n_clusters_a, n_clusters_b; /* C; clusters with rows in A / in B */
  int64_t max_cluster_rows;                       /* rows of the largest cluster (both groups together) */
  int32_t stratified;
} ob_cluster_info;
typedef struct {
  double gram_ms, counts_ms, apply_ms, solve_ms;
} ob_cluster_timing;
/* The size limits above on their own (host only): C clusters, k1 = P + 1 + n_y columns of v. */
int ob_cluster_check_shape(int64_t n_clusters, int32_t k1);
/* Host only. ids: one column over n_rows frame rows; group[r] = 0 (A), 1 (B), anything else: the row is in
   neither. A null id drops the row. dense[n_rows]: the row's cluster id or -1. perm_a / perm_b (as long as the
   groups' kept rows; n_rows each is always enough): the group's kept rows, as positions among them in frame
   order, sorted stably by cluster id. off_a / off_b [C + 1] (n_rows + 1 each is always enough): cluster c's
   rows of the group are perm[off[c] .. off[c + 1]). Any output may be NULL. */
int ob_cluster_index(const ob_column* ids, const int32_t* group, int64_t n_rows, int32_t stratified, int32_t* dense,
                     int64_t* perm_a, int64_t* perm_b, int64_t* off_a, int64_t* off_b, ob_cluster_info* info);
/* Q of one group: x (n x p, column-major, ldx), y[n], w[n] or NULL; perm[n] / off[C + 1] as above. q: [C][e_pad]
   with e_pad = 16 ceil(E / 16), E = (p + 2)(p + 3) / 2 pairs in ob_spec.h's order; rows[C]: the clusters' row
   counts. Rows go in permuted order in pieces of 256, the pieces are added in order. */
int ob_cluster_gram(ob_ctx* ctx, const double* x, int64_t n, int64_t ldx, int32_t p, const double* y, const double* w,
                    const int64_t* perm, const int64_t* off, int64_t n_clusters, double* q, uint32_t* rows);
/* counts[n_reps][C] (C = n_clusters_a + n_clusters_b) of replicates first_rep .. first_rep + n_reps - 1 from
   OBRC-1. Joint: C draws over [0, C). Stratified: n_clusters_a draws over [0, C_A), n_clusters_b over the rest. */
int ob_cluster_counts(ob_ctx* ctx, uint64_t seed, uint64_t first_rep, uint32_t n_reps, int64_t n_clusters_a,
                      int64_t n_clusters_b, int32_t stratified, uint32_t* counts);
/* out[n_reps][width] = counts[n_reps][C] (exact in f64) x q[C][width] on the f64 matrix units; width a multiple
   of 16. C is walked in cluster order in runs of 8192 whose partial sums are added in order. */
int ob_cluster_apply(ob_ctx* ctx, const uint32_t* counts, uint32_t n_reps, int64_t n_clusters, const double* q,
                     int32_t width, double* out);
/* The calling thread's last clustered boot (ob_prepared_boot, ob_builder_run_clustered): HIP-event ms. gram_ms is
   the one pass that forms Q, charged to the call that ran it. */
int ob_cluster_last_timing(ob_cluster_timing* out);
/* ob_builder_prepare / ob_builder_run / ob_builder_decompose_quantiles with the cluster bootstrap. A handle
   prepared this way routes ob_prepared_boot, ob_prepared_boot_device and ob_prepared_finish through it. */
int ob_builder_prepare_clustered(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                                 const ob_builder_config* cfg, const ob_cluster_config* ccfg, ob_prepared** out);
int ob_builder_run_clustered(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                             const ob_builder_config* cfg, const ob_cluster_config* ccfg, ob_results** out);
int ob_builder_decompose_quantiles_clustered(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                                             const ob_builder_config* cfg, const ob_cluster_config* ccfg,
                                             const double* taus, int32_t n_taus, ob_results** out);
/* C of the clustered run behind a result, -1 for a row bootstrap's. */
int64_t ob_results_n_clusters(const ob_results* r);
/* OB_E_INVALID on a handle that is not clustered. */
int ob_prepared_cluster_info(const ob_prepared* prep, ob_cluster_info* out);

/* ---- Delete-one-cluster jackknife and BCa intervals for clustered runs (the counterpart of
 * Stata's `jackknife, cluster()`) -----------------------------------------------------------------------
 * theta_(c), every component without cluster c, in closed form from what a clustered handle holds: with Q^xx_c,
 * b_c = sum w x y, S_c = sum w x, W_c = sum w of cluster c in group g, M = G_g - Q^xx_c and r_c = b_c - Q^xx_c beta_g,
 *     beta_g(c) - beta_g = -M^-1 r_c (one Cholesky of M per cluster and group),
 *     xbar_g(c) - xbar_g = (W_c xbar_g - S_c) / (W_g - W_c), the mean outcome likewise,
 * the same downdate of the pooled Gram for Pooled / Neumark and the Cotton weights from W_g - W_c (row counts
 * without weights). A group the cluster has no row in stays at the point estimate exactly. In joint mode the
 * strata are all C clusters (stratum 0), in stratified mode A's clusters and B's.
 * A cluster is DROPPED, and counted per stratum, when n_g - rows_c,g <= K for a group it touches (the
 * reference's InsufficientData), when W_g - W_c <= 0, or when a Cholesky pivot of M (for Pooled also of the
 * pooled downdate) is at most 2^-40 times the same pivot of the point estimate's factor. Fewer than 2 kept
 * clusters in a stratum that has any is OB_E_INSUFFICIENT.
 * Sums are f64 in a fixed order that depends on C alone (no floating atomics): a repeated call returns the same
 * bytes. It draws nothing from OBRC-1, so jack_se is an independent check of the cluster bootstrap's std_err.
 * Limits, each OB_E_UNSUPPORTED before any device work: K > OB_CLUSTER_JACK_MAX_K, normalized categoricals,
 * Heckman panels, more than one outcome. The delete-one-row entry points (ob_prepared_jackknife,
 * ob_prepared_finish_bca, ob_builder_run_bca) keep refusing a clustered handle; these are their clustered forms. */
#define OB_CLUSTER_JACK_MAX_K 32 /* design columns, the intercept included */
/* The limits above on their own (host only): k design columns with the intercept, C clusters (C < 2 is
   OB_E_INSUFFICIENT). Every entry point below makes exactly these checks first. */
int ob_cluster_jackknife_check_shape(int32_t k, int64_t n_clusters, int32_t n_norm, int32_t n_y, int32_t heckman,
                                     int32_t want_rows);
/* The production path over a clustered handle: the power sums of d = theta_(c) - theta_hat per stratum and
   ob_jackknife_finish's statistics (n_used / n_dropped / sums are per stratum; joint mode leaves stratum 1
   empty). The result is kept in the handle. OB_E_INVALID on a handle that is not clustered. */
int ob_prepared_cluster_jackknife(ob_prepared* prep, ob_jackknife_out* out);
/* For tests and inspection: theta[C x ob_prepared_row_len(prep)] row-major, cluster c's replicate-shaped row
   from the solve kernel itself on T_g - Q[c][g] (T_g = sum_c Q[c][g] in ob_cluster_apply's order; a group the
   cluster has no row in takes the point estimate's Gram): the first 6 + 2 K columns are the components, then
   beta_A, beta_B, xbar_A, xbar_B, beta*. kept[C]; a dropped cluster's row is NaN. n_dropped[2] (per stratum)
   may be NULL. deviations (may be NULL): [C x (6 + 2 K)], every cluster's d = theta_(c) - theta_hat exactly as the
   production path forms and sums it (NaN where that path drops the cluster). The same clusters are dropped as
   on the production path; no statistics are formed here, so a stratum with fewer than 2 kept clusters is not an
   error of this call. Rows go back to the host batch by batch: no more than 1 GiB of device memory beside Q. */
int ob_prepared_cluster_jackknife_rows(ob_prepared* prep, double* theta, uint8_t* kept, int64_t* n_dropped,
                                       double* deviations);
/* The same two passes on arrays. q: [C][2][e_pad], cluster c's Q of group A then of group B as ob_cluster_gram
   returns them per group (e_pad = 16 ceil((p + 2)(p + 3) / 32)); rows: [C][2] their row counts; n_clusters_a: A's
   clusters, which come first when stratified != 0. ob_cluster_jackknife needs no panel: gram is the point
   estimate's two extended Grams [2][e_pad] (the sum of q over the clusters serves), tail its beta_A, beta_B,
   xbar_A, xbar_B, beta* (5 (p + 1) values; for Pooled / Neumark beta* is recomputed from gram), n_a / n_b the
   groups' rows, weighted != 0 when the Grams carry weights; out->point is theta_hat recomputed from these.
   ob_cluster_jackknife_rows takes the point estimate and the solve kernel from a resident panel. Both make
   ob_cluster_jackknife_check_shape's checks and ob_cluster_check_shape's first. */
int ob_cluster_jackknife(ob_ctx* ctx, const double* q, const uint32_t* rows, int64_t n_clusters, int64_t n_clusters_a,
                         int32_t stratified, int32_t p, int32_t weighted, int64_t n_a, int64_t n_b, const double* gram,
                         const double* tail, int ref_mode, ob_jackknife_out* out);
int ob_cluster_jackknife_rows(ob_panel* panel, const double* q, const uint32_t* rows, int64_t n_clusters,
                              int64_t n_clusters_a, int32_t stratified, int ref_mode, double* theta, uint8_t* kept,
                              int64_t* n_dropped, double* deviations);
/* ob_prepared_finish with ci_lower / ci_upper of every component replaced by the BCa endpoints at `level`
   through ob_bca_stats with the delete-one-cluster accelerations (estimate, std_err, t_stat and p_value are
   untouched). Runs ob_prepared_cluster_jackknife if the handle has none yet. */
int ob_prepared_finish_cluster_bca(ob_prepared* prep, const double* rows, const uint8_t* ok, uint64_t n_reps,
                                   double level, ob_results** out);
/* ob_builder_run_clustered with BCa intervals: prepare + every replicate + the pass + the finish above.
   ob_results_jackknife serves its result. */
int ob_builder_run_clustered_bca(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                                 const ob_builder_config* cfg, const ob_cluster_config* ccfg, double level,
                                 ob_results** out);
/* The calling thread's last cluster jackknife pass: HIP-event ms of the kernel with its ordered sums. */
int ob_cluster_jackknife_last_timing(double* pass_ms);

/* ---- RIF decompositions of the variance, the Gini and quantile ranges -------------------
 * The recentred influence function of a distributional statistic as the outcome of the mean decomposition
 * (Firpo, Fortin, Lemieux 2009, 2018). For a group's outcome y of n rows, unweighted: mu = sum y / n,
 * r(i) = #{j : y_j <= y_i} (tied rows share the last rank of their run), p_i = r(i) / n.
 *   OB_RIF_VARIANCE  RIF_i = (y_i - mu)^2, statistic sum (y - mu)^2 / n.
 *   OB_RIF_GINI      GL_i = (1/n) sum_{y_j <= y_i} y_j, R = (1/n) sum GL_i, statistic G = 1 - 2R/mu,
 *                    RIF_i = 1 + (2R/mu^2) y_i - (2/mu) [y_i (1 - p_i) + GL_i]. y >= 0 and mu > 0.
 *   OB_RIF_IQR       p0 = tau_hi, p1 = tau_lo, 0 < tau_lo < tau_hi < 1: RIF_{tau_hi} - RIF_{tau_lo}, each ob_rif's
 *                    (type-7 quantile, its Silverman bandwidth and fallbacks, Gaussian density, floor 1e-8,
 *                    indicator y <= q); one sort and one bandwidth serve both. Statistic q_hi - q_lo.
 * Device pass: a stable radix sort of (y, row), tie runs and ranks, block scans of ob_rif_scan_block() sorted
 * values with the block totals scanned in block order, sums in pieces of that size added in order, the two
 * densities over chunks of the sorted values, a scatter to row order. Every sum is f64 in an order that depends
 * on n alone: a repeated call, or the same values in another row order, gives the same bytes per row.
 * Errors, each before any device work (a NULL ctx with good arguments is OB_E_INVALID "null pointer"): an unknown
 * statistic or bad tau OB_E_INVALID; n < 2 OB_E_INSUFFICIENT; n > 2^28 OB_E_UNSUPPORTED; a non-finite y
 * OB_E_INVALID; for the Gini a negative y or no positive one OB_E_INVALID. */
#define OB_RIF_VARIANCE 0
#define OB_RIF_GINI 1
#define OB_RIF_IQR 2
#define OB_RIF_QUANTILE 3 /* p0 = tau; the weighted entry points only */
typedef struct {
  int32_t stat;  /* OB_RIF_* */
  double p0, p1; /* OB_RIF_IQR: tau_hi, tau_lo; OB_RIF_QUANTILE: tau, unused; otherwise unused */
} ob_rif_spec;
typedef struct {
  double sort_ms, scan_ms, kde_ms, scatter_ms; /* kde_ms: the quantile pieces and densities of OB_RIF_IQR */
} ob_rif_timing;
/* rif_out[n] in y's row order, *statistic_out the statistic itself. */
int ob_rif_stat(ob_ctx* ctx, const double* y, int64_t n, const ob_rif_spec* spec, double* rif_out,
                double* statistic_out);
/* Sorted values per scan block and per piece of the ordered sums (a constant of the kernels). */
int32_t ob_rif_scan_block(void);
/* HIP-event ms of the calling thread's last ob_rif_stat / ob_builder_decompose_statistics (groups and statistics
   added up). */
int ob_rif_last_timing(ob_rif_timing* out);
/* One panel whose outcomes are the n_specs RIF columns of each group's outcome, built exactly as
   ob_builder_decompose_quantiles builds its panel: one resample and one Gram per replicate serve all of them, the
   same cap on outcomes applies, and out[t] is bitwise the single-statistic call. */
int ob_builder_decompose_statistics(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                                    const ob_builder_config* cfg, const ob_rif_spec* specs, int32_t n_specs,
                                    ob_results** out);
int ob_builder_decompose_statistics_clustered(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                                              const ob_builder_config* cfg, const ob_cluster_config* ccfg,
                                              const ob_rif_spec* specs, int32_t n_specs, ob_results** out);

/* ---- Decomposition of a gap in a 0/1 outcome: bootstrapped probit Oaxaca-Blinder -------------
 * The nonlinear decomposition of Fairlie (1999), Yun (2004) and Bauer-Sinning (2008). No counterpart in the
 * reference crate. X = [1, x_1..x_p], K = p + 1 <= OB_BINARY_MAX_K columns; Phi the standard normal cdf; c the
 * replicate's OBRS-3 counts (every row once in the point pass); n_g = sum c;
 *     Pbar(g, beta) = (1 / n_g) sum_{i in g} c_i Phi(x_i' beta).
 * beta_A, beta_B: the probit of y on X per group, by ob_probit's iteration (Fisher scoring from 0, the 1e-9
 * ridge, Phi clamped to [1e-10, 1 - 1e-10], 100 iterations, tol 1e-6). beta*: the group's own for
 * OB_REF_GROUP_A / OB_REF_GROUP_B, the row-share average wA beta_A + (1 - wA) beta_B, wA = n_A / (n_A + n_B),
 * for OB_REF_WEIGHTED / OB_REF_COTTON; OB_REF_POOLED / OB_REF_NEUMARK are OB_E_UNSUPPORTED.
 *     total_gap    = Pbar(A, beta_A) - Pbar(B, beta_B)
 *     explained    E = Pbar(A, beta*) - Pbar(B, beta*),  unexplained U = total_gap - E = U_A + U_B,
 *                  U_A = Pbar(A, beta_A) - Pbar(A, beta*), U_B = Pbar(B, beta*) - Pbar(B, beta_B)
 *     endowments   = Pbar(A, beta_B) - Pbar(B, beta_B),  coefficients = Pbar(B, beta_A) - Pbar(B, beta_B),
 *     interaction  = total_gap - endowments - coefficients
 *     explained_k   = E (xbar_A^k - xbar_B^k) beta*^k / sum_j (xbar_A^j - xbar_B^j) beta*^j      (Yun's weights)
 *     unexplained_k = U_A xbar_A^k (beta_A^k - beta*^k) / sum_j xbar_A^j (beta_A^j - beta*^j)
 *                   + U_B xbar_B^k (beta*^k - beta_B^k) / sum_j xbar_B^j (beta*^j - beta_B^j)
 * with xbar_g the replicate's count-weighted column means; a part whose denominator is exactly 0 contributes 0.0.
 * Row of a replicate, ob_binary_row_len(K) = 6 + 7K + 8 doubles:
 *     [0, 6)  explained, unexplained, endowments, coefficients, interaction, total_gap
 *     K explained_k | K unexplained_k | beta_A, beta_B, xbar_A, xbar_B, beta* (K each)
 *     Pbar(A,beta_A), Pbar(A,beta_B), Pbar(A,beta*), Pbar(B,beta_A), Pbar(B,beta_B), Pbar(B,beta*) | ybar_A, ybar_B
 * A replicate whose probit cannot solve its Hessian in either group has ok = 0 and is dropped and counted by
 * ob_prepared_finish; a point pass that fails so is OB_E_LINALG. Every sum is f64 in chunk order without atomics:
 * a replicate's row has the same bytes alone, in any batch and at any first_rep.
 * Errors of the frame entry points, all before any device work and before the context is read: model
 * OB_BINARY_LOGIT, weights, normalize, Heckman settings, Pooled / Neumark: OB_E_UNSUPPORTED; a null in a named
 * column: OB_E_INVALID; K > OB_BINARY_MAX_K: OB_E_UNSUPPORTED; an outcome value other than exactly 0.0 or 1.0, or a
 * group whose outcome is constant: OB_E_INVALID; a group with rows <= K: OB_E_INSUFFICIENT. On a handle prepared
 * here ob_prepared_boot, ob_prepared_boot_device (which synchronizes its stream) and ob_prepared_finish work;
 * ob_prepared_boot_sharded, ob_prepared_jackknife and ob_prepared_finish_bca are OB_E_UNSUPPORTED. */
#define OB_BINARY_MAX_K 32
#define OB_BINARY_PROBIT 0
#define OB_BINARY_LOGIT 1 /* OB_E_UNSUPPORTED: the per-replicate fit kernels are probit's */
typedef struct {
  double probit_ms;          /* the probit passes, summed over iterations and batches */
  int32_t probit_launches;
  int32_t probit_iterations; /* the longest batch's */
  double means_ms;           /* the mean-probability pass */
  double epilogue_ms;        /* the per-replicate rows */
} ob_binary_timing;
int ob_binary_row_len(int32_t k);
/* The shape limits above on their own (host only). */
int ob_binary_check_shape(int32_t k, int64_t n_a, int64_t n_b);
/* The mean-probability pass alone over one group: x (n x k, column-major, ldx >= n, column 0 all ones), y, counts
   (n bytes, or NULL for every row once), betas [3][k]. out[5 + k]: Pbar(beta_0), Pbar(beta_1), Pbar(beta_2), ybar,
   sum c, xbar_0 .. xbar_{k-1}. */
int ob_binary_means(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, int64_t n, int32_t k,
                    const uint8_t* counts, const double* betas, double* out);
/* HIP-event ms of the calling thread's last binary boot (or prepare: the point pass). */
int ob_binary_last_timing(ob_binary_timing* out);
int ob_builder_prepare_binary(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                              const ob_builder_config* cfg, int32_t model, ob_prepared** out);
/* prepare + cfg->bootstrap_reps replicates + finish. The tables are ob_builder_run's; total_gap is the predicted gap. */
int ob_builder_run_binary(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                          const ob_builder_config* cfg, int32_t model, ob_results** out);
/* The point-estimate row of a prepared run (any kind), owned by the handle. */
int ob_prepared_point_row(const ob_prepared* prep, const double** data, int64_t* len);

/* ---- Reweighted Oaxaca-Blinder decomposition with a bootstrapped propensity logit -------------
 * Fortin, Lemieux and Firpo (2011), section 5; Stata's `oaxaca_rif ..., rwlogit()`. No counterpart in the reference
 * crate (dfl.rs stops at densities). A is the non-reference group, B cfg->reference_group; x the design row with the
 * intercept (K <= OB_REWEIGHT_MAX_K columns, the builder's dummies included); w the sample weight (1 without
 * cfg->weights); c the replicate's OBRS-3 count of the row (1 in the point pass).
 *   Propensity: the logit of D = 1[A] on x over the stacked rows of A and B, each row's log-likelihood term times
 *   c w, by the Newton iteration of math/logit.rs:31-118: gamma from 0, p clamped to [1e-10, 1 - 1e-10], the
 *   information matrix sum c w p (1 - p) x x' solved by Cholesky, stop when ||step||_2 < 1e-6, at most 100 passes.
 *   Weights: psi = p / (1 - p) with the clamped p. The factor P(B) / P(A) of dfl.rs:116 is left out: every quantity
 *   below is a ratio of psi-weighted sums, in which it cancels.
 *   Fits, each the Cholesky solve of the weighted extended Gram: (beta_A, xbar_A, ybar_A) on A's rows with weights
 *   c w; (beta_B, xbar_B, ybar_B) on B's rows with c w; (beta_C, xbar_C, ybar_C) on B's rows with c w psi -- the
 *   counterfactual sample C. cfg->reference_coeffs is ignored: the decomposition defines its own three fits.
 *     total_gap           = ybar_A - ybar_B
 *     composition         = xbar_C . beta_C - xbar_B . beta_B      structure         = xbar_A . beta_A - xbar_C . beta_C
 *     pure_explained      = (xbar_C - xbar_B) . beta_B             pure_unexplained  = xbar_A . (beta_A - beta_C)
 *     specification_error = xbar_C . (beta_C - beta_B)             reweighting_error = (xbar_A - xbar_C) . beta_C
 * Row of a replicate, ob_reweight_row_len(K) = 7 + 11 K + 5 doubles:
 *     [0, 7)  total_gap, composition, structure, pure_explained, specification_error, pure_unexplained,
 *             reweighting_error (OB_RW_ROW_*)
 *     K pure_explained_k | K specification_error_k | K pure_unexplained_k | K reweighting_error_k (the summands)
 *     beta_A, beta_B, beta_C, xbar_A, xbar_B, xbar_C, gamma (K each)
 *     ybar_A, ybar_B, ybar_C | the effective sample size of psi on B, (sum c w psi)^2 / sum c (w psi)^2 | the
 *     logit's pass count
 * A replicate whose logit does not converge within 100 passes, whose information matrix has no Cholesky factor
 * (separation is the usual cause) or one of whose three fits fails has ok = 0 and a NaN row; ob_prepared_finish drops
 * and counts it. A point pass that fails so is OB_E_LINALG "Failed to solve Information Matrix in Logit. Perfect
 * separation?", ob_dfl_run's error. Every sum is f64 in chunk order without atomics: a replicate's row has the same
 * bytes alone, in any batch and at any first_rep. Option "hk_batch" caps a batch at n 64-replicate blocks (default:
 * as many as keep the chunk partials within 1 GiB).
 * Errors of the frame entry points, all before any device work and before the context is read: normalize, Heckman
 * settings: OB_E_UNSUPPORTED; a null or a non-finite value in a named column: OB_E_INVALID; K > OB_REWEIGHT_MAX_K:
 * OB_E_UNSUPPORTED; a group with rows <= K: OB_E_INSUFFICIENT. One outcome; the cluster bootstrap is not served (the
 * clustered entry points have no reweighted form). On a handle prepared here ob_prepared_boot,
 * ob_prepared_boot_device (which synchronizes its stream), ob_prepared_finish and ob_prepared_point_row work;
 * ob_prepared_boot_sharded, ob_prepared_jackknife and ob_prepared_finish_bca are OB_E_UNSUPPORTED.
 * Results of ob_prepared_finish / ob_builder_run_reweighted: the tables OB_RW_TABLE_* (estimate, standard error,
 * percentile interval and p over the replicates kept), ob_results_total_gap; OB_VEC_XA_MEAN, OB_VEC_XB_MEAN and
 * OB_VEC_BETA_STAR hold xbar_A, xbar_B and beta_C; the rest of the point row is ob_prepared_point_row's. */
#define OB_REWEIGHT_MAX_K 32
#define OB_RW_ROW_TOTAL_GAP 0
#define OB_RW_ROW_COMPOSITION 1
#define OB_RW_ROW_STRUCTURE 2
#define OB_RW_ROW_PURE_EXPLAINED 3
#define OB_RW_ROW_SPECIFICATION_ERROR 4
#define OB_RW_ROW_PURE_UNEXPLAINED 5
#define OB_RW_ROW_REWEIGHTING_ERROR 6
#define OB_RW_ROW_DETAILED 7
#define OB_RW_TABLE_AGGREGATE 0 /* the seven aggregates, in row order */
#define OB_RW_TABLE_PURE_EXPLAINED 1
#define OB_RW_TABLE_SPECIFICATION_ERROR 2
#define OB_RW_TABLE_PURE_UNEXPLAINED 3
#define OB_RW_TABLE_REWEIGHTING_ERROR 4
typedef struct {
  int32_t logit_passes;   /* the longest batch's */
  int32_t logit_launches; /* pass kernels over all batches */
  double logit_ms;        /* the logit pass kernels (the Newton steps not included) */
  double gram_ms;         /* the three Grams' kernels */
  double row_ms;          /* the solves and rows */
} ob_reweight_timing;
int ob_reweight_row_len(int32_t k);
/* The shape limits above on their own (host only). */
int ob_reweight_check_shape(int32_t k, int64_t n_a, int64_t n_b);
/* HIP-event ms of the calling thread's last reweighted boot (or prepare: the point pass). */
int ob_reweight_last_timing(ob_reweight_timing* out);
/* One logit pass alone: x (n x k, column-major, ldx >= n, column 0 all ones), d (n values, each 0.0 or 1.0), w (n
   weights or NULL for 1), counts (n bytes or NULL for every row once), gammas [n_gammas][k] with n_gammas <= 64 (each
   is one replicate's coefficient vector over the same counts). info [n_gammas][k x k] (symmetric, both triangles):
   sum c w p (1 - p) x x'; grad [n_gammas][k]: sum c w (d - p) x. */
int ob_reweight_logit_pass(ob_ctx* ctx, const double* x, int64_t ldx, const double* d, const double* w,
                           const uint8_t* counts, int64_t n, int32_t k, const double* gammas, int32_t n_gammas,
                           double* info, double* grad);
/* The psi-weighted extended Gram alone over one group: v = [x_0 .. x_{k-1}, y], gram [n_gammas][(k + 1) x (k + 1)]
   (symmetric, both triangles) = sum c w psi v v' with psi = p / (1 - p) of the clamped p at gammas[g];
   ess_den [n_gammas] = sum c (w psi)^2. Arguments as ob_reweight_logit_pass. */
int ob_reweight_gram(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, const double* w,
                     const uint8_t* counts, int64_t n, int32_t k, const double* gammas, int32_t n_gammas, double* gram,
                     double* ess_den);
int ob_builder_prepare_reweighted(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                                  const ob_builder_config* cfg, ob_prepared** out);
/* prepare + cfg->bootstrap_reps replicates + finish. */
int ob_builder_run_reweighted(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                              const ob_builder_config* cfg, ob_results** out);

/* ---- Weighted RIF pass and the reweighted decomposition of a statistic ----------------------
 * Firpo, Fortin and Lemieux's method whole: reweight B to A's covariates, then RIF regressions in A, B and C.
 * Weighted RIF of y[n] with weights w >= 0, W = sum w > 0: wt_i = w_i n / W; the rows ordered by y, stable; S_i
 * the inclusive sum of wt up to the end of y_i's tie run; F_i = S_i / n; mu = sum wt y / n; Y(t), 0 < t <= n, the
 * sorted value at the first position whose run-end S >= t (the last value if rounding leaves t above the last S).
 *   OB_RIF_VARIANCE  RIF_i = (y_i - mu)^2, statistic sum wt (y - mu)^2 / n.
 *   OB_RIF_GINI      GL_i = (1/n) sum_{y_j <= y_i} wt_j y_j, R = (1/n) sum wt_i GL_i, statistic G = 1 - 2R/mu,
 *                    RIF_i = 1 + (2R/mu^2) y_i - (2/mu) [y_i (1 - F_i) + GL_i].
 *   OB_RIF_QUANTILE  ob_rif's with every order statistic read through Y: h = (n - 1) tau, lo = floor(h), f = h - lo,
 *                    q = Y(lo + 1) + f (Y(min(lo + 2, n)) - Y(lo + 1)); sd = sqrt(sum wt (y - mu)^2 / (n - 1)); the
 *                    quartiles Y(min(max(ceil(p n), 1), n)); ob_rif's fallbacks and bandwidth 0.9 spread n^-0.2 with n
 *                    the row count; density sum wt phi((q - y) / bw) / (n bw), floor 1e-8;
 *                    RIF_i = q + (tau - 1[y_i <= q]) / density. Statistic q.
 *   OB_RIF_IQR       the difference of two such quantiles on one bandwidth.
 * At w = 1 these are the unweighted definitions above. Every sum is f64 in an order that depends on n alone and
 * runs over the sorted rows (W included): a repeated call gives the same bytes, weights scaled by a power of two
 * give the same bytes, and on distinct y a permutation of the rows gives the same statistic bytes. Inside a tie
 * run the rows keep their input order, so with unequal weights there a permutation moves last bits.
 * Errors, each before any device work and before the context is read: a bad spec OB_E_INVALID; n < 2
 * OB_E_INSUFFICIENT; n > 2^28 OB_E_UNSUPPORTED; a non-finite y or w, a negative w, W = 0 OB_E_INVALID; for the Gini
 * a negative y or no positive one among the rows with w > 0 OB_E_INVALID. ob_rif_stat and
 * ob_builder_decompose_statistics keep refusing OB_RIF_QUANTILE. */
int ob_rif_stat_weighted(ob_ctx* ctx, const double* y, const double* w, int64_t n, const ob_rif_spec* spec,
                         double* rif_out, double* statistic_out);
/* The reweighted decomposition above with the statistic's RIF as the outcome: after the point logit, the weighted RIF
 * of A's outcome (weights w), of B's (w) and of B's under w psi-hat (the counterfactual sample C) replace y in the
 * fits of A, B and C. Everything else is ob_builder_prepare_reweighted's: the counts, the per-replicate logit, the
 * three Grams, the solves, the row of ob_reweight_row_len(K) doubles, the refusals, and what works on the handle.
 * The RIFs are fixed at the point estimate: a replicate refits the logit and the three regressions but does not
 * recompute the statistic (as the quantile path of ob_builder_decompose_quantiles does not). The row's ybar entries
 * are the weighted means of the RIFs; the statistics themselves come from ob_prepared_reweight_statistics. */
int ob_builder_prepare_reweighted_statistic(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                                            const ob_builder_config* cfg, const ob_rif_spec* spec, ob_prepared** out);
/* out = nu_A, nu_B, nu_C. OB_E_INVALID on a handle of the mean (or of another kind). */
int ob_prepared_reweight_statistics(const ob_prepared* prep, double out[3]);
#define OB_REWEIGHT_MAX_STATS 16
/* Several statistics in one run: one resample and one logit fit per replicate serve all of them; out[t] is bitwise
   the single-statistic run (prepare + cfg->bootstrap_reps replicates + finish) with the same seed. n_specs >
   OB_REWEIGHT_MAX_STATS is OB_E_UNSUPPORTED. */
int ob_builder_run_reweighted_statistics(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                                         const ob_builder_config* cfg, const ob_rif_spec* specs, int32_t n_specs,
                                         ob_results** out);

/* ---- Distribution-regression decomposition of quantile gaps ------------------------------------
 * Chernozhukov, Fernandez-Val and Melly (2013), "Inference on counterfactual distributions"; Stata's `cdeco` /
 * `counterfactual`, R's `Counterfactual`. No counterpart in the reference crate. A is the non-reference group, B
 * cfg->reference_group; x the design row with the intercept in column 0 (K <= OB_DR_MAX_K columns); w the sample
 * weight (1 without cfg->weights); c the replicate's OBRS-3 count of the row (1 in the point pass).
 *   Thresholds c_1 < .. < c_T, 2 <= T <= OB_DR_MAX_T: given, or (ob_dr_config.thresholds == NULL) n_thresholds
 *   unweighted sample quantiles of the pooled outcome (A's rows then B's) at the levels lo + (hi - lo) t / (n - 1),
 *   t = 0 .. n - 1, by ob_rif's linear interpolation: h = (N - 1) level, s[floor h] + (h - floor h) (s[ceil h] -
 *   s[floor h]) on the sorted outcome. Exact duplicates are removed and the number kept is T. The thresholds are
 *   fixed at prepare time: a replicate does not move them.
 *   Fits: for g in {A, B} and each t the logit of d = 1[y <= c_t] on x over g's rows with weights c w, by Newton
 *   from beta = 0: p clamped to [1e-10, 1 - 1e-10], the information matrix sum c w p (1 - p) x x' solved by
 *   Cholesky (ob::chol_factor's operation order), converged when ||step||_2 < 1e-6, at most 100 passes. Every fit
 *   has its own done flag: once converged no later pass touches it.
 *   Distributions: F_jg(c_t) = sum_{i in j} c_i w_i L(x_i' beta_{g,t}) / sum_{i in j} c_i w_i with the same clamped
 *   sigmoid L, for (j, g) = AA, BB, AB and BA. F_C := F_AB, A's covariates with B's coefficients (the reading of C
 *   of the reweighted decomposition above); BA is reported and not decomposed.
 *   Distribution effects at every threshold: total = F_AA - F_BB, composition = F_C - F_BB, structure = F_AA - F_C.
 *   Quantile effects: each of F_AA, F_BB and F_C is rearranged (sorted ascending over t) into F~. For each tau,
 *   t* = min{t : F~_t >= tau} and Q = c_{t*-1} + (tau - F~_{t*-1}) (c_{t*} - c_{t*-1}) / (F~_{t*} - F~_{t*-1});
 *   Q = c_1 if t* = 1 and Q = c_T if tau > F~_T (the two edge cases). total(tau) = Q_A - Q_B, composition(tau) =
 *   Q_C - Q_B, structure(tau) = Q_A - Q_C.
 * Row of a replicate, ob_dr_row_len(T, n_q) = 6 n_q + 7 T + 1 doubles:
 *     [3][n_q] quantile effects total, composition, structure | [3][n_q] quantiles Q_A, Q_B, Q_C |
 *     [3][T] distribution effects total, composition, structure | [4][T] F_AA, F_BB, F_AB, F_BA (not rearranged) |
 *     the largest pass count among the replicate's 2 T fits.
 * A replicate one of whose fits does not converge or has no Cholesky factor has ok = 0 and a NaN row, which
 * ob_prepared_finish drops and counts; in the point pass that is OB_E_LINALG for the whole call (a threshold that
 * nobody or everybody of a group lies under is one way it happens). Every sum is f64 in chunk order without
 * floating-point atomics: a replicate's row has the same bytes alone, in any batch and at any first_rep. Option
 * "hk_batch" caps a batch at n 64-replicate blocks (default: as many replicates as keep the chunk partials within
 * 1 GiB).
 * Errors of the frame entry points, all before any device work and before the context is read: normalize, Heckman
 * settings, K > OB_DR_MAX_K, more than OB_DR_MAX_T thresholds, more than OB_DR_MAX_Q quantiles: OB_E_UNSUPPORTED;
 * a null or non-finite value in a named column, thresholds that are not finite and strictly increasing, fewer than
 * two thresholds, a tau outside (0, 1), no quantile: OB_E_INVALID; a group with rows <= K: OB_E_INSUFFICIENT.
 * cfg->reference_coeffs is ignored. The cluster bootstrap is not served. On a handle prepared here ob_prepared_boot,
 * ob_prepared_boot_device, ob_prepared_finish and ob_prepared_point_row work; ob_prepared_boot_sharded,
 * ob_prepared_jackknife and ob_prepared_finish_bca are OB_E_UNSUPPORTED.
 * Results of ob_prepared_finish / ob_builder_run_dr: the tables OB_DR_TABLE_* in row order, every component through
 * the aggregation of the other runs (estimate, standard error, percentile interval, p); component names are
 * "<part>@<index>" with part one of total, composition, structure (effects), A, B, C (quantiles), AA, BB, AB, BA
 * (distributions) and index that of the quantile or threshold. */
#define OB_DR_MAX_K 32
#define OB_DR_MAX_T 64
#define OB_DR_MAX_Q 32
#define OB_DR_MAX_VECTORS 128
#define OB_DR_TABLE_QUANTILE_EFFECTS 0
#define OB_DR_TABLE_QUANTILES 1
#define OB_DR_TABLE_DISTRIBUTION_EFFECTS 2
#define OB_DR_TABLE_CDF 3
typedef struct {
  const double* thresholds; /* n_thresholds values, or NULL: pooled quantiles at n_thresholds levels of [lo, hi] */
  int32_t n_thresholds;
  double lo, hi;
  const double* quantiles;  /* n_quantiles values in (0, 1) */
  int32_t n_quantiles;
} ob_dr_config;
typedef struct {
  int32_t passes;   /* the longest batch's Newton passes */
  int32_t launches; /* pass kernels over all batches */
  double pass_ms;   /* the threshold logit pass kernels (the Newton steps not included) */
  double cdf_ms;    /* the distribution pass */
  double row_ms;    /* the rows */
} ob_dr_timing;
typedef struct {
  int32_t n_thresholds, n_quantiles, k; /* thresholds kept, quantiles, design columns */
  int32_t n_requested;                  /* thresholds before duplicates were removed */
  int32_t n_out_of_range;               /* (tau, distribution) pairs of the point estimate that hit an edge case */
  const double* thresholds;             /* [T] */
  const double* quantiles;              /* [n_q] */
  const double* beta;                   /* [2][T][k]: the point fits of A then B */
  const int32_t* passes;                /* [2][T] */
  const uint8_t* out_of_range;          /* [3][n_q]: A, B, C; 1 below F~_1's threshold, 2 above F~_T */
} ob_dr_info;
int ob_dr_row_len(int32_t n_thresholds, int32_t n_quantiles);
/* The shape limits above on their own (host only). k: design columns with the intercept. */
int ob_dr_check_shape(int32_t k, int64_t n_a, int64_t n_b, int32_t n_thresholds, int32_t n_quantiles);
/* HIP-event ms of the calling thread's last distribution-regression boot (or prepare: the point pass). */
int ob_dr_last_timing(ob_dr_timing* out);
/* Host only: the thresholds of a count. out [n_thresholds]; *n_kept of them are filled after duplicate removal. */
int ob_dr_thresholds(const double* y, int64_t n, int32_t n_thresholds, double lo, double hi, double* out,
                     int32_t* n_kept);
/* Host only: rearrange f [T] and invert it at taus [n_q] on thresholds [T]. q [n_q]; rearranged [T] (or NULL);
   edge [n_q] (or NULL): 0, 1 (t* = 1) or 2 (tau > F~_T). */
int ob_dr_quantiles(const double* f, const double* thresholds, int32_t n_thresholds, const double* taus, int32_t n_q,
                    double* q, double* rearranged, uint8_t* edge);
/* Host only: the aggregation of ob_prepared_finish on rows of ob_dr_row_len(T, n_q) doubles and their point row. */
int ob_dr_finish_rows(const double* point_row, int32_t n_thresholds, int32_t n_q, const double* rows, const uint8_t* ok,
                      uint64_t n_reps, ob_results** out);
/* One threshold logit pass alone over one group of rows: x (n x k, column-major, ldx >= n, column 0 all ones), y (n),
   w (n weights or NULL for 1), counts (n bytes or NULL for every row once), thresholds [T] (any finite values, T <=
   OB_DR_MAX_T), betas [T][k]. info [T][k x k] (symmetric, both triangles): sum c w p (1 - p) x x'; grad [T][k]:
   sum c w (1[y <= c_t] - p) x. */
int ob_dr_logit_pass(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, const double* w, const uint8_t* counts,
                     int64_t n, int32_t k, const double* thresholds, int32_t n_thresholds, const double* betas,
                     double* info, double* grad);
/* The distribution pass alone: sums [m] = sum c w L(x' beta_v) for betas [m][k], m <= OB_DR_MAX_VECTORS, and
   *wsum = sum c w. Arguments as ob_dr_logit_pass. */
int ob_dr_cdf(ob_ctx* ctx, const double* x, int64_t ldx, const double* w, const uint8_t* counts, int64_t n, int32_t k,
              const double* betas, int32_t m, double* sums, double* wsum);
int ob_builder_prepare_dr(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                          const ob_builder_config* cfg, const ob_dr_config* dr, ob_prepared** out);
/* prepare + cfg->bootstrap_reps replicates + finish. */
int ob_builder_run_dr(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                      const ob_dr_config* dr, ob_results** out);
/* The handle's thresholds, point fits, pass counts and edge-case counts (owned by the handle). OB_E_INVALID on a
   handle of another kind. */
int ob_prepared_dr_info(const ob_prepared* prep, ob_dr_info* out);

/* ---- Per-replicate RIF of a quantile over resample counts --------------------------------------
 * decompose_quantile(s) computes the RIF once and bootstraps with it held fixed, so every replicate reuses the
 * point estimate's quantile and density. This pass refits both on the resample (Firpo, Fortin, Lemieux 2009; Stata's
 * `oaxaca_rif` under `bootstrap`) without a sort per replicate. A group's rows stand in stable ascending order of
 * y; a replicate is its counts c_i over those rows (sum c_i = n). With Y(k) the y of the first position whose
 * inclusive count prefix exceeds k, the values are rif.rs:14-88 on the expanded resample:
 *     h = (n - 1) tau;  q = Y(floor h) when h is whole, else Y(floor h) + frac (Y(ceil h) - Y(floor h)), the multiply
 *         and the add rounded separately (no FMA): q is bitwise the reference's
 *     mean, sd (over n - 1) of the resample;  iqr = Y(ceil(0.75 n) - 1) - Y(ceil(0.25 n) - 1)
 *     spread = iqr > 1e-8 ? min(sd, iqr / 1.34) : sd;  spread < 1e-8 -> 1.0;  bw = 0.9 spread n^-0.2
 *     f = sum c_i phi((q - y_i) / bw) / (n bw), floored at 1e-8 (floored = 1)
 *     RIF_i = A - B [y_i <= q],  B = 1 / f,  A = q + tau B;  p = upper_bound(y, q): y_i <= q is the row prefix [0, p)
 * and, over v = [1, x_1 .. x_P] (K = P + 1), the y-pairs of the replicate's extended Gram:
 *     T_a = sum_{i < p} c_i v_ia (T_0 = N_le, an exact integer);  G[a, y] = A G[0, a] - B T_a;
 *     G[y, y] = A^2 n - (2 A B - B^2) N_le
 * Limits: K > OB_RIFQ_MAX_K or more than OB_RIFQ_MAX_TAUS quantiles: OB_E_UNSUPPORTED; tau outside (0, 1) or not
 * strictly increasing, y not finite or not ascending, x not finite, counts that do not sum to n: OB_E_INVALID; fewer
 * than 2 rows (or, for a decomposition's shape, a group with rows <= K): OB_E_INSUFFICIENT. All before any device
 * work. Every sum is f64 in an order fixed by n, without atomics: a replicate's values have the same bytes alone, in
 * any batch, and for tau_t alone or among other quantiles. */
#define OB_RIFQ_MAX_K 32
#define OB_RIFQ_MAX_TAUS 8
typedef struct {
  double search_ms;  /* order statistics, quantiles, spread, bandwidth */
  double density_ms; /* the density and column sums over every row: the hot pass */
  double patch_ms;   /* masked sums, f, the Gram's y-pairs */
  double gram_ms;    /* a prepared refit's boots: resample counts, the f64 Gram and its reduce (0 for ob_rifq_pass) */
  double solve_ms;   /* a prepared refit's boots: y-pairs stored, the solves and the rows of every tau (0 likewise) */
} ob_rifq_timing;
typedef struct {
  int32_t n_taus, k;
  int64_t n_a, n_b;
  int64_t n_density_floored; /* floored densities (replicate, group, tau) of the point pass and every boot since */
  const double* taus;        /* [n_taus] */
  const int32_t* perm_a;     /* [n_a] sorted position -> row of group A's cleaned rows (stable ascending y) */
  const int32_t* perm_b;     /* [n_b] */
  const double* q;           /* [2][n_taus] point quantiles, A then B */
  const double* f;           /* [2][n_taus] point densities after the floor */
} ob_rifq_info;
/* The row of ob_builder_prepare_quantiles_refit's handle: the OLS row (ob_row_len) followed by q_A, q_B, f_A, f_B, N_le,A,
   N_le,B. */
int ob_rifq_row_len(int32_t k, int32_t n_base);
/* The shape limits above on their own (host only). k: design columns with the intercept. */
int ob_rifq_check_shape(int32_t k, int32_t n_taus, const double* taus, int64_t n_a, int64_t n_b);
/* The pass over one group. y_sorted [n] ascending; counts [n_reps][n] bytes, or NULL for the point pass (every row
   once, n_reps = 1); x [p][ldx] predictor columns in y's row order (NULL when p = 0). Outputs: q, f, n_le
   [n_reps][n_taus]; bw [n_reps]; t [n_reps][n_taus][p + 1]; gy [n_reps][n_taus][p + 2] = G[a, y] for a <= p, then
   G[y, y] (may be NULL); floored [n_reps][n_taus] (may be NULL). */
int ob_rifq_pass(ob_ctx* ctx, const double* y_sorted, int64_t n, const uint8_t* counts, int32_t n_reps,
                 const double* taus, int32_t n_taus, const double* x, int64_t ldx, int32_t p, double* q, double* bw,
                 double* f, double* n_le, double* t, double* gy, uint8_t* floored);
/* HIP-event ms of the calling thread's last ob_rifq_pass, prepare or boot of a refit handle. */
int ob_rifq_last_timing(ob_rifq_timing* out);
/* decompose_quantiles with the RIF refitted on every replicate. Row-order convention: the handle holds each group's
   cleaned rows in stable ascending order of y, and OBRS-3 position i of group g is the i-th row in that order, so the
   same seed draws other rows than the fixed-RIF run. The Gram is the engine's f64 one over that panel; its y-pairs
   are replaced by the pass above, once per tau, before the engine's solve. Rows are outcome-major [n_taus][n_reps],
   each ob_rifq_row_len(K, 0) doubles. The handle serves ob_prepared_boot, ob_prepared_boot_device (which
   synchronizes), ob_prepared_finish (tau 0) and ob_prepared_point_row ([n_taus][row_len]); residuals are empty.
   Refused before any device work: sample weights, normalize, Heckman settings, a cluster setting, K or n_taus over
   the limits: OB_E_UNSUPPORTED; bad taus, a null or non-finite value in a named column: OB_E_INVALID; a group with
   rows <= K or fewer than 2: OB_E_INSUFFICIENT. ob_prepared_boot_sharded, the jackknives and finish_bca on the
   handle: OB_E_UNSUPPORTED. */
int ob_builder_prepare_quantiles_refit(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                                       const ob_builder_config* cfg, const double* taus, int32_t n_taus,
                                       ob_prepared** out);
/* prepare + cfg->bootstrap_reps replicates + finish per tau: out[n_taus]. */
int ob_builder_decompose_quantiles_refit(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                                         const ob_builder_config* cfg, const double* taus, int32_t n_taus,
                                         ob_results** out);
/* The sort permutations, the point q and f and the floor count (owned by the handle). OB_E_INVALID on a handle of
   another kind. */
int ob_prepared_rifq_info(const ob_prepared* prep, ob_rifq_info* out);
/* ob_prepared_finish for quantile t of a refit handle (or statistic t of ob_builder_prepare_statistics_refit's):
   rows / ok are t's block of a boot. */
int ob_prepared_finish_tau(ob_prepared* prep, int32_t t, const double* rows, const uint8_t* ok, uint64_t n_reps,
                           ob_results** out);

/* ---- Per-replicate RIF of the variance, the Gini and quantile ranges over resample counts ------
 * The refit above for the statistics of ob_builder_decompose_statistics, without a sort or an n-length column per
 * replicate. Setting as above: rows in stable ascending order of y, a replicate is its counts c_i (sum c_i = n),
 * v = [1, x_1 .. x_P], K = P + 1. Per statistic the pass gives its value nu on the expanded resample and the y-pairs
 * G[a, RIF] = sum c v_a RIF, G[RIF, RIF] = sum c RIF^2 of the replicate's extended Gram, with RIF as in 5.12:
 *   OB_RIF_VARIANCE  d = y - mu0 (mu0 the sample's own mean), M0_a = sum c v_a, M1_a = sum c v_a d,
 *                    M2_a = sum c v_a d^2, M3 = sum c d^3, M4 = sum c d^4, delta = M1_0 / n:
 *                    nu = (M2_0 - n delta^2) / n;  G[a, RIF] = M2_a - 2 delta M1_a + delta^2 M0_a;
 *                    G[RIF, RIF] = M4 - 4 delta M3 + 6 delta^2 M2_0 - 4 delta^3 M1_0 + delta^4 n
 *   OB_RIF_GINI      Cin_i, Sin_i the inclusive prefixes of c and c y in row order, mu = Sin_{n-1} / n,
 *                    z_i = y_i (1 - Cin_i / n) + Sin_i / n (the same at a row and at the end of its tie run),
 *                    R = (sum c_i Sin_i + E) / n^2, E = sum over tie runs of more than one row of
 *                    y_run (m_run^2 - sum_{i in run} c_i^2) / 2, m_run = sum_{i in run} c_i; alpha = 2R / mu^2,
 *                    beta = 2 / mu: nu = 1 - 2R / mu;  G[a, RIF] = M0_a + alpha sum c v_a y - beta sum c v_a z;
 *                    G[RIF, RIF] = n + alpha^2 sum c y^2 + beta^2 sum c z^2 + 2 alpha sum c y - 2 beta sum c z
 *                                  - 2 alpha beta sum c y z.  A replicate whose mu is 0 is flagged not ok.
 *   OB_RIF_IQR       RIF_hi - RIF_lo of the pass above (one bandwidth): nu = q_hi - q_lo, G[a, RIF] the difference of
 *                    the two G[a, y], G[RIF, RIF] = G_hh + G_ll - 2 (A_h A_l n - A_h B_l N_le,lo - A_l B_h N_le,hi
 *                    + B_h B_l N_le,lo).
 * Limits, each before any device work and with a NULL context too: K > OB_RIFQ_MAX_K, more than OB_RIFS_MAX_STATS
 * statistics, more than OB_RIFQ_MAX_TAUS distinct quantiles over all ranges, more than 16384 replicates a call:
 * OB_E_UNSUPPORTED; y not finite or not ascending, x not finite, counts that do not sum to n, bad range parameters, for
 * the Gini a negative y or no positive one: OB_E_INVALID; n < 2 (or, for a decomposition's shape, a group with rows
 * <= K): OB_E_INSUFFICIENT. Every sum is f64 in an order fixed by n and the chunk table, without atomics: a
 * replicate's values have the same bytes alone, in any batch, and for a statistic alone or among others. */
#define OB_RIFS_MAX_STATS 8
typedef struct {
  double moment_ms; /* the variance sums and the chunk totals over every row */
  double scan_ms;   /* chunk totals into chunk carries */
  double gini_ms;   /* the Gini's prefix pass over every row */
  double tie_ms;    /* the Gini's tie-run term E */
  double finish_ms; /* chunk partials in chunk order, nu and the y-pairs */
  double gram_ms;   /* a prepared refit's boots: resample counts, the f64 Gram and its reduce (0 for ob_rifs_pass) */
  double solve_ms;  /* a prepared refit's boots: y-pairs stored, the solves and the rows of every statistic */
  double rifq_ms;   /* the quantile pass's three kernels for the ranges */
} ob_rifs_timing;
typedef struct {
  int32_t n_specs, k;
  int64_t n_a, n_b;
  int64_t n_density_floored; /* floored densities (replicate, group, range) of the point pass and every boot since */
  const ob_rif_spec* specs;  /* [n_specs] */
  const int32_t* perm_a;     /* [n_a] sorted position -> row of group A's cleaned rows (stable ascending y) */
  const int32_t* perm_b;     /* [n_b] */
  const double* nu;          /* [2][n_specs] point statistics, A then B */
} ob_rifs_info;
/* The row of ob_builder_prepare_statistics_refit's handle: the OLS row (ob_row_len) followed by nu_A, nu_B. */
int ob_rifs_row_len(int32_t k, int32_t n_base);
/* The shape limits above on their own (host only). k: design columns with the intercept. */
int ob_rifs_check_shape(int32_t k, const ob_rif_spec* specs, int32_t n_specs, int64_t n_a, int64_t n_b);
/* The pass over one group. y_sorted [n] ascending; counts [n_reps][n] bytes, or NULL for the point pass (every row
   once, n_reps = 1); x [p][ldx] predictor columns in y's row order (NULL when p = 0). Outputs: nu [n_reps][n_specs];
   gy [n_reps][n_specs][p + 2] = G[a, RIF] for a <= p, then G[RIF, RIF]; floored [n_reps][n_specs], 1 where a range's
   density was floored (may be NULL); ok [n_reps][n_specs], 0 where a Gini's mu is 0 (nu is then NaN and the pairs 0;
   may be NULL). */
int ob_rifs_pass(ob_ctx* ctx, const double* y_sorted, int64_t n, const uint8_t* counts, int32_t n_reps,
                 const ob_rif_spec* specs, int32_t n_specs, const double* x, int64_t ldx, int32_t p, double* nu,
                 double* gy, uint8_t* floored, uint8_t* ok);
/* HIP-event ms of the calling thread's last ob_rifs_pass, prepare or boot of a statistics refit handle. */
int ob_rifs_last_timing(ob_rifs_timing* out);
/* decompose_statistics with the RIF refitted on every replicate: ob_builder_prepare_quantiles_refit step by step,
   with the same row-order convention (OBRS-3 position i of group g is the i-th row in stable ascending order of y, so
   the same seed draws other rows than the fixed-RIF run). Rows are outcome-major [n_specs][n_reps], each
   ob_rifs_row_len(K, 0) doubles. The handle serves ob_prepared_boot, ob_prepared_boot_device (which synchronizes),
   ob_prepared_finish (statistic 0), ob_prepared_finish_tau (statistic t) and ob_prepared_point_row
   ([n_specs][row_len]); residuals are empty. Refused before any device work: sample weights, normalize, Heckman
   settings, a cluster setting, the limits above: OB_E_UNSUPPORTED; bad specs, a null or non-finite value in a named
   column, for the Gini a negative outcome or a group with no positive one: OB_E_INVALID; a group with rows <= K or
   fewer than 2: OB_E_INSUFFICIENT. ob_prepared_boot_sharded, the jackknives and finish_bca on the handle:
   OB_E_UNSUPPORTED. */
int ob_builder_prepare_statistics_refit(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                                        const ob_builder_config* cfg, const ob_rif_spec* specs, int32_t n_specs,
                                        ob_prepared** out);
/* prepare + cfg->bootstrap_reps replicates + finish per statistic: out[n_specs]. */
int ob_builder_decompose_statistics_refit(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                                          const ob_builder_config* cfg, const ob_rif_spec* specs, int32_t n_specs,
                                          ob_results** out);
/* The statistics, the sort permutations, the point nu and the floor count (owned by the handle). OB_E_INVALID on a
   handle of another kind. */
int ob_prepared_rifs_info(const ob_prepared* prep, ob_rifs_info* out);

/* ---- Nopo's exact-matching decomposition with a bootstrapped common support --------------------
 * Nopo (2008), "Matching as a tool to decompose wage gaps"; Stata's `nopomatch`. No counterpart in the reference
 * crate. Every other decomposition here extrapolates one group's fitted structure to rows of the other group that
 * have no counterpart there; this one compares like with like and reports what the rows without a counterpart owe:
 *     D = D_X + D_0 + D_A + D_B.
 *   Groups and rows: A is the non-reference group, B cfg->reference_group; total_gap = ybar_A - ybar_B. Row i has
 *   outcome y_i, weight w_i (1 without cfg->weights) and resample count c_i (1 in the point pass).
 *   Cells: a cell x is one distinct combination of the values of all matching columns, cfg->predictors then
 *   cfg->categorical. Numeric columns match on exact value (-0.0 = 0.0; i64 columns as integers), categorical columns
 *   on their string bytes. Ids number the distinct key tuples of the rows of A and B in lexicographic order, numeric
 *   columns ascending, categorical columns by bytes; a row of a third group level has id -1.
 *   Row order: each group's rows stand in stable ascending order of cell id, and OBRS-3 position i of a group is its
 *   i-th row in that order (as in the refits: the same seed draws other rows than ob_builder_run does).
 *   Per-cell sums, per group g and cell x, over the group's rows of the cell in that order:
 *     N_g(x) = sum c w, S_g(x) = sum c (w y). A cell's rows are one run of the order; where a chunk boundary of the
 *     panel's chunk table cuts the run, the pieces (fragments) are summed each on its own and added in chunk order.
 *   Support: a cell is in the support S of a replicate iff N_A(x) > 0 and N_B(x) > 0 in that replicate: the common
 *   support is decided again in every replicate.
 *   Aggregates, each accumulated over the cells in id order: N_g, S_g over all cells; N_g^S, S_g^S over support
 *   cells; N_g^out, S_g^out over the others (sums of their own, not differences);
 *     CF = sum_{x in S} N_B(x) (S_A(x) / N_A(x)) / N_B^S.
 *   Terms: D_X = S_A^S / N_A^S - CF; D_0 = CF - S_B^S / N_B^S;
 *     D_A = (N_A^out / N_A) (S_A^out / N_A^out - S_A^S / N_A^S), exactly 0.0 when N_A^out = 0;
 *     D_B = (N_B^out / N_B) (S_B^S / N_B^S - S_B^out / N_B^out), exactly 0.0 when N_B^out = 0;
 *     D = S_A / N_A - S_B / N_B.
 * Row of a replicate, ob_nopo_row_len() = 13 doubles:
 *     D, D_X, D_0, D_A, D_B | ybar_A, ybar_B, E_A[y|S], E_B[y|S], CF | N_A^S / N_A, N_B^S / N_B (the matched shares)
 *     | the number of support cells.
 * A replicate with an empty support, or with N_A = 0 or N_B = 0, has ok = 0 and a NaN row, which ob_prepared_finish
 * drops and counts. Every sum is f64 in a fixed order without atomics: a replicate's row has the same bytes alone, in
 * any batch and at any first_rep. Option "hk_batch" caps a batch at n 64-replicate blocks (default: as many
 * replicates as keep the fragment table within 1 GiB).
 * Errors of the frame entry points, all before any device work and before the context is read: normalize, Heckman
 * settings, more than OB_NOPO_MAX_CELLS cells, a group of 2^31 rows or more: OB_E_UNSUPPORTED; no matching column, a
 * null or non-finite value in a named column, a negative weight: OB_E_INVALID; a group without rows or without
 * positive weight, a point pass with an empty support ("no common support"): OB_E_INSUFFICIENT.
 * cfg->reference_coeffs is ignored. The cluster bootstrap is not served. On a handle prepared here ob_prepared_boot,
 * ob_prepared_boot_device, ob_prepared_finish and ob_prepared_point_row work; ob_prepared_boot_sharded,
 * ob_prepared_jackknife and ob_prepared_finish_bca are OB_E_UNSUPPORTED.
 * Results of ob_prepared_finish / ob_builder_run_nopo: table 0 holds total_gap, composition (D_X), unexplained (D_0),
 * unmatched_a (D_A), unmatched_b (D_B), matched_share_a and matched_share_b, each with the point row's estimate and
 * the standard error, percentile interval and p of ob_bootstrap_stats over the ok replicates. */
/* (2^20 - 4096) / 2: a 64-replicate block's fragment table within 1 GiB at the worst fragment count (ob_nopo.hpp) */
#define OB_NOPO_MAX_CELLS 522240
typedef struct {
  double cell_ms;   /* the per-cell sums */
  double row_ms;    /* the rows */
  double counts_ms; /* the resample: the segments' count images */
} ob_nopo_timing;
typedef struct {
  int32_t n_cells, n_support_cells;
  int64_t n_rows, n_a, n_b;     /* rows of the frame, of A, of B */
  const int64_t* n_cell_a;      /* [n_cells] rows of A in the cell */
  const int64_t* n_cell_b;
  const double* w_a;            /* [n_cells] N_A(x) of the point pass */
  const double* w_b;
  const double* mean_a;         /* [n_cells] S_A(x) / N_A(x) of the point pass, NaN where N_A(x) = 0 */
  const double* mean_b;
  const uint8_t* in_support;    /* [n_cells] */
  const int32_t* row_cell;      /* [n_rows] the cell of every row of the frame, -1 for a row of neither group */
} ob_nopo_info;
int ob_nopo_row_len(void);
/* The shape limits above on their own (host only). */
int ob_nopo_check_shape(int64_t n_cells, int64_t n_a, int64_t n_b);
/* Host only: the cell of every row of the frame (row_cell [n_rows]) and the number of cells. The refusals above
   apply; the groups' sizes, the weights' sums and the support are not looked at. */
int ob_nopo_cells(const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg, int32_t* row_cell,
                  int32_t* n_cells);
/* The cell pass alone over one group of rows in ascending order of cell: y (n), w (n weights or NULL for 1), cell (n
   ids in [0, n_cells), ascending), counts [n_reps][n] bytes (NULL: the point pass, n_reps = 1). n_sums and s_sums
   [n_reps][n_cells]: N(x) and S(x), a cell's fragments added in chunk order; a cell without rows gives 0. */
int ob_nopo_sums(ob_ctx* ctx, const double* y, const double* w, const int32_t* cell, int64_t n, int32_t n_cells,
                 const uint8_t* counts, int32_t n_reps, double* n_sums, double* s_sums);
/* Host only: the aggregation of ob_prepared_finish on rows of ob_nopo_row_len() doubles and their point row. */
int ob_nopo_finish_rows(const double* point_row, const double* rows, const uint8_t* ok, uint64_t n_reps, ob_results** out);
/* HIP-event ms of the calling thread's last matching-decomposition boot (or prepare: the point pass) or ob_nopo_sums. */
int ob_nopo_last_timing(ob_nopo_timing* out);
int ob_builder_prepare_nopo(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                            const ob_builder_config* cfg, ob_prepared** out);
/* prepare + cfg->bootstrap_reps replicates + finish. */
int ob_builder_run_nopo(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                        ob_results** out);
/* The point pass's cell table and every row's cell (owned by the handle). OB_E_INVALID on a handle of another kind. */
int ob_prepared_nopo_info(const ob_prepared* prep, ob_nopo_info* out);

/* ---- Bootstrapped DFL density decomposition with confidence bands ------------------------------
 * DiNardo, Fortin and Lemieux (1996): the densities of the outcome in A, in B and in B reweighted to A's covariates
 * (the counterfactual C), on a grid, with the propensity logit refitted in every bootstrap replicate. ob_dfl_run
 * gives the three curves of the reference crate; this is the same picture under the builder's conventions, with
 * sample weights and with inference. A is the non-reference group, B cfg->reference_group; x the design row with the
 * intercept in column 0 (K <= OB_REWEIGHT_MAX_K columns); w the sample weight (1 without cfg->weights); c the
 * replicate's OBRS-3 count of the row (1 in the point pass): all exactly as in the reweighted decomposition above.
 *   Grid g_0 < .. < g_{G-1}, 2 <= G <= OB_DENSITY_MAX_GRID: given (finite and strictly increasing), or
 *   (ob_density_config.grid == NULL) g_j = min + j (max - min) / G over the outcomes of A and B together, the rule of
 *   dfl.rs:164-172 (the product j * step is rounded before the sum); grid_size 0 is 100.
 *   Bandwidths h_A, h_B: given (finite and > 0), or (0) ob_silverman_bandwidth of each group's outcome, unweighted
 *   (dfl.rs:174-175). They are fixed at prepare time: a replicate does not move them. f_C uses h_B (dfl.rs:178).
 *   Per replicate: gamma is the propensity logit of the reweighted decomposition, unchanged (Newton from 0, the
 *   clamp of p to [1e-10, 1 - 1e-10], the stopping rule, the failure flags); psi_i = p_i / (1 - p_i) on B's rows;
 *   with phi(u) = exp(-u^2 / 2) / sqrt(2 pi)
 *     f_A(g) = sum_A c w phi((g - y) / h_A) / (h_A sum_A c w)
 *     f_B(g) = sum_B c w phi((g - y) / h_B) / (h_B sum_B c w)
 *     f_C(g) = sum_B c w psi phi((g - y) / h_B) / (h_B sum_B c w psi).
 *   The factor P(B) / P(A) of dfl.rs:116 cancels in f_C.
 * Row of a replicate, ob_density_row_len(K, G) = 6 G + K + 2 doubles:
 *     f_A | f_B | f_C | total = f_A - f_B | composition = f_C - f_B | structure = f_A - f_C (G each) | gamma (K) |
 *     the effective sample size (sum c w psi)^2 / sum c (w psi)^2 | the replicate's logit passes.
 * A replicate whose logit fails or does not converge, or one of whose groups has sum c w = 0, has ok = 0 and a NaN
 * row; in the point pass that is OB_E_LINALG for the whole call. Every sum is f64, over a chunk's rows in row order
 * and over the chunks in chunk order, without atomics: a replicate's row has the same bytes alone, in any batch and at
 * any first_rep. Option "hk_batch" caps a batch at n 64-replicate blocks.
 * Errors of the frame entry points, all before any device work and before the context is read: normalize, Heckman
 * settings, K > OB_REWEIGHT_MAX_K, G > OB_DENSITY_MAX_GRID: OB_E_UNSUPPORTED; a null or non-finite value in a named
 * column, a negative weight, G < 2, a grid that is not finite and strictly increasing, a bandwidth that is not finite
 * and > 0 (0 asks for the default): OB_E_INVALID; a group with rows <= K or without positive weight:
 * OB_E_INSUFFICIENT. cfg->reference_coeffs is ignored. The cluster bootstrap is not served. On a handle prepared
 * here ob_prepared_boot, ob_prepared_boot_device, ob_prepared_finish and ob_prepared_point_row work;
 * ob_prepared_boot_sharded, ob_prepared_jackknife and ob_prepared_finish_bca are OB_E_UNSUPPORTED.
 * Results of ob_prepared_finish / ob_builder_run_density / ob_density_finish_rows: table OB_DENSITY_TABLE_CURVES
 * holds the 6 G entries of the curves in row order, each through the aggregation of the other runs (estimate = the
 * point row's, standard error, percentile interval, p); names are "<curve>@<j>" with curve one of density_a,
 * density_b, density_counterfactual, total, composition, structure. Table OB_DENSITY_TABLE_BANDS holds, under the
 * same names, the uniform 95 % band of each curve: over the replicates kept and the grid points with se_j > 0,
 * t_r = max_j |v_rj - point_j| / se_j; crit is the ascending-sorted t at index min(R - 1, floor(0.95 R)), R the
 * replicates kept; ci_lower / ci_upper = point_j -+ crit se_j (the point itself where se_j = 0), estimate = point_j,
 * std_err = se_j, t_stat = crit (the same for every entry of a curve), p_value = NaN. A curve without a kept replicate
 * or without a grid point of positive se has crit = NaN. */
#define OB_DENSITY_MAX_GRID 256
#define OB_DENSITY_MAX_VECTORS 64
#define OB_DENSITY_TABLE_CURVES 0
#define OB_DENSITY_TABLE_BANDS 1
typedef struct {
  int32_t grid_size;  /* 0: 100 */
  const double* grid; /* grid_size points, or NULL: the rule above */
  double bandwidth_a; /* 0: ob_silverman_bandwidth of A's outcome */
  double bandwidth_b; /* 0: of B's */
} ob_density_config; /* a NULL configuration is every default */
typedef struct {
  int32_t logit_passes;   /* the longest batch's Newton rounds */
  int32_t logit_launches; /* logit pass kernels over all batches */
  double logit_ms;        /* the logit pass kernels (the Newton steps not included) */
  double density_ms;      /* the density pass */
  double finish_ms;       /* the rows */
} ob_density_timing;
typedef struct {
  int32_t grid_size, k;
  const double* grid; /* [grid_size] */
  double bandwidth_a, bandwidth_b;
  int64_t n_a, n_b;
} ob_density_info;
/* 6 G + K + 2, or 0 for k < 1 or G outside [2, OB_DENSITY_MAX_GRID]. */
int ob_density_row_len(int32_t k, int32_t grid_size);
/* The shape limits above on their own (host only). k: design columns with the intercept. */
int ob_density_check_shape(int32_t k, int64_t n_a, int64_t n_b, int32_t grid_size);
/* HIP-event ms of the calling thread's last density boot (or prepare: the point pass) or ob_density_pass. */
int ob_density_last_timing(ob_density_timing* out);
/* Host only: the default grid of grid_size points (0: 100) over y (n finite values). out [grid_size]. */
int ob_density_grid(const double* y, int64_t n, int32_t grid_size, double* out);
/* The density pass alone over one group of rows: x (n x k, column-major, ldx >= n, column 0 all ones), y (n), w (n
   weights or NULL for 1), counts (n bytes or NULL for every row once), gammas [m][k], 1 <= m <= OB_DENSITY_MAX_VECTORS
   (NULL: psi = 1 and m = 1), grid [grid_size] (any finite values), h > 0. With v = w psi: num [m][grid_size] =
   sum c v phi((g_j - y) / h), den [m] = sum c v, den2 [m] = sum c v^2; the chunk partials are added in chunk order. */
int ob_density_pass(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, const double* w, const uint8_t* counts,
                    int64_t n, int32_t k, const double* gammas, int32_t m, const double* grid, int32_t grid_size, double h,
                    double* num, double* den, double* den2);
/* Host only: the aggregation of ob_prepared_finish on rows of ob_density_row_len(k, grid_size) doubles and their
   point row. */
int ob_density_finish_rows(const double* point_row, int32_t k, int32_t grid_size, const double* rows, const uint8_t* ok,
                           uint64_t n_reps, ob_results** out);
int ob_builder_prepare_density(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                               const ob_builder_config* cfg, const ob_density_config* dc, ob_prepared** out);
/* prepare + cfg->bootstrap_reps replicates + finish. */
int ob_builder_run_density(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                           const ob_builder_config* cfg, const ob_density_config* dc, ob_results** out);
/* The grid and bandwidths a handle was prepared with; the pointer lives as long as the handle. */
int ob_prepared_density_info(const ob_prepared* prep, ob_density_info* out);

/* ---- Bootstrapped Tobit decomposition of a censored outcome --------------------------------------
 * Bauer and Sinning (2008, 2010), Stata's `nldecompose ..., tobit`: the decomposition of a gap in an outcome that is
 * observed as y = max(lower, min(upper, y*)), y* = x'beta + sigma eps, eps ~ N(0, 1), with either limit optional
 * (none: the Gaussian MLE). No counterpart in the reference crate. A is the non-reference group, B
 * cfg->reference_group; x the design row with the intercept in column 0 (K <= OB_TOBIT_MAX_K columns); w the sample
 * weight (1 without cfg->weights); c the replicate's OBRS-3 count of the row (1 in the point pass). A row is
 * left-censored if y == lower, right-censored if y == upper, else uncensored.
 *   Fit, per group and replicate, in Olsen's parameters eta = [delta; theta], delta = beta / sigma, theta = 1 / sigma,
 *   by Newton's method on the concave log-likelihood. With v = [x; -y], u = theta y - x'delta and lambda = phi / Phi:
 *     gradient = sum c w s v + (N_unc / theta) e_theta,   s = u | -lambda(u) | +lambda(-u)  (uncensored | left | right)
 *     -Hessian = sum c w h v v' + (N_unc / theta^2) e_theta e_theta',   h = 1 | lambda(u) (lambda(u) + u) |
 *     lambda(-u) (lambda(-u) - u);   N_unc = sum c w over the uncensored rows.
 *   The step is the Cholesky solve of -Hessian; while theta + d theta <= 0 the whole step is halved, at most 30 times
 *   (a step still outside, or not finite, fails the fit); the fit stops when the norm of the step taken is below 1e-6,
 *   and fails when it has not after OB_TOBIT_MAX_PASSES passes. The point fit starts from the group's (weighted) least
 *   squares on all rows: delta = beta_ols / s, theta = 1 / s, s^2 = sum w r^2 / sum w; every replicate starts from its
 *   group's point fit. A fit whose resample holds an uncensored count sum (sum c) of at most K is dropped before its
 *   first step: OB_TOBIT_FAILED with eta at its start and no pass counted.
 *   lambda is evaluated without the quotient below z = -0.46875 sqrt 2: finite for every finite z.
 *   The conditional mean m(xb, sigma) = lower Phi(z_a) + upper (1 - Phi(z_b)) + (Phi(z_b) - Phi(z_a)) xb
 *   + sigma (phi(z_a) - phi(z_b)), z_a = (lower - xb) / sigma, z_b = (upper - xb) / sigma, the terms of an absent limit
 *   dropped; M[g][h] = sum_g c w m(x'beta_h, sigma_h) / sum_g c w.
 * Row of a replicate, ob_tobit_row_len(K) = 6 + 7K + 17 doubles (beta* = beta_A under OB_REF_GROUP_A, M[g][*] alike):
 *     explained = M[A][*] - M[B][*], unexplained = total - explained, endowments = M[A][B] - M[B][B],
 *     coefficients = M[B][A] - M[B][B], interaction = total - endowments - coefficients, total = M[A][A] - M[B][B]
 *     | explained_j (K) | unexplained_j (K): Yun's terms as in the binary row, a part with a zero denominator 0.0
 *     | beta_A, beta_B, xbar_A, xbar_B, beta* (K each)
 *     | the latent terms (xbar_A - xbar_B)'beta*, xbar_A'(beta_A - beta*) + xbar_B'(beta* - beta_B), their sum
 *     | M[A][A], M[A][B], M[B][A], M[B][B] | ybar_A, ybar_B | sigma_A, sigma_B
 *     | the censored shares (of sum c w): left A, right A, left B, right B | the passes of A's and B's fit.
 * A replicate one of whose fits failed, or one of whose groups has sum c w = 0, has ok = 0 and a NaN row, which
 * ob_prepared_finish drops and counts. Every sum is f64, over a chunk's rows in row order and over the chunks in chunk
 * order, without atomics: a replicate's row has the same bytes alone, in any batch and at any first_rep. Option
 * "hk_batch" caps a batch at n 64-replicate blocks.
 * Errors of the frame entry points, all before any device work and before the context is read: normalize, Heckman
 * settings, reference coefficients other than OB_REF_GROUP_A / OB_REF_GROUP_B (sigma* has no agreed definition for
 * them), K > OB_TOBIT_MAX_K: OB_E_UNSUPPORTED; a null or non-finite value in a named column, a negative weight, a
 * non-finite limit, lower >= upper, an outcome below lower or above upper: OB_E_INVALID; a group whose uncensored rows
 * are at most K: OB_E_INSUFFICIENT; a start or point fit that fails: OB_E_LINALG. The cluster bootstrap is not served.
 * On a handle prepared here ob_prepared_boot, ob_prepared_boot_device, ob_prepared_finish, ob_prepared_point_row and
 * ob_prepared_tobit_info work; ob_prepared_boot_sharded, ob_prepared_jackknife and ob_prepared_finish_bca are
 * OB_E_UNSUPPORTED. Not built: the split of the unexplained part into a beta share and a sigma share.
 * Results of ob_prepared_finish / ob_builder_run_tobit / ob_tobit_finish_rows: OB_TABLE_TWO_FOLD, OB_TABLE_THREE_FOLD,
 * OB_TABLE_DETAILED_EXPLAINED and OB_TABLE_DETAILED_UNEXPLAINED as ob_builder_run fills them, and
 * OB_TOBIT_TABLE_LATENT with explained, unexplained and total_gap of the latent outcome; ob_results_total_gap is the
 * row's total. */
#define OB_TOBIT_MAX_K 31
#define OB_TOBIT_MAX_PASSES 100
#define OB_TOBIT_MAX_ARRAY_REPS 1024
#define OB_TOBIT_DONE 1u
#define OB_TOBIT_FAILED 2u
#define OB_TOBIT_TABLE_LATENT 3
typedef struct {
  double lower, upper;           /* read only where the flag beside it is set */
  int32_t has_lower, has_upper;
} ob_tobit_config; /* a NULL configuration is no limit */
typedef struct {
  int32_t passes;        /* the longest batch's Newton rounds */
  int32_t pass_launches; /* pass kernels over all batches */
  double pass_ms;        /* the pass kernels (the Newton steps not included) */
  double means_ms;       /* the means pass */
  double row_ms;         /* the rows */
} ob_tobit_timing;
typedef struct {
  int32_t k, has_lower, has_upper, passes_a, passes_b;
  double lower, upper;
  int64_t n_a, n_b, n_left_a, n_right_a, n_left_b, n_right_b; /* rows, and rows at the limits */
  const double* eta; /* [2][k + 1] the point fits of A and B (owned by the handle) */
} ob_tobit_info;
/* 6 + 7K + 17, or 0 for k < 1. */
int ob_tobit_row_len(int32_t k);
/* The shape limits above on their own (host only). k: design columns with the intercept; n_a, n_b: uncensored rows. */
int ob_tobit_check_shape(int32_t k, int64_t n_a, int64_t n_b);
/* HIP-event ms of the calling thread's last Tobit boot (or prepare: the point pass), ob_tobit_fit or ob_tobit_rows. */
int ob_tobit_last_timing(ob_tobit_timing* out);
/* Host only: out[i] = lambda(z[i]) by the branches the kernels take. */
int ob_tobit_lambda(const double* z, int64_t n, double* out);
/* One pass alone over one group of rows: x (n x k, column-major, ldx >= n, column 0 all ones), y (n, within the
   limits), w (n weights or NULL for 1), counts (n bytes or NULL for every row once), etas [m][k + 1], 1 <= m <= 64,
   theta > 0. info [m][k + 1][k + 1] = -Hessian and grad [m][k + 1] = the gradient above (the N_unc terms added on the
   host), n_unc [m]; the chunk partials are added in chunk order. */
int ob_tobit_pass(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, const double* w, const uint8_t* counts,
                  int64_t n, int32_t k, const ob_tobit_config* tc, const double* etas, int32_t m, double* info,
                  double* grad, double* n_unc);
/* The fits alone over one group of rows: counts [n_reps][n] bytes (NULL: n_reps fits of every row once), 1 <= n_reps
   <= OB_TOBIT_MAX_ARRAY_REPS, eta0 [k + 1] the start of every fit (NULL: the least-squares start above). eta
   [n_reps][k + 1], flags [n_reps] (OB_TOBIT_DONE | OB_TOBIT_FAILED; a fit without OB_TOBIT_DONE did not converge),
   passes [n_reps]. */
int ob_tobit_fit(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, const double* w, int64_t n, int32_t k,
                 const ob_tobit_config* tc, const uint8_t* counts, int32_t n_reps, const double* eta0, double* eta,
                 uint32_t* flags, uint32_t* passes);
/* The means pass alone over one group of rows and one replicate's counts (n bytes or NULL): etas [2][k + 1] the fits
   whose parameters are applied. out [6 + k] = M under etas[0], M under etas[1], ybar, sum c w, the left and the right
   censored share, xbar (k). */
int ob_tobit_means(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, const double* w, const uint8_t* counts,
                   int64_t n, int32_t k, const ob_tobit_config* tc, const double* etas, double* out);
/* Fits (from each group's least-squares start), means and rows over two groups of rows: counts_a [n_reps][n_a] and
   counts_b [n_reps][n_b] bytes (both NULL: the point pass, n_reps = 1). rows [n_reps][ob_tobit_row_len(k)], ok
   [n_reps]. */
int ob_tobit_rows(ob_ctx* ctx, int32_t k, const ob_tobit_config* tc, int32_t reference_coeffs, const double* xa, int64_t ldxa,
                  const double* ya, const double* wa, int64_t na, const uint8_t* counts_a, const double* xb, int64_t ldxb,
                  const double* yb, const double* wb, int64_t nb, const uint8_t* counts_b, int32_t n_reps, double* rows,
                  uint8_t* ok);
/* Host only: the aggregation of ob_prepared_finish on rows of ob_tobit_row_len(k) doubles and their point row; the
   detailed components are named "x0" .. "x<k-1>". */
int ob_tobit_finish_rows(const double* point_row, int32_t k, const double* rows, const uint8_t* ok, uint64_t n_reps,
                         ob_results** out);
int ob_builder_prepare_tobit(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                             const ob_builder_config* cfg, const ob_tobit_config* tc, ob_prepared** out);
/* prepare + cfg->bootstrap_reps replicates + finish. */
int ob_builder_run_tobit(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                         const ob_tobit_config* tc, ob_results** out);
/* The limits, the rows at them and the point fits a handle was prepared with. OB_E_INVALID on a handle of another
   kind. */
int ob_prepared_tobit_info(const ob_prepared* prep, ob_tobit_info* out);

#ifdef __cplusplus
}
#endif
#endif /* OAXACA_BOOT_H */
