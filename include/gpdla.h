/* gpdla.h -- C ABI of the MI355X GP-DLA likelihood engine (libgpdla.so).
 *
 * Drop-in boundary for the hot path of sbird/gp_dla_detection (paths are relative to the
 * reference repository):
 *
 *   reference interface                                  replaced by
 *   ---------------------------------------------------  -------------------------------------
 *   voigt MEX: absorption = voigt(lambdas, z, N, nl)     gpdla_voigt_f64
 *     (voigt.c:253-304, called at process_qsos.m:186)
 *   log_p = log_mvnpdf_low_rank(y, mu, M, d)             gpdla_log_mvnpdf_low_rank_f64
 *     (log_mvnpdf_low_rank.m:5-33, process_qsos.m:151,196)
 *   process_qsos.m:88-220 per-spectrum loop + parfor    gpdla_engine_create / _process /
 *     over DLA samples (process_qsos.m:184-198)            _synchronize / _destroy
 *   generate_dla_samples.m:8-57 (haltonset/scramble,     gpdla_generate_dla_samples_f64,
 *     ksdensity, polyfit, integral, fzero)                 gpdla_halton_rr2_f64
 *   read_spec.m:27-38, preload_qsos.m:18-67              gpdla_read_spec_f32,
 *                                                          gpdla_preload_qsos_f32
 *
 * Conventions
 *   - Plain pointers and sizes only.  The caller owns every buffer; the engine owns only its
 *     device workspaces.  Nothing allocated by the library is returned across the ABI.
 *   - Matrices follow MATLAB: M is (rows x k) COLUMN-major.
 *   - Every function returns an int status: GPDLA_OK (0), a negative error, or GPDLA_ENUMERIC
 *     (a non-positive Cholesky/LDL pivot or a non-finite value was met; the affected outputs
 *     are NaN -- MATLAB's chol would have raised, log_mvnpdf_low_rank.m:24).
 *     A message is available from gpdla_last_error() (thread-local).
 *   - Reentrant.  One engine is driven by one host thread; engines on different devices (or
 *     the same device) may run concurrently.
 *   - There is no CPU fallback: without a usable HIP device every compute entry point fails
 *     with GPDLA_EDEVICE.
 */
#ifndef GPDLA_H
#define GPDLA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPDLA_OK 0
#define GPDLA_ENUMERIC 1
#define GPDLA_EINVAL (-1)
#define GPDLA_EDEVICE (-2)
#define GPDLA_ENOMEM (-3)
#define GPDLA_EUNSUPPORTED (-4)

/* ABI version (gpdla_version()).  2: gpdla_stats gained contraction_ms / contraction_launches
 * (its size changed: a caller compiled against a version-1 header must use gpdla_engine_get_stats_n
 * with its own sizeof(gpdla_stats), or be rebuilt).  3: gpdla_device_pci_bus_id.  4: the DLA-sample
 * generator (gpdla_halton_rr2_f64, gpdla_generate_dla_samples_f64) and the ingest kernels.
 * 5: gpdla_last_call_kernel_ms. */
#define GPDLA_ABI_VERSION 5

#define GPDLA_MEM_HOST 0
#define GPDLA_MEM_DEVICE 1

/* absorption-index handling (process_qsos.m:180,189) */
#define GPDLA_ABSORPTION_REFERENCE 0 /* reproduce the quirk: absorption(1:n) of the m in-range values */
#define GPDLA_ABSORPTION_UNMASKED 1  /* pair every unmasked pixel with its own profile value */
/* Likelihood path.  AUTO = the fused single-kernel sweep for ranks 1..24 (compiled for 4 8 10 12 16
 * 20 24; a rank in between runs on the next compiled one with M padded by zero columns, which is
 * exact: pivots 1, zero updates), otherwise the panel-GEMM path (weights kernel + fp64 Gram/u GEMM +
 * batched LDL^T), which takes any rank 1..64 (BASELINE configs[4]: k = 50). */
#define GPDLA_PATH_AUTO 0
#define GPDLA_PATH_FUSED 1
#define GPDLA_PATH_PANEL_GEMM 2
/* Fused sweep with the Gram/u contraction on the int8 matrix cores (Ozaki digit slicing: 32-bit
 * quantised operands, exact integer accumulation, fp64 everywhere else); k <= 20 (compiled for 20,
 * lower ranks zero-padded) with num_lines = 3.  Spectra with more than 30,000 pixels fall back to the
 * fp64 fused kernel.  Agrees with the fp64 path to <= 4e-9 relative on the log-likelihoods (measured
 * 3.8e-9 at BASELINE configs[1]; tests assert 1e-8). */
#define GPDLA_PATH_FUSED_I8 3
/* Panel-GEMM path with the Gram/u GEMMs on the int8 matrix cores (same Ozaki scheme as
 * GPDLA_PATH_FUSED_I8), any rank 1..64 with num_lines = 3; for BASELINE configs[4] (k = 50, quoted in
 * fp32) it agrees with fp64 to <= 4e-9 relative (tests assert 1e-8), far inside fp32's ~5e-6. */
#define GPDLA_PATH_PANEL_GEMM_I8 4
/* GPDLA_PATH_PANEL_GEMM_I8 with a 24-bit Gram contraction: 3 digit planes per operand and the 6 digit
 * pairs of level <= 2 for the k(k+1)/2 Gram entries (instead of 4 planes and 10 pairs: 40% fewer
 * matrix-core operations); the k u entries keep the 32-bit scheme.  Fp32-class, as BASELINE configs[4]
 * is quoted (an fp32 Gram/Cholesky gives 4.5-6e-6): a few 1e-7 relative from fp64 on
 * the log-likelihoods at k = 50, inside the 1e-6 contract. */
#define GPDLA_PATH_PANEL_GEMM_I8_24 5

/* Learned null model (learned_qso_model_<set>.mat, read at process_qsos.m:30-35).  Host memory. */
typedef struct gpdla_model {
  int32_t num_rest;              /* rest-grid size (1,217 for 911.75:0.25:1215.75) */
  int32_t k;                     /* rank (set_parameters.m:36) */
  const double* rest_wavelengths;/* [num_rest], strictly increasing */
  const double* mu;              /* [num_rest] */
  const double* M;               /* [num_rest x k], column-major */
  const double* log_omega;       /* [num_rest] */
  double log_c_0, log_tau_0, log_beta;
} gpdla_model;

/* DLA parameter samples (dla_samples.mat, read at process_qsos.m:38-40).  Host memory. */
typedef struct gpdla_samples {
  int64_t num_samples;           /* S (set_parameters.m:48) */
  const double* offset_samples;  /* [S] in [0,1]; any finite value is accepted, NaN / inf is GPDLA_EINVAL */
  const double* nhi_samples;     /* [S] N_HI in cm^-2 (10.^log_nhi_samples) */
} gpdla_samples;

/* set_parameters.m knobs the path reads. */
typedef struct gpdla_params {
  int32_t num_lines;             /* 1..31 (set_parameters.m:63; voigt.c:16) */
  int32_t width;                 /* must be 3 (set_parameters.m:59 == voigt.c:229) */
  double pixel_spacing;          /* 1e-4 dex (set_parameters.m:60) */
  double min_lambda, max_lambda; /* 911.75, 1215.75 (set_parameters.m:33-34) */
  double lya_wavelength;         /* 1215.6701 (set_parameters.m:5) */
  double lyman_limit;            /* 911.7633 (set_parameters.m:7) */
  double min_z_cut, max_z_cut;   /* kms_to_z(3000) (set_parameters.m:65,69) */
  int32_t absorption_mode;       /* GPDLA_ABSORPTION_* */
  int32_t max_batch_spectra;     /* spectra per device batch; 0 = library default */
  int32_t path;                  /* GPDLA_PATH_*: fused kernel or panel-GEMM (see below) */
} gpdla_params;

/* Preloaded spectra (preloaded_qsos.mat cells, process_qsos.m:46-61), CSR-packed.
 * `offsets` is ALWAYS host memory; the pixel arrays and z_qsos live in `memory`. */
typedef struct gpdla_spectra {
  int32_t memory;                /* GPDLA_MEM_HOST or GPDLA_MEM_DEVICE */
  int64_t num_spectra;           /* Q */
  const int64_t* offsets;        /* [Q+1] host; spectrum q = pixels offsets[q]..offsets[q+1]-1 */
  const double* wavelengths;     /* observed, Angstrom */
  const double* flux;
  const double* noise_variance;
  const uint8_t* pixel_mask;     /* nonzero = masked */
  const double* z_qsos;          /* [Q] */
} gpdla_spectra;

/* Per-spectrum outputs (the hot-path subset of processed_qsos_<set>.mat, process_qsos.m:235-249). */
typedef struct gpdla_results {
  int32_t memory;                      /* GPDLA_MEM_HOST or GPDLA_MEM_DEVICE */
  double* log_likelihoods_no_dla;      /* [Q]   process_qsos.m:150-152 */
  double* sample_log_likelihoods_dla;  /* [Q x sample_ld] spectrum-major, or NULL (process_qsos.m:195) */
  int64_t sample_ld;                   /* >= S */
  double* log_likelihoods_dla;         /* [Q]   process_qsos.m:202-209 */
  double* min_z_dlas;                  /* [Q]   process_qsos.m:160 (may be NULL) */
  double* max_z_dlas;                  /* [Q]   process_qsos.m:161 (may be NULL) */
  int32_t* num_pixels;                 /* [Q]   n, unmasked in-range pixels (may be NULL) */
} gpdla_results;

/* Kernel-time accounting (HIP events on the engine's stream), cumulative since create/reset.
 * likelihood_ms spans each batch's likelihood work on the engine's stream.  contraction_ms is the sum
 * of the event spans around each Gram/u GEMM launch (panel-GEMM paths): with one panel stream those
 * spans lie inside likelihood_ms; with panel_streams > 1 the launches of different streams overlap in
 * time and each span also counts the time its launch waits behind the other streams' kernels, so the
 * sum is not part of likelihood_ms and can exceed it (set 1 panel stream to time the kernel alone). */
typedef struct gpdla_stats {
  double prep_ms, likelihood_ms, reduce_ms;
  int64_t prep_launches, likelihood_launches, reduce_launches;
  int64_t spectra, sample_evals;       /* sample_evals = sum over spectra of S (null evals excluded) */
  double contraction_ms;               /* panel-GEMM paths: summed GEMM launch spans (see above) */
  int64_t contraction_launches;
} gpdla_stats;

typedef struct gpdla_engine gpdla_engine;

int gpdla_engine_create(int32_t device, const gpdla_model* model, const gpdla_samples* samples,
                        const gpdla_params* params, gpdla_engine** out);
/* Enqueue the whole pipeline for all spectra.  With GPDLA_MEM_HOST results the call blocks until
 * the outputs are copied back; with device results it returns after enqueueing (use
 * gpdla_engine_synchronize).  Spectra may be processed in several device batches.  With host
 * inputs and host results the batches are pipelined: batch b's inputs are copied in, and batch
 * b - 1's results copied out, on a copy stream of the engine's own while the kernels run. */
int gpdla_engine_process(gpdla_engine* engine, const gpdla_spectra* spectra,
                         const gpdla_results* results);
/* Wait for enqueued work; returns GPDLA_ENUMERIC if any pivot was non-positive since the last call. */
int gpdla_engine_synchronize(gpdla_engine* engine);
/* Use an external hipStream_t (NULL restores the engine's own stream; the null stream itself is
 * selected by gpdla_engine_use_null_stream).  All kernels of a process
 * call are ordered on that stream (after the work already on it); the host-buffer copies above run on
 * the engine's copy stream, ordered against it by events. */
int gpdla_engine_set_stream(gpdla_engine* engine, void* hip_stream);
/* Order the kernels on the null stream (stream 0, e.g. PyTorch's default stream), as
 * gpdla_engine_set_stream does for any other stream. */
int gpdla_engine_use_null_stream(gpdla_engine* engine);
/* Panel-GEMM paths (fp64 and int8): the number of compute streams (1..4, default 2) a batch's spectra
 * alternate over.  Spectrum q of a batch runs on stream q % n (0 = the engine's stream, the others
 * engine-owned) with a workspace of its own, forked from and joined back into the engine's stream;
 * results are bitwise identical for every n. */
int gpdla_engine_set_panel_streams(gpdla_engine* engine, int32_t n);
int gpdla_engine_get_stats(gpdla_engine* engine, gpdla_stats* stats);
/* The same, writing at most stats_bytes bytes (a caller's sizeof(gpdla_stats) from an older header). */
int gpdla_engine_get_stats_n(gpdla_engine* engine, gpdla_stats* stats, int64_t stats_bytes);
int gpdla_engine_reset_stats(gpdla_engine* engine);
void gpdla_engine_destroy(gpdla_engine* engine);

/* ---- Multi-DLA search (Ho, Bird & Garnett 2020, arXiv:2003.11036; DESIGN.md "Multi-DLA") ---------
 * Level 1 is gpdla_engine_process's single-DLA model.  At level d = 2..max_dlas sample j holds d
 * DLAs: its own (z_j, N_j) and the d - 1 of a base sample b_d(j) drawn from the level-(d-1) posterior
 * of the same spectrum by inverse-CDF resampling with the uniform resample_uniforms[(d-2) S + j].  The
 * absorption is the product of the d separately broadened profiles; a sample closer than
 * min_z_separation in z to one of its base DLAs is NaN; the level's evidence is the log-mean-exp over
 * its non-NaN samples minus (d-1) occam_log_penalty.  A level below which no sample is finite is NaN
 * with base indices -1, as is every deeper one.  Sample indices are in the caller's sample order.
 * Fused fp64 path with num_lines = 3 only (GPDLA_EUNSUPPORTED otherwise when max_dlas > 1). */
#define GPDLA_MAX_DLAS 4
typedef struct gpdla_multi_dla {
  int32_t max_dlas;                  /* D, 1..GPDLA_MAX_DLAS */
  double min_z_separation;           /* kms_to_z(3000) in the reference lineage */
  double occam_log_penalty;          /* per additional DLA; log(S) is the paper's Occam factor */
  const double* resample_uniforms;   /* host [(D-1) x S] in [0, 1), one row per level; NULL if D = 1 */
  const int32_t* forced_base_inds;   /* host [D-1][Q][S], 0-based, -1 = none; or NULL.  When given the
                                        resampler is skipped (tests, replaying a saved run) */
} gpdla_multi_dla;

typedef struct gpdla_results_multi {
  int32_t memory;                      /* GPDLA_MEM_HOST or GPDLA_MEM_DEVICE */
  double* log_likelihoods_no_dla;      /* [Q] */
  double* log_likelihoods_dla;         /* [D][Q] */
  double* sample_log_likelihoods_dla;  /* [D][Q][sample_ld], or NULL */
  int64_t sample_ld;                   /* >= S */
  int32_t* base_sample_inds;           /* [D-1][Q][sample_ld] 0-based, -1 = none; or NULL */
  double* min_z_dlas;                  /* [Q] (may be NULL) */
  double* max_z_dlas;                  /* [Q] (may be NULL) */
  int32_t* num_pixels;                 /* [Q] (may be NULL) */
} gpdla_results_multi;

/* Kernel times of gpdla_engine_process_multi (HIP events), cumulative since create / reset_stats.
 * level_ms[0] is the level-1 likelihood time (the same span gpdla_stats::likelihood_ms counts);
 * level_ms[d-1], d >= 2, spans the level-d sweep; resample_ms the resampling / chain kernels and
 * multi_reduce_ms the NaN-aware log-mean-exp of the levels >= 2. */
typedef struct gpdla_multi_stats {
  double level_ms[GPDLA_MAX_DLAS];
  int64_t level_launches[GPDLA_MAX_DLAS];
  double resample_ms;
  int64_t resample_launches;
  double multi_reduce_ms;
  int64_t multi_reduce_launches;
} gpdla_multi_stats;

/* All levels for all spectra.  Spectra go through in device batches, each drained before the next
 * (no copy pipeline).  Host or device memory as in gpdla_engine_process; with device results the call
 * still returns only after the last batch has finished.  Returns GPDLA_ENUMERIC like
 * gpdla_engine_process (a non-positive pivot; the designated NaNs above do not count). */
int gpdla_engine_process_multi(gpdla_engine* engine, const gpdla_spectra* spectra,
                               const gpdla_multi_dla* multi, const gpdla_results_multi* results);
int gpdla_engine_get_multi_stats(gpdla_engine* engine, gpdla_multi_stats* stats);
/* The resampler alone, host buffers: for each of `rows` rows of S log likelihoods (row stride ld),
 * w_i = exp(ll_i - max), NaN -> 0, C the inclusive prefix sum; out_inds[r * S + j] = the smallest i
 * with C_i > u[j] C_{S-1} (the last i with w_i > 0 if rounding leaves none), or -1 for every j of a
 * row whose weight sum is 0 or not finite.  u: [S] in [0, 1). */
int gpdla_resample_f64(int32_t device, const double* ll, int64_t rows, int64_t S, int64_t ld,
                       const double* u, int32_t* out_inds);

/* ---- Posterior summaries ---------------------------------------------------
 * What the catalogue (generate_ascii_catalog.m:73-80) and the population statistics (CDDF_analysis/
 * calc_cddf.py:98, _get_z_nhi_hist :829-870) take from the sample log-likelihoods, reduced on the device
 * so the [D][Q][S] array itself becomes optional.  Per spectrum and level d:
 *   map_sample_inds       the smallest index attaining the maximum over the non-NaN samples (nanmax's
 *                         first maximum), -1 if every sample is NaN; map_log_likelihoods that maximum (NaN)
 *   map_z_dlas/_log_nhis  the d (z_DLA, log N_HI) pairs of that sample: its own, then those of its base
 *                         chain (b1 = level d's base index of j, b2 = level d-1's base index of b1,
 *                         ...: base_sample_inds[d-2][q][j], [d-3][q][b1], ...); z = min_z + (max_z - min_z) *
 *                         offset with the product and the sum rounded separately.  Slots >= d are NaN; all
 *                         are NaN when there is no MAP sample or the chain meets a -1.
 * and for level 1, when a grid is given, the normalised masses pi_j = w_j / W, w_j = exp(l_j - max)
 * (NaN -> 0), W = sum w_j (every pi = 0 if W is 0 or not finite), summed per bin of the grid: sample j
 * belongs to bin (iz, in) when z_edges[iz] <= z_j < z_edges[iz+1] and log_nhi_edges[in] <= log_nhi_j <
 * log_nhi_edges[in+1]; samples outside are dropped.  The GPDLA_SUMMARY_PLANES sums per bin are
 *   sum pi, sum pi^2, sum N pi, sum N^2 pi, sum N^2 pi^2      (N = nhi_samples)
 * Every output is a fixed-order reduction: repeated calls and any split into device batches agree bit for
 * bit. */
#define GPDLA_SUMMARY_PLANES 5
#define GPDLA_SUMMARY_MAX_BINS 1024
typedef struct gpdla_summary_spec {
  const double* log_nhi_samples;     /* host [S], the engine's samples' log10 N_HI in the caller's order */
  int32_t num_z_bins, num_nhi_bins;  /* nz, nn with nz nn <= GPDLA_SUMMARY_MAX_BINS; 0, 0 = MAP only */
  const double* z_edges;             /* host [nz + 1], absolute redshift, finite, strictly increasing */
  const double* log_nhi_edges;       /* host [nn + 1], likewise */
} gpdla_summary_spec;

typedef struct gpdla_summaries {
  int32_t memory;                    /* GPDLA_MEM_HOST or GPDLA_MEM_DEVICE */
  int32_t* map_sample_inds;          /* [D][Q] 0-based, -1 = none */
  double* map_log_likelihoods;       /* [D][Q] */
  double* map_z_dlas;                /* [D][Q][GPDLA_MAX_DLAS] */
  double* map_log_nhis;              /* [D][Q][GPDLA_MAX_DLAS] */
  double* bin_planes;                /* [Q][GPDLA_SUMMARY_PLANES][nz][nn]; NULL only when nz = nn = 0 */
} gpdla_summaries;

/* gpdla_engine_process_multi (max_dlas 1..GPDLA_MAX_DLAS, the same restrictions and the same results,
 * bit for bit) with the summaries computed per device batch after its last level.  Here
 * results->sample_log_likelihoods_dla and ->base_sample_inds may be NULL at no loss: the catalogue and
 * the binned masses no longer need them.  GPDLA_EINVAL for a null spec, summaries or required array, one
 * of nz / nn zero and the other not, more than GPDLA_SUMMARY_MAX_BINS bins, non-finite or
 * non-increasing edges. */
int gpdla_engine_process_summaries(gpdla_engine* engine, const gpdla_spectra* spectra,
                                   const gpdla_multi_dla* multi, const gpdla_results_multi* results,
                                   const gpdla_summary_spec* spec, const gpdla_summaries* summaries);
/* Cumulative kernel time (HIP events) and count of the summary launches since create / reset_stats. */
int gpdla_engine_get_summary_stats(gpdla_engine* engine, double* ms, int64_t* launches);
/* The summary kernel alone, host buffers: ll [levels][rows][ld] (ld >= S), the samples in the rows'
 * order (offset_samples, log_nhi_samples, nhi_samples, each [S]), min_z / max_z [rows], base_inds
 * [levels - 1][rows][ld] (0-based, -1 = none; NULL when levels = 1).  spec gives the grid (its
 * log_nhi_samples is not read here); outputs as in gpdla_summaries with D = levels, Q = rows, in host
 * memory. */
int gpdla_posterior_summary_f64(int32_t device, const double* ll, int64_t rows, int64_t S, int64_t ld,
                                const double* offset_samples, const double* log_nhi_samples,
                                const double* nhi_samples, const double* min_z, const double* max_z,
                                const int32_t* base_inds, int32_t levels, const gpdla_summary_spec* spec,
                                int32_t* map_sample_inds, double* map_log_likelihoods, double* map_z_dlas,
                                double* map_log_nhis, double* bin_planes);

/* ---- Sub-DLA model and Lyman-series forest (Ho, Bird & Garnett 2020) ---------
 * Forest.  For a pixel at observed wavelength lambda of a quasar at z_QSO and line i = 1..L
 * (lambda_i = the i-th Lyman-series wavelength, c_i = f_i lambda_i / (f_1 lambda_1)):
 *   z_i = (lambda - lambda_i) / lambda_i,   t_i(tau_0, beta) = tau_0 c_i (1 + z_i)^beta [z_i <= z_QSO]
 * summed in line order.  variance_series replaces process_qsos.m:145-147 by
 *   omega^2 = exp(2 log omega) (1 - exp(-sum_i t_i(tau_0, beta)) + c_0)^2   (the model's tau_0, beta, c_0)
 * and mean_flux multiplies mu by exp(-sum_i t_i(mean_flux_tau_0, mean_flux_beta)) for every model (null,
 * sub-DLA, every DLA level).  lambda is the pixel's own wavelength; masked and padding slots stay neutral.
 * Fused fp64 path only: on an int8 or panel-GEMM engine gpdla_engine_set_forest returns
 * GPDLA_EUNSUPPORTED (their slot scalars feed quantisation scales derived from mu, which the forest
 * kernel does not rebuild). */
typedef struct gpdla_forest {
  int32_t num_forest_lines;          /* L, 1..31 */
  int32_t variance_series;           /* nonzero: omega^2 sums the series */
  int32_t mean_flux;                 /* nonzero: mu is suppressed by the mean flux */
  double mean_flux_tau_0;            /* finite, >= 0 (Kim et al. 2007: 0.0023) */
  double mean_flux_beta;             /* finite (Kim et al. 2007: 3.65) */
} gpdla_forest;
/* Applies to every later process* call of the engine; NULL restores the Lya-only null model.
 * GPDLA_EINVAL for L outside 1..31, a non-finite or negative mean_flux_tau_0, a non-finite
 * mean_flux_beta. */
int gpdla_engine_set_forest(gpdla_engine* engine, const gpdla_forest* forest);
/* gpdla_engine_set_forest plus what the mean flux F = exp(-sum_i t_i(mean_flux_tau_0, mean_flux_beta))
 * multiplies, for every model: 0 mu (= gpdla_engine_set_forest, which therefore
 * also resets a scope set earlier), 1 mu and the rows of M (the Ho, Bird & Garnett 2020 inference), 2 mu,
 * the rows of M and omega^2 (by F^2, after variance_series): y ~ N(F mu, diag(F) M M' diag(F) +
 * diag(F^2 omega^2 + sigma^2)), the model training under the mean flux learns.  Each interpolated M entry
 * is multiplied by F once and the Khatri-Rao entries are products of the scaled entries.  GPDLA_EINVAL
 * for a scope outside 0..2 and for a scope != 0 with mean_flux == 0 (or forest == NULL);
 * GPDLA_EUNSUPPORTED on int8 and panel-GEMM engines; a failed call leaves the setting as it was.  Under a
 * scope != 0 a second kernel follows the forest kernel in every device batch; its time is added to
 * gpdla_model_stats.forest_ms and it counts in forest_launches (two per batch). */
int gpdla_engine_set_forest_scoped(gpdla_engine* engine, const gpdla_forest* forest, int32_t mean_flux_scope);
/* sum_i t_i(tau_0, beta) at n observed wavelengths (host buffers), by the device function the engine's
 * forest kernel calls. */
int gpdla_forest_f64(int32_t device, const double* wavelengths, int64_t n, double z_qso, double tau_0,
                     double beta, int32_t num_forest_lines, double* out);

/* Sub-DLA model: one absorber at z_j = min_z + (max_z - min_z) offset_j (the engine's own offsets) with
 * column density nhi_samples[j]; its sample likelihood is the level-1 likelihood with that column
 * density, its evidence gpdla_engine_process's log-mean-exp (any NaN -> NaN).  It never enters a
 * multi-DLA chain.  Fused fp64 path only (GPDLA_EUNSUPPORTED otherwise). */
typedef struct gpdla_sub_dla {
  const double* nhi_samples;         /* host [S], cm^-2, finite and > 0, in the caller's sample order */
} gpdla_sub_dla;
typedef struct gpdla_results_sub {
  int32_t memory;                      /* GPDLA_MEM_HOST or GPDLA_MEM_DEVICE */
  double* log_likelihoods_lls;         /* [Q] evidence */
  double* sample_log_likelihoods_lls;  /* [Q x sample_ld] spectrum-major, or NULL */
  int64_t sample_ld;                   /* >= S */
  /* the MAP sample (filled when the call has a summary spec; each may be NULL) */
  const double* log_nhi_samples;       /* host [S] log10 of nhi_samples; required for the MAP outputs */
  int32_t* map_sample_inds;            /* [Q] 0-based, -1 = none */
  double* map_log_likelihoods;         /* [Q] */
  double* map_z_lls;                   /* [Q] */
  double* map_log_nhi_lls;             /* [Q] */
} gpdla_results_sub;
/* gpdla_engine_process_summaries (spec != NULL) or gpdla_engine_process_multi (spec == NULL) with the
 * sub-DLA sweep run per device batch after its level 1, while the slot panel is resident.  With
 * sub == NULL it is that call, bit for bit; with sub, every other result is unchanged bit for bit.
 * GPDLA_EINVAL for a null, non-positive or non-finite column density or a null results_sub / evidence
 * array. */
int gpdla_engine_process_models(gpdla_engine* engine, const gpdla_spectra* spectra,
                                const gpdla_multi_dla* multi, const gpdla_sub_dla* sub,
                                const gpdla_results_multi* results_multi, const gpdla_results_sub* results_sub,
                                const gpdla_summary_spec* spec, const gpdla_summaries* summaries);
/* Cumulative kernel times (HIP events) and launch counts since create / reset_stats: the forest kernel
 * and the sub-DLA sweeps (likelihood launch; its log-mean-exp and MAP launches are counted apart). */
typedef struct gpdla_model_stats {
  double forest_ms, sub_dla_ms, sub_dla_reduce_ms;
  int64_t forest_launches, sub_dla_launches, sub_dla_reduce_launches;
} gpdla_model_stats;
int gpdla_engine_get_model_stats(gpdla_engine* engine, gpdla_model_stats* stats);

/* ---- Population statistics (CDDF_analysis/calc_cddf.py) -----------------------
 * What the reference's confidence intervals on f(N), dN/dX and Omega_DLA need from the level-1 sample
 * rows (_split_distributions_single, calc_cddf.py:724-778), reduced per device batch after its last
 * level.  With pi_j the normalised level-1 masses exactly as the summaries form them and p_dla the
 * spectrum's posterior probability of at least one DLA, p_j = p_dla pi_j, and sample j belongs to a bin
 * of the spec's own (z, log N_HI) grid by the summaries' rule (half-open, z with separately rounded
 * product and sum; samples outside belong to no bin).  Per spectrum q:
 *   poisson_plane   per bin, the sum of p_j over its samples with p_thresh_sample < p_j < p_switch, added
 *                   in sample-index order
 *   large_*         the samples with p_j >= p_switch that fall in some bin, by increasing sample index:
 *                   index (0-based), p_j and bin (iz num_nhi_bins + in); unused slots -1 / NaN / -1
 *   p_dlas          the p_dla used: formed on the device from the evidences and the spec's log priors as
 *                   exp(lp_m - max) / sum over the models no-DLA, DLA levels 1..D (a NaN evidence at a
 *                   level >= 2 counts as -inf) and, with the sub-DLA model, sub-DLA;
 *                   p_dla = 1 - p_no (- p_sub).  NaN when a posterior is NaN: such a row gives zeros.
 * sum pi = 1 bounds the large samples by 1 / p_switch, hence p_switch >= 1 / GPDLA_POPULATION_MAX_LARGE.
 * Every output is a fixed-order reduction: repeated calls and any split into device batches agree bit
 * for bit. */
#define GPDLA_POPULATION_MAX_LARGE 8
typedef struct gpdla_population_spec {
  const double* log_nhi_samples;     /* host [S]; not read by gpdla_population_split_f64 */
  int32_t num_z_bins, num_nhi_bins;  /* nz, nn >= 1 with nz nn <= GPDLA_SUMMARY_MAX_BINS */
  const double* z_edges;             /* host [nz + 1], absolute redshift, finite, strictly increasing */
  const double* log_nhi_edges;       /* host [nn + 1], likewise */
  double p_thresh_sample;            /* in [0, p_switch) (calc_cddf.py:47: 1e-4) */
  double p_switch;                   /* >= 1 / GPDLA_POPULATION_MAX_LARGE (calc_cddf.py:50: 0.25) */
  double p_thresh_spec;              /* recorded for the host stage (calc_cddf.py:45: 0.05); not applied here */
  /* log priors, host; read by gpdla_engine_process_population only */
  const double* log_priors_no_dla;   /* [Q] */
  const double* log_priors_dla;      /* [D][Q] */
  const double* log_priors_lls;      /* [Q]; required with the sub-DLA model */
} gpdla_population_spec;

typedef struct gpdla_population {
  int32_t memory;                    /* GPDLA_MEM_HOST or GPDLA_MEM_DEVICE */
  double* poisson_plane;             /* [Q][nz][nn] */
  int32_t* large_inds;               /* [Q][GPDLA_POPULATION_MAX_LARGE] */
  double* large_probs;               /* [Q][GPDLA_POPULATION_MAX_LARGE] */
  int32_t* large_bins;               /* [Q][GPDLA_POPULATION_MAX_LARGE] */
  double* p_dlas;                    /* [Q] */
} gpdla_population;

/* gpdla_engine_process_models plus the population outputs; with pspec and population both NULL it is
 * that call, bit for bit, and with them every other result is unchanged bit for bit.  GPDLA_EINVAL for
 * one of the two NULL and the other not, a null array, a malformed grid, p_switch < 1 /
 * GPDLA_POPULATION_MAX_LARGE or p_thresh_sample outside [0, p_switch). */
int gpdla_engine_process_population(gpdla_engine* engine, const gpdla_spectra* spectra,
                                    const gpdla_multi_dla* multi, const gpdla_sub_dla* sub,
                                    const gpdla_results_multi* results_multi, const gpdla_results_sub* results_sub,
                                    const gpdla_summary_spec* spec, const gpdla_summaries* summaries,
                                    const gpdla_population_spec* pspec, const gpdla_population* population);
/* Cumulative kernel time (HIP events) and count of the population launches (the posterior and the split
 * launch of a batch are one span) since create / reset_stats. */
int gpdla_engine_get_population_stats(gpdla_engine* engine, double* ms, int64_t* launches);
/* The split kernel alone, host buffers: ll [rows][ld] (ld >= S), the samples in the rows' order, min_z /
 * max_z / p_dlas [rows] (p_dlas in [0, 1] or NaN).  Outputs as in gpdla_population with Q = rows. */
int gpdla_population_split_f64(int32_t device, const double* ll, int64_t rows, int64_t S, int64_t ld,
                               const double* offset_samples, const double* log_nhi_samples, const double* min_z,
                               const double* max_z, const double* p_dlas, const gpdla_population_spec* spec,
                               double* poisson_plane, int32_t* large_inds, double* large_probs, int32_t* large_bins);
/* Poisson-binomial pmf of num_bins trial lists in CSR form (host buffers): bin b holds the probabilities
 * probs[offsets[b] .. offsets[b + 1]) (offsets[0] = 0, n_b <= GPDLA_PMF_MAX_TRIALS each) and receives the
 * n_b + 1 coefficients of prod_j (1 - p_j + p_j x) at pmf[offsets[b] + b ...]; n_b = 0 gives [1.0].  A
 * product of polynomials with non-negative coefficients (no DFT): chunks of GPDLA_PMF_CHUNK trials by the
 * recurrence pmf[k] <- pmf[k] (1 - p) + pmf[k - 1] p, folded left to right by convolution, so every
 * coefficient above the smallest normal is within a relative 4 (n_b + 1) 2^-53 of the exact one and a
 * bin's result does not depend on the other bins of the call.  GPDLA_EINVAL for a probability outside
 * [0, 1] or non-finite.  gpdla_last_call_kernel_ms then reports 2 spans: the chunk launch, the folds. */
#define GPDLA_PMF_CHUNK 512
#define GPDLA_PMF_MAX_TRIALS (1 << 18)
int gpdla_poisson_binomial_pmf_f64(int32_t device, const double* probs, const int64_t* offsets, int64_t num_bins,
                                   double* pmf);

/* ---- Population statistics over every multi-DLA level --------------------------
 * The reductions above count the level-1 samples only.  These count every absorber of every level of a
 * max_dlas = D run, under section 12's model.  For spectrum q, level d = 1..D and sample j (caller order):
 *   masses      pi_{d,j} = w / W over level d's row, w = exp(l_d[j] - max over the non-NaN entries) (NaN ->
 *               0), W = sum w, every pi 0 if W is 0 or not finite; formed by the partial sums and trees of
 *               the level-1 reductions, so pi_{1,j} is their pi_j bit for bit
 *   absorbers   sample (d, j) carries d of them: slot 0 is sample j itself, slots 1..d-1 its base chain
 *               b1 = base_sample_inds[d-2][q][j], b2 = base_sample_inds[d-3][q][b1], ... (the walk of
 *               map_z_dlas).  Slot i has z = min_z + (max_z - min_z) offset_i (product and sum rounded
 *               separately), log N_i and N_i of its sample and the bin the level-1 rule gives those.  A chain
 *               that meets -1 or an index outside [0, S) voids every slot of the sample: it contributes
 *               nothing, though its pi still counts in W
 *   posteriors  P_d = exp(lp_d - max) / sum over the models no-DLA, DLA 1..D (a NaN evidence at a level >= 2
 *               counts as -inf) and, with the sub-DLA model, sub-DLA: the terms p_dlas is formed from.  Any
 *               other NaN makes every P_d of the spectrum NaN, and the spectrum contributes nothing.  The
 *               sub-DLA model is not a DLA and enters none of the sums below
 *   bin_planes     (summary grid) per level and bin, over the (sample, slot) pairs whose slot falls in the
 *                  bin: sum pi, pi^2, N pi, N^2 pi, N^2 pi^2 with N the slot's column density, added in
 *                  (sample index, slot) order.  Level 1's planes are gpdla_summaries.bin_planes bit for bit
 *   poisson_plane  (population grid) with p = P_d pi_{d,j}: a sample with p_thresh_sample < p < p_switch (or
 *                  with p >= p_switch and no slot inside the grid: nothing) adds p to the bin of each of its
 *                  slots inside the grid, in (sample index, slot) order
 *   large_*        the samples with p >= p_switch and at least one slot inside the grid, by increasing sample
 *                  index: index (0-based), p and one bin per slot (iz num_nhi_bins + in; -1 for a slot outside
 *                  the grid or beyond d).  They add nothing to poisson_plane.  sum_j P_d pi_{d,j} <= 1 bounds
 *                  them by 1 / p_switch <= GPDLA_POPULATION_MAX_LARGE per level.  Unused entries -1 / NaN / -1
 * The expected number of DLAs of spectrum q in bin b is sum_d P_d sum_{(j, slot) in b} pi_{d,j}; the host
 * stage treats every (level, sample, slot) as one Bernoulli trial of probability P_d pi_{d,j}.  Every
 * output is a fixed-order reduction of the spectrum's own rows: repeated calls and any split into device
 * batches agree bit for bit.  No floating-point atomics. */
typedef struct gpdla_level_population {
  int32_t memory;                    /* GPDLA_MEM_HOST or GPDLA_MEM_DEVICE */
  double* level_posteriors;          /* [D][Q] */
  double* bin_planes;                /* [Q][D][GPDLA_SUMMARY_PLANES][nz][nn], summary grid; NULL without one */
  double* poisson_plane;             /* [Q][D][nz][nn], population grid */
  int32_t* large_inds;               /* [Q][D][GPDLA_POPULATION_MAX_LARGE] */
  double* large_probs;               /* [Q][D][GPDLA_POPULATION_MAX_LARGE] */
  int32_t* large_bins;               /* [Q][D][GPDLA_POPULATION_MAX_LARGE][GPDLA_MAX_DLAS] */
} gpdla_level_population;
/* gpdla_engine_process_population plus the reductions over every level; with levels NULL it is that call,
 * bit for bit, and with it every other result is unchanged bit for bit.  The new launches run per device
 * batch after its last level and the existing summary and population launches.  A half is asked for by its
 * arrays and either may be absent: bin_planes (it needs spec with a grid), or level_posteriors,
 * poisson_plane and large_* together (they need pspec, for the priors and the thresholds).  GPDLA_EINVAL for
 * levels without any array, a half without its spec, a null array of a half asked for or a bad memory kind;
 * GPDLA_EUNSUPPORTED on int8 and panel-GEMM engines. */
int gpdla_engine_process_levels(gpdla_engine* engine, const gpdla_spectra* spectra,
                                const gpdla_multi_dla* multi, const gpdla_sub_dla* sub,
                                const gpdla_results_multi* results_multi, const gpdla_results_sub* results_sub,
                                const gpdla_summary_spec* spec, const gpdla_summaries* summaries,
                                const gpdla_population_spec* pspec, const gpdla_population* population,
                                const gpdla_level_population* levels);
/* Cumulative kernel time (HIP events) and count of the level-population launches (a batch's launches are
 * one span) since create / reset_stats. */
int gpdla_engine_get_level_population_stats(gpdla_engine* engine, double* ms, int64_t* launches);
/* The level planes alone, host buffers, with gpdla_posterior_summary_f64's inputs: ll [levels][rows][ld],
 * base_inds [levels - 1][rows][ld] (NULL when levels = 1); spec must have a grid.  bin_planes is
 * [rows][levels][GPDLA_SUMMARY_PLANES][nz][nn]. */
int gpdla_level_planes_f64(int32_t device, const double* ll, int64_t rows, int64_t S, int64_t ld,
                           const double* offset_samples, const double* log_nhi_samples, const double* nhi_samples,
                           const double* min_z, const double* max_z, const int32_t* base_inds, int32_t levels,
                           const gpdla_summary_spec* spec, double* bin_planes);
/* The level split alone, host buffers: as above plus level_posteriors [levels][rows] (an input: each in
 * [0, 1] or NaN) and the grid and thresholds of spec (its priors and log_nhi_samples are not read).
 * Outputs as in gpdla_level_population with D = levels, Q = rows. */
int gpdla_population_split_levels_f64(int32_t device, const double* ll, int64_t rows, int64_t S, int64_t ld,
                                      const double* offset_samples, const double* log_nhi_samples,
                                      const double* min_z, const double* max_z, const int32_t* base_inds,
                                      int32_t levels, const double* level_posteriors,
                                      const gpdla_population_spec* spec, double* poisson_plane,
                                      int32_t* large_inds, double* large_probs, int32_t* large_bins);

/* ---- Posterior intervals ----------------------------------------------------
 * Marginal posterior summaries of z_DLA and log N_HI for every absorber of every level: what
 * DLACatalogue.find_delta_NHI / find_delta_z (CDDF_analysis/calc_cddf.py:872-886) start, for all levels
 * and with moments and quantiles.  Row q, level d in 1..D, slot u in 0..d-1.  c_u(j) is the chain of
 * sample j exactly as the MAP pairs form it (c_0 = j, then the base indices); a sample whose chain is
 * void (a -1 or an index outside [0, S) on the way) contributes to nothing below.  pi_j = w_j / W as in
 * the summaries.  The slot's values are
 *   x^z_j = min_z + (max_z - min_z) * offset[c_u(j)]  (product and sum rounded separately),
 *   x^N_j = log_nhi[c_u(j)].
 * Per (q, d, u) and parameter:
 *   lr_ranges   min and max of x over the non-NaN samples with l_j > m - lr_delta (m the row's maximum,
 *               the difference rounded once, the comparison strict); lr_counts [D][Q] the number of such
 *               samples.  Exact reductions.  NaN, NaN when there is none.
 *   means, sds  mean = sum pi x / T, sd = sqrt(sum pi (x - mean)^2 / T), T = sum pi over the valid-chain
 *               samples; the second sum is a second pass centred on the computed mean.  Every sum is formed
 *               in the order of W: strided per-thread partials, xor butterfly, waves in order.  NaN when
 *               T is 0.
 *   quantiles   per level p in levels[]: the smallest value x* of the slot whose cumulative mass
 *               F(x*) = sum_{x_j <= x*} pi_j reaches p T_c.  The masses are summed per dense rank of the
 *               value (equal values share a rank) in sample-index order, first over coarse bins rank >> s
 *               (s the smallest shift that leaves at most 1,024 bins of S ranks), then over the 2^s ranks
 *               of the coarse bin each level selects; the cdf is a fixed-order scan of the bins (four bins
 *               per thread in order, the 256 thread sums by a 64-lane shift scan, the 4 waves in order),
 *               T_c the coarse scan's total, and the fine scan starts from the coarse scan's partial.  The
 *               bin taken is the first non-empty one whose cdf reaches the target; if rounding leaves none,
 *               the last non-empty one (gpdla_resample_f64's rule).  x* is bitwise one of the slot's values.
 *               NaN when T_c is 0.
 * A row whose W is 0 or not finite gives NaN everywhere and a count of 0; slots >= d are NaN.  If min_z or
 * max_z is not finite, or max_z < min_z, the row's z outputs are NaN and the log N_HI outputs are still
 * computed; min_z == max_z is legal.  offset_samples and log_nhi_samples must be finite.  S <=
 * GPDLA_INTERVAL_MAX_SAMPLES.  A row's outputs are a function of the row alone: repeated calls, any split
 * into device batches, host or device results and runs with or without the sample buffers agree bit for
 * bit. */
#define GPDLA_INTERVAL_MAX_LEVELS 8
#define GPDLA_INTERVAL_MAX_SAMPLES (1 << 20)
typedef struct gpdla_interval_spec {
  const double* log_nhi_samples;     /* host [S], the samples' log10 N_HI in the caller's order */
  double lr_delta;                   /* > 0, finite (the reference's 2) */
  int32_t num_levels;                /* 1..GPDLA_INTERVAL_MAX_LEVELS */
  double levels[GPDLA_INTERVAL_MAX_LEVELS];  /* strictly inside (0, 1), strictly increasing */
} gpdla_interval_spec;

typedef struct gpdla_intervals {
  int32_t memory;                    /* GPDLA_MEM_HOST or GPDLA_MEM_DEVICE */
  double* z_means;                   /* [D][Q][GPDLA_MAX_DLAS] */
  double* z_sds;
  double* log_nhi_means;
  double* log_nhi_sds;
  double* z_lr_ranges;               /* [D][Q][GPDLA_MAX_DLAS][2]: min, max */
  double* log_nhi_lr_ranges;
  double* z_quantiles;               /* [D][Q][GPDLA_MAX_DLAS][num_levels] */
  double* log_nhi_quantiles;
  int32_t* lr_counts;                /* [D][Q] */
} gpdla_intervals;

/* gpdla_engine_process_summaries with the interval launches after the summary launch of each device batch;
 * every other result is that call's, bit for bit.  spec's grid stays optional and the sample arrays of
 * results may be NULL.  GPDLA_EINVAL for a null ispec, intervals or array of either, lr_delta <= 0 or not
 * finite, num_levels outside 1..GPDLA_INTERVAL_MAX_LEVELS, a level outside (0, 1), levels not strictly
 * increasing, or more than GPDLA_INTERVAL_MAX_SAMPLES samples. */
int gpdla_engine_process_intervals(gpdla_engine* engine, const gpdla_spectra* spectra,
                                   const gpdla_multi_dla* multi, const gpdla_results_multi* results,
                                   const gpdla_summary_spec* spec, const gpdla_summaries* summaries,
                                   const gpdla_interval_spec* ispec, const gpdla_intervals* intervals);
/* Cumulative kernel time (HIP events) and count of the interval launches since create / reset_stats. */
int gpdla_engine_get_interval_stats(gpdla_engine* engine, double* ms, int64_t* launches);
/* The interval kernel alone, host buffers, with gpdla_posterior_summary_f64's inputs (ispec's
 * log_nhi_samples is not read here); outputs as in gpdla_intervals with D = levels, Q = rows, in host
 * memory. */
int gpdla_posterior_intervals_f64(int32_t device, const double* ll, int64_t rows, int64_t S, int64_t ld,
                                  const double* offset_samples, const double* log_nhi_samples,
                                  const double* min_z, const double* max_z, const int32_t* base_inds,
                                  int32_t levels, const gpdla_interval_spec* ispec,
                                  const gpdla_intervals* intervals);

/* voigt MEX replacement (voigt.c:253-304).  Host buffers.  out has n_padded - 6 values. */
int gpdla_voigt_f64(const double* lambdas, int64_t n_padded, double z, double N,
                    int32_t num_lines, double* out);
/* Batched form: out[s*(n_padded-6) + i] for `count` (z, N) pairs over one padded grid. */
int gpdla_voigt_batch_f64(const double* lambdas, int64_t n_padded, const double* z,
                          const double* N, int64_t count, int32_t num_lines, double* out);
/* log N(y; mu, M M' + diag(d)) (log_mvnpdf_low_rank.m:5-33).  Host buffers, M n x k column-major. */
int gpdla_log_mvnpdf_low_rank_f64(const double* y, const double* mu, const double* M,
                                  const double* d, int64_t n, int32_t k, double* out);

/* ---- GP null-model training objective ----------------------------------------
 * objective.m: f(x) = sum_i spectrum_loss(...) and its gradient g(x), with
 *   x = [M(:) (num_pixels x k, column-major); log_omega (num_pixels); log_c_0; log_tau_0; log_beta]
 * (objective.m:21-30).  The training data are the matrices of learn_qso_model.m:63-84,
 * num_quasars x num_pixels, ROW-major here (row i = quasar i; NaN = missing pixel, objective.m:43).
 * As in the reference, the tau_0 and beta priors enter g only, not f (objective.m:59-71).
 * gpdla_objective_create copies host data to the device (memory = GPDLA_MEM_HOST) or borrows
 * device arrays (GPDLA_MEM_DEVICE, which must outlive the handle); each _eval takes host x and
 * writes host f and g (g may be NULL).  num_pixels <= 4096, k <= 64.  Spectra go through the
 * kernels in launches of up to 2^29 doubles of workspace; the environment variable
 * GPDLA_OBJECTIVE_BATCH (read at create) caps the spectra per launch further. */
typedef struct gpdla_objective gpdla_objective;
int gpdla_objective_create(int32_t device, int64_t num_quasars, int64_t num_pixels, int32_t k,
                           const double* centered_rest_fluxes, const double* lya_1pzs,
                           const double* rest_noise_variances, int32_t memory, gpdla_objective** out);
int gpdla_objective_eval(gpdla_objective* objective, const double* x, double* f, double* g);
void gpdla_objective_destroy(gpdla_objective* objective);
/* spectrum_loss.m:14-76 for one spectrum (host buffers): n pixels, M n x k column-major, omega2
 * per pixel.  Any gradient output may be NULL. */
int gpdla_spectrum_loss_f64(const double* y, const double* lya_1pz, const double* noise_variance,
                            const double* M, const double* omega2, int64_t n, int32_t k, double c_0,
                            double tau_0, double beta, double* nlog_p, double* dM, double* dlog_omega,
                            double* dlog_c_0, double* dlog_tau_0, double* dlog_beta);

/* ---- The Lyman-series forest in the training objective ------------------------
 * The null model gpdla_engine_set_forest evaluates with variance_series, as the objective: spectrum_loss's
 * optical depth tau_0 lya_1pz^beta (spectrum_loss.m:23) becomes the series sum above,
 *   tau = sum_{i=1..L} t_i(tau_0, beta)   at   lambda = lya_1pz lambda_1,   z_QSO the spectrum's own,
 * by the same device function, comparison and line order; d tau / d log tau_0 = tau and
 * d tau / d log beta = beta sum_i t_i log(1 + z_i) enter the gradient.  Everything else is objective.m.
 * gpdla_objective_set_forest copies z_qsos[num_quasars] (host or device memory) and applies to every later
 * _eval; z_qsos = NULL restores the Lya-only objective.  GPDLA_EINVAL for num_forest_lines outside 1..31,
 * a bad memory kind or a non-finite z. */
int gpdla_objective_set_forest(gpdla_objective* objective, const double* z_qsos, int32_t memory,
                               int32_t num_forest_lines);
/* gpdla_spectrum_loss_f64 under the series, for one spectrum at z_qso. */
int gpdla_spectrum_loss_forest_f64(const double* y, const double* lya_1pz, const double* noise_variance,
                                   const double* M, const double* omega2, int64_t n, int32_t k, double c_0,
                                   double tau_0, double beta, double z_qso, int32_t num_forest_lines,
                                   double* nlog_p, double* dM, double* dlog_omega, double* dlog_c_0,
                                   double* dlog_tau_0, double* dlog_beta);
/* sum_i t_i(tau_0, beta) for a num_quasars x num_pixels row-major matrix of 1 + z_Lya (host buffers), row q
 * at z_qsos[q] and lambda = lya_1pz lambda_1: gpdla_forest_f64's sum, one block per row.  NaN in gives NaN
 * out.  exp(-out) with Kim et al.'s tau_0, beta is the mean flux the training preparation divides out. */
int gpdla_forest_rows_f64(int32_t device, const double* lya_1pzs, const double* z_qsos, int64_t num_quasars,
                          int64_t num_pixels, double tau_0, double beta, int32_t num_forest_lines, double* out);

/* ---- DLA parameter samples ------------------------------------------------------
 * generate_dla_samples.m:8-57 on the device: the RR2-scrambled Halton points (:8-9), ksdensity of the
 * catalogue's column densities on the 1,000-point fit grid at MATLAB's default bandwidth (:32-33), the
 * quadratic log-density fit (:34, host QR) normalised over [fit_min, fit_upper] (:37-38) and the inverse
 * mixture CDF of every sample's second Halton coordinate (:42-55, fzero), nhi = 10^log_nhi (:57).
 * Host buffers.  The prior's fields are set_parameters.m:49-53's (0.9, 20, 23, 20, 22) and the 25.0 of
 * generate_dla_samples.m:38. */
typedef struct gpdla_dla_prior {
  double alpha;                    /* weight of the fitted component (set_parameters.m:49) */
  double uniform_min, uniform_max; /* uniform component of log10 N_HI (:50-51) */
  double fit_min, fit_max;         /* KDE / fit range (:52-53) */
  double fit_upper;                /* upper limit of the normalising integral (generate_dla_samples.m:38) */
} gpdla_dla_prior;
/* Points start, start + stride, ... (num of them) of the RR2-scrambled Halton sequence in `dims` bases
 * (haltonset(dims, 'Skip', start, 'Leap', stride - 1) + scramble(..., 'RR2'); index 0 is the origin):
 * out[j * dims + d], bit-exact.  Bases 2..64, dims <= 16. */
int gpdla_halton_rr2_f64(int32_t device, int64_t start, int64_t stride, int64_t num, const int32_t* bases,
                         int32_t dims, double* out);
/* log_nhis: the catalogue's n_data column densities (the non-empty cells concatenated, :26-28).
 * Writes num_samples offsets, log10 N_HI and N_HI samples; fit (may be NULL) receives the polyfit
 * coefficients c2, c1, c0, the normaliser Z and the KDE bandwidth.  GPDLA_ENUMERIC when the density
 * estimate vanishes on the fit grid or the fit does not normalise. */
int gpdla_generate_dla_samples_f64(int32_t device, const double* log_nhis, int64_t n_data, int64_t num_samples,
                                   const gpdla_dla_prior* prior, double* offset_samples, double* log_nhi_samples,
                                   double* nhi_samples, double* fit);

/* ---- Spectrum ingest -----------------------------------------------------------
 * read_spec.m:27-38 and preload_qsos.m:18-67 on the device, over the fitsread columns of a catalogue
 * (FITS parsing stays on the host).  Host buffers.  Thresholds are compared exactly (the defaults are
 * all representable in single); brightsky_bit is read_spec.m:9's 1-based bit of the and_mask (24). */
typedef struct gpdla_preload_params {
  double normalization_min_lambda, normalization_max_lambda;   /* set_parameters.m:29-30 (1310, 1325) */
  double min_lambda, max_lambda;                               /* :33-34 (911.75, 1215.75) */
  double loading_min_lambda, loading_max_lambda;               /* :21-22 (910, 1217) */
  int32_t min_num_pixels;                                      /* :26 (200) */
  int32_t brightsky_bit;                                       /* read_spec.m:9 (24) */
} gpdla_preload_params;
/* wavelengths = 10.^loglam (single, correctly rounded), noise_variance = 1 ./ ivar,
 * pixel_mask = ivar == 0 | bitget(and_mask, 24) (read_spec.m:27-38), elementwise over n pixels. */
int gpdla_read_spec_f32(int32_t device, int64_t n, const float* loglam, const float* ivar, const int32_t* and_mask,
                        float* wavelengths, float* noise_variance, uint8_t* pixel_mask);
/* preload_qsos.m:18-67 over num_quasars spectra in CSR (offsets[Q + 1], offsets[0] = 0; the fitsread
 * columns flux, loglam, ivar, and_mask; z_qsos[Q]).  filter_flags[Q] (in/out): entries > 0 are skipped;
 * bit 3 (4) / bit 4 (8) are set for an unnormalisable spectrum / too few pixels.  Out: the cells in CSR
 * (out_offsets[Q + 1]; each out_* array needs offsets[Q] entries at most), normalizers[Q] (0 where not
 * loaded) and, if not NULL, medians[Q] (the single normalisation median, NaN where undefined). */
int gpdla_preload_qsos_f32(int32_t device, int64_t num_quasars, const int64_t* offsets, const float* flux,
                           const float* loglam, const float* ivar, const int32_t* and_mask, const double* z_qsos,
                           const gpdla_preload_params* params, uint8_t* filter_flags, int64_t* out_offsets,
                           float* out_wavelengths, float* out_flux, float* out_noise_variance,
                           uint8_t* out_pixel_mask, double* normalizers, float* medians);

/* ---- Bootstrap sample errors -----------------------------------------------------
 * calc_cddf.py's resample / get_sample_errors (:126-184): replicas of the sightline sample drawn with
 * replacement, stratified by redshift, and the population sums of every replica.  A replica is a vector of
 * multiplicities counts[Q]; its sums are the product sums[B][N] = counts[B][Q] rows[Q][N] on the f64 matrix
 * cores, with rows the per-spectrum terms catalog.cddf_moments accumulates plus the path columns.
 *
 *   strata   CSR: stratum s holds the spectra members[stratum_offsets[s] .. stratum_offsets[s + 1]) (n_s >= 1
 *            of them, every spectrum in at most one stratum); spectra in no stratum are never drawn
 *   draws    Philox4x64-10 keyed by seed[0..1], stateless: draw g (a position in members) of replica r uses
 *            counter (g >> 2, 0, r, 0), output word g & 3.  With u that word and s the stratum holding g, the
 *            drawn spectrum is members[stratum_offsets[s] + mulhi64(u, n_s)] (bias n_s / 2^64).  Replica r is
 *            first_replica + its index in the call, so a call's replicas depend on nothing else in it
 *   sums     the reduction order over the spectra is a function of Q and the constants of
 *            gpdla_bootstrap_tiling alone: a replica's sums do not depend on B, on first_replica, on the
 *            chunking or on the other replicas (bit for bit); split-K partials are added in ascending order */
typedef struct gpdla_bootstrap_spec {
  uint64_t seed[2];                  /* the Philox key */
  int64_t num_replicas;              /* B >= 1 */
  int64_t first_replica;             /* >= 0 */
  int32_t num_strata;                /* >= 1 */
  const int64_t* stratum_offsets;    /* host [num_strata + 1], from 0, strictly increasing */
  const int32_t* members;            /* host [stratum_offsets[num_strata]], each in 0..Q-1, none twice */
} gpdla_bootstrap_spec;
/* The compile-time shape of the sums kernel: replicas and columns per block tile, spectra per K stage,
 * spectra per split-K slice, most replicas per device chunk. */
int gpdla_bootstrap_tiling(int32_t* tile_m, int32_t* tile_n, int32_t* stage_k, int32_t* k_slice,
                           int32_t* max_chunk);
/* counts[B][Q] (host) of spec's replicas: a row sums to the member count, a stratum's part of it to n_s.
 * gpdla_last_call_kernel_ms: one span per replica chunk.  GPDLA_EINVAL for B < 1, Q < 1, a member outside
 * 0..Q-1 or listed twice, an empty stratum, first_replica < 0. */
int gpdla_bootstrap_counts_i32(int32_t device, int64_t Q, const gpdla_bootstrap_spec* spec, int32_t* counts);
/* The four moment planes of every spectrum (host buffers), rows[q ld_rows + 0 .. 4 nz nn): p A and
 * p B - p p C of catalog.cddf_moments for moment = False, then the same pair for moment = True, every
 * product and the difference rounded separately (no FMA), so they equal numpy's bit for bit.  planes is
 * [Q][D][GPDLA_SUMMARY_PLANES][nz nn].  level_posteriors NULL (D must be 1): p = p_dlas.  Otherwise [Q][D] and a
 * row is sum_d P_d A_d and sum_d (P_d B_d - P_d P_d C_d) from 0.0, d ascending, NaN P_d skipped.  A spectrum
 * with p_dlas <= p_thresh_spec or NaN, or keep (NULL: all kept) 0, gets zeros.  The columns from 4 nz nn on
 * are not written.  One span per spectrum chunk.  GPDLA_EINVAL for Q < 1, D outside 1..GPDLA_MAX_DLAS, a
 * malformed grid, ld_rows < 4 nz nn. */
int gpdla_bootstrap_rows_f64(int32_t device, const double* planes, int32_t D, const double* p_dlas,
                             const double* level_posteriors, const uint8_t* keep, int64_t Q, int32_t nz, int32_t nn,
                             double p_thresh_spec, double* rows, int64_t ld_rows);
/* sums[B][N] = counts[B][Q] rows[Q][N] (host buffers) from the caller's counts.  Two spans per replica chunk
 * (the product, the split-K reduction).  GPDLA_EINVAL for B, Q or N < 1, a negative count, a non-finite row
 * entry. */
int gpdla_bootstrap_sums_f64(int32_t device, const int32_t* counts, const double* rows, int64_t B, int64_t Q,
                             int64_t N, double* sums);
/* The counts made and used on the device, in replica chunks sized from free memory: bit for bit
 * gpdla_bootstrap_counts_i32 followed by gpdla_bootstrap_sums_f64.  Three spans per chunk (draws, product,
 * reduction).  The GPDLA_EINVAL cases of both. */
int gpdla_bootstrap_f64(int32_t device, const double* rows, int64_t Q, int64_t N, const gpdla_bootstrap_spec* spec,
                        double* sums);

/* ---- Per-spectrum SNR (calc_cddf.py find_snr, :906-924) ------------------------------------------------
 * Over the pixels with wavelength > 1215.67 (1 + max_z_dlas[q]) (compared in double): the flux is floored --
 * with normalizers, flux / norm < 0.1 (in double) sets it to norm 0.1 (formed in double, rounded to the
 * cells' class); without, flux < 0.1 sets it to 0.1 -- the ratio sqrt(noise_variance) / |flux|, numpy's
 * median of it (the mean of the two middle values for an even count) and snr = 1 / median are formed in the
 * cells' own class.  Any NaN ratio gives NaN, and so does an empty set.  Spectrum q's pixels are
 * offsets[q] .. offsets[q + 1].  One span.  GPDLA_EINVAL for Q < 1 or offsets not ascending from 0. */
int gpdla_spectrum_snrs_f32(int32_t device, int64_t Q, const int64_t* offsets, const float* wavelengths,
                            const float* flux, const float* noise_variance, const double* max_z_dlas,
                            const double* normalizers, float* snrs);
int gpdla_spectrum_snrs_f64(int32_t device, int64_t Q, const int64_t* offsets, const double* wavelengths,
                            const double* flux, const double* noise_variance, const double* max_z_dlas,
                            const double* normalizers, double* snrs);

/* ---- Search cuts: proximity zone and noisy pixels --------------------------------
 * calc_cddf.py's `lowzcut` (:352, :739-741) and `filter_noisy_pixels` (:387-438, :746-747, :934) as one
 * launch over CSR spectra: per spectrum q, with min_z / max_z its search range and span = max_z - min_z,
 * every operation in double and rounded on its own (no FMA):
 *   pixels      those with 1215.67 (1 + min_z) < wavelength < 1215.67 (1 + max_z) (both strict), in pixel
 *               order, pixel_counts[q] = n of them; the pixel mask is not consulted.  Pixel i of them is good
 *               when noise_variance < noise_thresh (NaN, +inf and equality are bad); with the pixel cut off
 *               (noise_thresh NaN) every one is good.  bitmap_words holds the good flags, bit i of the
 *               spectrum's stretch (word i / 32, bit i % 32), the stretch starting at word bitmap_offsets[q]
 *               and ceil(len_q / 32) words long; the bits from n on are 0
 *   z_uppers    max(max_z - proximity_zone, min_z), or max_z with the proximity cut off (proximity_zone NaN)
 *   samples     the reductions given these results (gpdla_sample_cuts below) put an absorber slot at
 *               redshift z into a bin only if z < z_upper (proximity cut on) and pixel
 *               (int)(((z - min_z) / span) n) is good (pixel cut on; this operation order, truncated; an index
 *               outside [0, n), a NaN, n = 0 or span = 0 excludes the slot).  Nothing else about a sample
 *               changes: its mass still counts in W, a void chain still voids it, and a surviving slot of a
 *               multi-DLA sample counts though a sibling is cut
 *   path        per grid given, nz + 1 values per spectrum: bins [e_c, e_c+1], then the whole extent
 *               [e_0, e_nz].  For [z_lo, z_hi]: 0 unless min_z < z_hi and z_upper > z_lo; pmin = max(z_lo,
 *               min_z), pmax = min(z_hi, z_upper); X(pmax) - X(pmin) when every pixel is good (n >= 1) or the
 *               pixel cut is off; 0 when n = 0, or n = 1 with its pixel bad; otherwise with zz_i = min_z +
 *               (span i) / (n - 1) the sum over the starts -- pixels i < n - 1, good, pmin <= zz_i <= pmax, and
 *               i = 0 or pixel i - 1 not (good with zz >= pmin) -- of X(zz_(e-1)) - X(zz_i) when e, the first
 *               bad pixel after i, exists and zz_e < pmax, else X(pmax) - X(zz_i).  X(z) = 2 sqrt(omega_m
 *               (1 + z)^3 + 1 - omega_m) / (3 omega_m), the cube as two products.  The terms are added as
 *               strided per-thread partial sums in pixel order, a 64-lane xor butterfly and the waves in
 *               order: fixed by n alone
 * No floating-point atomics; a spectrum's outputs are a function of the spectrum alone, so repeated calls
 * and any batching agree bit for bit. */
typedef struct gpdla_search_cuts {
  double proximity_zone;             /* finite and >= 0 (calc_cddf.py: 0.1), or NaN: off */
  double noise_thresh;               /* NaN: off */
  double omega_m;                    /* in (0, 1]; read only with a grid */
  int32_t num_z_bins_summary;        /* 0: no summary grid */
  const double* z_edges_summary;     /* host [nz + 1], finite, strictly increasing */
  int32_t num_z_bins_population;     /* 0: no population grid */
  const double* z_edges_population;
} gpdla_search_cuts;

typedef struct gpdla_search_cut_results {
  int32_t memory;                    /* GPDLA_MEM_HOST; gpdla_engine_process_cuts also takes GPDLA_MEM_DEVICE */
  double* z_uppers;                  /* [Q] */
  int32_t* pixel_counts;             /* [Q] */
  int64_t* bitmap_offsets;           /* [Q + 1], written: sum over the spectra before q of ceil(len / 32) */
  uint32_t* bitmap_words;            /* [sum_q ceil(len_q / 32)] */
  double* path_summary;              /* [Q][nz + 1], or NULL without the summary grid */
  double* path_population;           /* [Q][nz_p + 1], or NULL without the population grid */
} gpdla_search_cut_results;

/* The kernel alone, host buffers: spectrum q's pixels are offsets[q] .. offsets[q + 1].  One span.
 * GPDLA_EINVAL for Q < 1, offsets not ascending from 0, both thresholds NaN, a negative or infinite
 * proximity_zone, a malformed grid, omega_m outside (0, 1] with a grid, a grid without its path array or a
 * path array without its grid, a null array, or memory other than GPDLA_MEM_HOST. */
int gpdla_search_cuts_f64(int32_t device, int64_t Q, const int64_t* offsets, const double* wavelengths,
                          const double* noise_variance, const double* min_z, const double* max_z,
                          const gpdla_search_cuts* cuts, const gpdla_search_cut_results* results);

/* What the reductions read of a cut (host arrays): the outputs above, row r of the reduction being spectrum r. */
typedef struct gpdla_sample_cuts {
  const double* z_uppers;            /* [rows], or NULL: no proximity test */
  const int32_t* pixel_counts;       /* [rows], or NULL: no pixel test */
  const int64_t* bitmap_offsets;     /* [rows + 1] with pixel_counts: ascending from 0 */
  const uint32_t* bitmap_words;      /* [bitmap_offsets[rows]] */
} gpdla_sample_cuts;
/* gpdla_level_planes_f64 and gpdla_population_split_levels_f64 with the two sample tests above applied to every
 * absorber slot of every level (levels = 1: the level-1 rule).  cuts NULL: those calls, bit for bit.
 * GPDLA_EINVAL additionally for cuts with neither test, pixel_counts without the bitmap, offsets not ascending
 * from 0, or a pixel count outside [0, 32 words of the row]. */
int gpdla_level_planes_cut_f64(int32_t device, const double* ll, int64_t rows, int64_t S, int64_t ld,
                               const double* offset_samples, const double* log_nhi_samples, const double* nhi_samples,
                               const double* min_z, const double* max_z, const int32_t* base_inds, int32_t levels,
                               const gpdla_summary_spec* spec, const gpdla_sample_cuts* cuts, double* bin_planes);
int gpdla_population_split_levels_cut_f64(int32_t device, const double* ll, int64_t rows, int64_t S, int64_t ld,
                                          const double* offset_samples, const double* log_nhi_samples,
                                          const double* min_z, const double* max_z, const int32_t* base_inds,
                                          int32_t levels, const double* level_posteriors,
                                          const gpdla_population_spec* spec, const gpdla_sample_cuts* cuts,
                                          double* poisson_plane, int32_t* large_inds, double* large_probs,
                                          int32_t* large_bins);

/* gpdla_engine_process_levels plus the search cuts: with cuts and results both NULL it is that call, bit for
 * bit; with them every output that is not a grid reduction (evidences, sample rows, MAP values, posteriors) is
 * unchanged bit for bit, and every grid reduction of the call -- gpdla_summaries.bin_planes, gpdla_population
 * and gpdla_level_population -- applies the sample tests.  The cut launch runs per device batch once min_z /
 * max_z exist and before the first grid reduction, on the batch's resident pixels; the noise variance is the
 * one the engine was given.  results may be host or device memory; the path grids are the cuts' own edge
 * arrays.  GPDLA_EINVAL for one of the two NULL and the other not, the gpdla_search_cuts_f64 cases, or a call
 * with neither a summary grid nor a population spec; GPDLA_EUNSUPPORTED with the sub-DLA model and on int8 and
 * panel-GEMM engines. */
int gpdla_engine_process_cuts(gpdla_engine* engine, const gpdla_spectra* spectra,
                              const gpdla_multi_dla* multi, const gpdla_sub_dla* sub,
                              const gpdla_results_multi* results_multi, const gpdla_results_sub* results_sub,
                              const gpdla_summary_spec* spec, const gpdla_summaries* summaries,
                              const gpdla_population_spec* pspec, const gpdla_population* population,
                              const gpdla_level_population* levels, const gpdla_search_cuts* cuts,
                              const gpdla_search_cut_results* results);
/* Cumulative kernel time (HIP events) and count of the search-cut launches since create / reset_stats. */
int gpdla_engine_get_cut_stats(gpdla_engine* engine, double* ms, int64_t* launches);

/* ---- Model spectra: absorption, GP continuum and goodness of fit on the pixels ---------
 * For spectrum q and its counts[q] absorbers (z_dlas[q][i], log_nhis[q][i], i < counts[q]; 0: the null model), on
 * the likelihood's n unmasked in-range pixels in pixel order, with mu, M, omega^2, y, sigma^2 as the sweeps see
 * them (after the forest launches when a forest is set):
 *   a       the product of the absorbers' Voigt profiles: num_lines lines, the padded grid and instrument
 *           broadening of gpdla_voigt_f64, each absorber broadened on its own, params.absorption_mode indexing
 *   d = a^2 omega^2 + sigma^2, r = y - a mu, V = diag(a) M, B = I + V'D^-1 V, u = V'D^-1 r, w = B^-1 u
 *   absorption a_j; model_mean a_j mu_j; continuum_mean mu_j + M_j w; continuum_sd sqrt(M_j B^-1 M_j'), the
 *   posterior sd of the low-rank continuum (the white omega term is not in it)
 *   chi2 = r'D^-1 r - u'B^-1 u = r'K^-1 r;  log_likelihood = -(chi2 + log det B + sum log d_j + n log 2 pi) / 2
 * Flux-like outputs are in the caller's units (a spectrum prep rescaled by a power of two is scaled back exactly).
 * The per-pixel arrays are ragged: spectrum q's n_q values go to cap_offsets[q] + 0 .. n_q - 1, pixel_inds being
 * each value's pixel index within the spectrum; num_pixels[q] = n_q.  cap_offsets[q + 1] - cap_offsets[q] must be
 * at least n_q (the spectrum's in-range pixel count is an upper bound); what lies between n_q and the capacity is
 * NaN / -1 with host results and untouched with device results.  A spectrum over its capacity is not written at
 * all (NaN scalars, its num_pixels) and the call returns GPDLA_EINVAL naming it; the other spectra are complete.
 * An absorber with a non-finite parameter gives NaN outputs for its spectrum, a spectrum without usable pixels NaN
 * scalars and n = 0.  GPDLA_ENUMERIC: a pivot of B was not positive (that spectrum's outputs are NaN).
 * Results are a function of the spectrum and its absorbers alone: repeated calls, any max_batch_spectra, host or
 * device memory agree bit for bit.  GPDLA_EUNSUPPORTED on int8 and panel-GEMM engines. */
typedef struct gpdla_model_absorbers {
  const int32_t* counts;             /* host [Q], 0..GPDLA_MAX_DLAS */
  const double* z_dlas;              /* host [Q][GPDLA_MAX_DLAS] */
  const double* log_nhis;            /* host [Q][GPDLA_MAX_DLAS], log10 N_HI */
  const double* nhis;                /* host [Q][GPDLA_MAX_DLAS] N_HI in cm^-2, or NULL: 10^log_nhis */
} gpdla_model_absorbers;

typedef struct gpdla_model_spectra {
  int32_t memory;                    /* GPDLA_MEM_HOST or GPDLA_MEM_DEVICE: where the arrays below live */
  const int64_t* cap_offsets;        /* host [Q + 1], ascending */
  int32_t* pixel_inds;               /* [cap_offsets[Q]] */
  double* absorption;
  double* model_mean;
  double* continuum_mean;
  double* continuum_sd;
  double* chi2;                      /* [Q] */
  double* log_likelihoods;           /* [Q] */
  int32_t* num_pixels;               /* [Q] */
  int32_t* levels;                   /* [Q] the level drawn, written by gpdla_engine_process_spectra_models only; or NULL */
} gpdla_model_spectra;

/* prep_kernel (and the forest launches when set) on the given spectra, then the model-spectra kernel with the
 * caller's absorbers: no search, no samples read. */
int gpdla_engine_model_spectra(gpdla_engine* engine, const gpdla_spectra* spectra,
                               const gpdla_model_absorbers* absorbers, const gpdla_model_spectra* results);
/* The same launch inside a search: gpdla_engine_process_summaries -- or, with ispec and intervals set (both or
 * neither), gpdla_engine_process_intervals -- (same arguments, same outputs bit for bit) and,
 * per device batch after the summary launch, on the panel the sweeps just used, the model of each spectrum's level:
 *   GPDLA_MODEL_LEVEL_BEST   the DLA level d in 1..max_dlas with the largest log_likelihoods_dla[d - 1][q] +
 *                            log_priors_dla[d - 1][q] (the level of the highest model posterior; first maximum, NaN
 *                            ignored, level 1 when all are NaN), taken on the device.  log_priors_dla may be NULL
 *                            with max_dlas = 1
 *   GPDLA_MODEL_LEVEL_GIVEN  levels[q] in 0..max_dlas (0: the null model)
 * The absorbers are level d's d MAP pairs of the summaries (gpdla_summaries.map_z_dlas / map_log_nhis), N_HI =
 * 10^log N_HI formed on the device exactly as gpdla_engine_model_spectra forms it without `nhis`, so the results are
 * bitwise those of that call fed the same pairs.  A level without a MAP sample gives NaN outputs.  results->levels
 * receives the level drawn.  Errors as gpdla_engine_model_spectra and gpdla_engine_process_summaries, and
 * GPDLA_EINVAL for a level outside 0..max_dlas, NULL levels, or BEST with max_dlas > 1 and no priors. */
#define GPDLA_MODEL_LEVEL_BEST 0
#define GPDLA_MODEL_LEVEL_GIVEN 1
typedef struct gpdla_model_levels {
  int32_t level_mode;                /* GPDLA_MODEL_LEVEL_* */
  const int32_t* levels;             /* host [Q] with GIVEN */
  const double* log_priors_dla;      /* host [max_dlas][Q] with BEST */
} gpdla_model_levels;
int gpdla_engine_process_spectra_models(gpdla_engine* engine, const gpdla_spectra* spectra, const gpdla_multi_dla* multi,
                                        const gpdla_results_multi* results_multi, const gpdla_summary_spec* spec,
                                        const gpdla_summaries* summaries, const gpdla_interval_spec* ispec,
                                        const gpdla_intervals* intervals, const gpdla_model_levels* levels,
                                        const gpdla_model_spectra* results);
/* Cumulative kernel time (HIP events) and count of the model-spectra launches since create / reset_stats. */
int gpdla_engine_get_model_spectra_stats(gpdla_engine* engine, double* ms, int64_t* launches);

/* ---- Count mixture: the total column of a redshift bin on a lattice -------------------
 * calc_cddf.py's _get_omega_confidence_intervals (:562-636) combines the count distributions of a redshift
 * bin's column-density bins into the distribution of T = sum_b n_b N_b.  Here T lives on a dense fp64 lattice of
 * `cells` entries that starts as delta at cell 0, and a problem (one redshift bin) is a chain of stages, each a
 * sparse pmf of taps (shift_i, p_i):
 *   stage    next[g] = sum_i p_i cur[g - shift_i], one FMA chain per cell in ascending i, terms with g < shift_i
 *            absent.  Two taps of a stage may share a shift.  A cell's value depends on its problem's taps alone:
 *            not on the other problems of the call, on GPDLA_MIX_TILE or on GPDLA_MIX_TAPS
 *   cdf      the inclusive prefix sum of the final lattice, in an order that cells and GPDLA_MIX_TILE fix; it
 *            never decreases
 *   levels   per level l in (0, 1): lower_cells = the first cell with cdf >= l; upper_cells = the first occupied
 *            (pmf > 0) cell strictly above the first cell with cdf > l (the reference's "one past" upper end,
 *            :986-1019); either is the last occupied cell where no such cell exists (:634-635), and 0 for a
 *            lattice without mass.  mass = the cdf's last value (the levels are not rescaled by it)
 * Inputs are host arrays in CSR form: problem p holds the stages stage_offsets[p] .. stage_offsets[p + 1] (none:
 * the delta itself), stage s the taps tap_offsets[s] .. tap_offsets[s + 1].  Outputs: lower_cells / upper_cells
 * [num_problems][num_levels], mass [num_problems] and, unless NULL, pmf [num_problems][cells], the final
 * lattices.  GPDLA_EINVAL for a negative shift or one below its predecessor in the stage, a negative or
 * non-finite probability, an empty stage, cells outside 1..GPDLA_MIX_MAX_CELLS, a problem whose summed largest
 * shifts reach `cells`, a level outside (0, 1), more than GPDLA_MIX_MAX_LEVELS levels or 65535 problems.
 * Workspace: 16 bytes per problem and cell.  gpdla_last_call_kernel_ms then reports 3 spans: the stage launches
 * (one per stage index, over the cells that can be non-zero by then), the scan, the search. */
#define GPDLA_MIX_MAX_LEVELS 8
#define GPDLA_MIX_MAX_CELLS (1 << 28)
int gpdla_count_mixture_f64(int32_t device, const double* probs, const int32_t* shifts, const int64_t* tap_offsets,
                            const int64_t* stage_offsets, int64_t num_problems, int64_t cells, const double* levels,
                            int32_t num_levels, int32_t* lower_cells, int32_t* upper_cells, double* mass, double* pmf);
/* GPDLA_MIX_TILE, GPDLA_MIX_TAPS (csrc/tuning.h) and GPDLA_MIX_MAX_LEVELS of this build. */
int gpdla_count_mixture_tiling(int32_t* tile, int32_t* taps, int32_t* max_levels);

/* Diagnostics (test support; not used by the compute path).
 * Re/Im of the Faddeeva function the line tables are fitted from (host, long double). */
int gpdla_diag_faddeeva_w(double x, double y, double* re, double* im);
/* Max relative error of the fitted profile table of `line` against its long-double source. */
int gpdla_diag_line_table_error(int32_t line, double* max_rel_err);
/* The panel-GEMM weights kernels' raw 3-line absorption exp(-N sum_j lc_j V_j) (before the
 * instrument broadening) at n wavelengths, on the device: f32 = 1 the 24-bit path's packed-fp32
 * profile, f32 = 0 the fp64 one (gemm_i8.hip).  GPDLA_EDEVICE without a device. */
int gpdla_diag_raw_profile3(const double* lambdas, int64_t n, double z, double N, int32_t f32, double* out);

/* Device buffers for callers without a GPU array library (the benchmark, tests, C callers).
 * Callers that already hold device memory (e.g. PyTorch tensors) pass those pointers instead. */
int gpdla_device_malloc(int32_t device, int64_t bytes, void** ptr);
int gpdla_device_free(int32_t device, void* ptr);
int gpdla_memcpy_htod(int32_t device, void* dst, const void* src, int64_t bytes);
int gpdla_memcpy_dtoh(int32_t device, void* dst, const void* src, int64_t bytes);

const char* gpdla_last_error(void);
int32_t gpdla_version(void);
int32_t gpdla_device_count(void);
/* PCI bus id ("dddd:bb:dd.f") of a device, into buf (len >= 13): which physical GPU a rank drives
 * (the multi-GPU bench reports it per rank; process_qsos.m:88's spectra loop split over devices). */
int gpdla_device_pci_bus_id(int32_t device, char* buf, int32_t len);
/* Kernel times (ms, HIP events) of the calling thread's last call of gpdla_read_spec_f32,
 * gpdla_preload_qsos_f32, gpdla_halton_rr2_f64, gpdla_generate_dla_samples_f64,
 * gpdla_poisson_binomial_pmf_f64 or gpdla_count_mixture_f64, one per launch in launch order: read_spec 1;
 * preload_qsos 3 (range keys, scan, write); halton 1; generate 3 (KDE, Halton, inverse CDF); pmf 2 (chunks, all
 * fold steps); count_mixture 3 (all stage launches, scan, search); the bootstrap and SNR calls as
 * their comments say (the first 8 spans of a call are kept).  *count = launches recorded (0 for an empty call); at most capacity copied. */
int gpdla_last_call_kernel_ms(double* ms, int32_t capacity, int32_t* count);

#ifdef __cplusplus
}
#endif
#endif /* GPDLA_H */
