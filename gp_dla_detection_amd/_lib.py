"""ctypes binding of ``libgpdla.so`` (include/gpdla.h).

The library is built in-tree (``__graft_entry__.build()`` / ``python -m gp_dla_detection_amd.build``).
There is no CPU fallback: if the library is missing or no HIP device is present, compute calls
raise.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

LIB_PATH = Path(os.environ.get("GPDLA_LIB") or Path(__file__).resolve().parent / "libgpdla.so")

GPDLA_OK = 0
GPDLA_ENUMERIC = 1
GPDLA_EINVAL = -1
GPDLA_EDEVICE = -2
GPDLA_ENOMEM = -3
GPDLA_EUNSUPPORTED = -4
MEM_HOST = 0
MEM_DEVICE = 1
ABSORPTION_REFERENCE = 0
ABSORPTION_UNMASKED = 1
PATH_AUTO = 0
PATH_FUSED = 1
PATH_PANEL_GEMM = 2
PATH_FUSED_I8 = 3
PATH_PANEL_GEMM_I8 = 4
PATH_PANEL_GEMM_I8_24 = 5

dp = C.POINTER(C.c_double)
i64p = C.POINTER(C.c_int64)
u8p = C.POINTER(C.c_uint8)
i32p = C.POINTER(C.c_int32)
fp = C.POINTER(C.c_float)
u32p = C.POINTER(C.c_uint32)


class Model(C.Structure):
    _fields_ = [("num_rest", C.c_int32), ("k", C.c_int32), ("rest_wavelengths", dp), ("mu", dp),
                ("M", dp), ("log_omega", dp), ("log_c_0", C.c_double), ("log_tau_0", C.c_double),
                ("log_beta", C.c_double)]


class Samples(C.Structure):
    _fields_ = [("num_samples", C.c_int64), ("offset_samples", dp), ("nhi_samples", dp)]


class Params(C.Structure):
    _fields_ = [("num_lines", C.c_int32), ("width", C.c_int32), ("pixel_spacing", C.c_double),
                ("min_lambda", C.c_double), ("max_lambda", C.c_double),
                ("lya_wavelength", C.c_double), ("lyman_limit", C.c_double),
                ("min_z_cut", C.c_double), ("max_z_cut", C.c_double),
                ("absorption_mode", C.c_int32), ("max_batch_spectra", C.c_int32),
                ("path", C.c_int32)]


class Spectra(C.Structure):
    _fields_ = [("memory", C.c_int32), ("num_spectra", C.c_int64), ("offsets", i64p),
                ("wavelengths", dp), ("flux", dp), ("noise_variance", dp), ("pixel_mask", u8p),
                ("z_qsos", dp)]


class Results(C.Structure):
    _fields_ = [("memory", C.c_int32), ("log_likelihoods_no_dla", dp),
                ("sample_log_likelihoods_dla", dp), ("sample_ld", C.c_int64),
                ("log_likelihoods_dla", dp), ("min_z_dlas", dp), ("max_z_dlas", dp),
                ("num_pixels", i32p)]


class Stats(C.Structure):
    _fields_ = [("prep_ms", C.c_double), ("likelihood_ms", C.c_double), ("reduce_ms", C.c_double),
                ("prep_launches", C.c_int64), ("likelihood_launches", C.c_int64),
                ("reduce_launches", C.c_int64), ("spectra", C.c_int64), ("sample_evals", C.c_int64),
                ("contraction_ms", C.c_double), ("contraction_launches", C.c_int64)]


MAX_DLAS = 4


class ModelAbsorbers(C.Structure):
    _fields_ = [("counts", i32p), ("z_dlas", dp), ("log_nhis", dp), ("nhis", dp)]


class ModelSpectra(C.Structure):
    _fields_ = [("memory", C.c_int32), ("cap_offsets", i64p), ("pixel_inds", i32p), ("absorption", dp),
                ("model_mean", dp), ("continuum_mean", dp), ("continuum_sd", dp), ("chi2", dp),
                ("log_likelihoods", dp), ("num_pixels", i32p), ("levels", i32p)]


MODEL_LEVEL_BEST = 0
MODEL_LEVEL_GIVEN = 1


class ModelLevels(C.Structure):
    _fields_ = [("level_mode", C.c_int32), ("levels", i32p), ("log_priors_dla", dp)]


class MultiDla(C.Structure):
    _fields_ = [("max_dlas", C.c_int32), ("min_z_separation", C.c_double), ("occam_log_penalty", C.c_double),
                ("resample_uniforms", dp), ("forced_base_inds", i32p)]


class ResultsMulti(C.Structure):
    _fields_ = [("memory", C.c_int32), ("log_likelihoods_no_dla", dp), ("log_likelihoods_dla", dp),
                ("sample_log_likelihoods_dla", dp), ("sample_ld", C.c_int64), ("base_sample_inds", i32p),
                ("min_z_dlas", dp), ("max_z_dlas", dp), ("num_pixels", i32p)]


class MultiStats(C.Structure):
    _fields_ = [("level_ms", C.c_double * MAX_DLAS), ("level_launches", C.c_int64 * MAX_DLAS),
                ("resample_ms", C.c_double), ("resample_launches", C.c_int64),
                ("multi_reduce_ms", C.c_double), ("multi_reduce_launches", C.c_int64)]


SUMMARY_PLANES = 5
SUMMARY_MAX_BINS = 1024


class SummarySpec(C.Structure):
    _fields_ = [("log_nhi_samples", dp), ("num_z_bins", C.c_int32), ("num_nhi_bins", C.c_int32),
                ("z_edges", dp), ("log_nhi_edges", dp)]


class Summaries(C.Structure):
    _fields_ = [("memory", C.c_int32), ("map_sample_inds", i32p), ("map_log_likelihoods", dp),
                ("map_z_dlas", dp), ("map_log_nhis", dp), ("bin_planes", dp)]


INTERVAL_MAX_LEVELS = 8
INTERVAL_MAX_SAMPLES = 1 << 20


class IntervalSpec(C.Structure):
    _fields_ = [("log_nhi_samples", dp), ("lr_delta", C.c_double), ("num_levels", C.c_int32),
                ("levels", C.c_double * INTERVAL_MAX_LEVELS)]


class Intervals(C.Structure):
    _fields_ = [("memory", C.c_int32), ("z_means", dp), ("z_sds", dp), ("log_nhi_means", dp), ("log_nhi_sds", dp),
                ("z_lr_ranges", dp), ("log_nhi_lr_ranges", dp), ("z_quantiles", dp), ("log_nhi_quantiles", dp),
                ("lr_counts", i32p)]


class Forest(C.Structure):
    _fields_ = [("num_forest_lines", C.c_int32), ("variance_series", C.c_int32), ("mean_flux", C.c_int32),
                ("mean_flux_tau_0", C.c_double), ("mean_flux_beta", C.c_double)]


class SubDla(C.Structure):
    _fields_ = [("nhi_samples", dp)]


class ResultsSub(C.Structure):
    _fields_ = [("memory", C.c_int32), ("log_likelihoods_lls", dp), ("sample_log_likelihoods_lls", dp),
                ("sample_ld", C.c_int64), ("log_nhi_samples", dp), ("map_sample_inds", i32p),
                ("map_log_likelihoods", dp), ("map_z_lls", dp), ("map_log_nhi_lls", dp)]


class ModelStats(C.Structure):
    _fields_ = [("forest_ms", C.c_double), ("sub_dla_ms", C.c_double), ("sub_dla_reduce_ms", C.c_double),
                ("forest_launches", C.c_int64), ("sub_dla_launches", C.c_int64),
                ("sub_dla_reduce_launches", C.c_int64)]


POPULATION_MAX_LARGE = 8
PMF_CHUNK = 512
PMF_MAX_TRIALS = 1 << 18


class PopulationSpec(C.Structure):
    _fields_ = [("log_nhi_samples", dp), ("num_z_bins", C.c_int32), ("num_nhi_bins", C.c_int32),
                ("z_edges", dp), ("log_nhi_edges", dp), ("p_thresh_sample", C.c_double), ("p_switch", C.c_double),
                ("p_thresh_spec", C.c_double), ("log_priors_no_dla", dp), ("log_priors_dla", dp),
                ("log_priors_lls", dp)]


class Population(C.Structure):
    _fields_ = [("memory", C.c_int32), ("poisson_plane", dp), ("large_inds", i32p), ("large_probs", dp),
                ("large_bins", i32p), ("p_dlas", dp)]


class LevelPopulation(C.Structure):
    _fields_ = [("memory", C.c_int32), ("level_posteriors", dp), ("bin_planes", dp), ("poisson_plane", dp),
                ("large_inds", i32p), ("large_probs", dp), ("large_bins", i32p)]


class SearchCuts(C.Structure):
    _fields_ = [("proximity_zone", C.c_double), ("noise_thresh", C.c_double), ("omega_m", C.c_double),
                ("num_z_bins_summary", C.c_int32), ("z_edges_summary", dp), ("num_z_bins_population", C.c_int32),
                ("z_edges_population", dp)]


class SearchCutResults(C.Structure):
    _fields_ = [("memory", C.c_int32), ("z_uppers", dp), ("pixel_counts", i32p), ("bitmap_offsets", i64p),
                ("bitmap_words", u32p), ("path_summary", dp), ("path_population", dp)]


class SampleCuts(C.Structure):
    _fields_ = [("z_uppers", dp), ("pixel_counts", i32p), ("bitmap_offsets", i64p), ("bitmap_words", u32p)]


class BootstrapSpec(C.Structure):
    _fields_ = [("seed", C.c_uint64 * 2), ("num_replicas", C.c_int64), ("first_replica", C.c_int64),
                ("num_strata", C.c_int32), ("stratum_offsets", i64p), ("members", i32p)]


def bootstrap_tiling() -> dict:
    """The compile-time shape of the bootstrap sums kernel (gpdla_bootstrap_tiling): replicas and columns per
    block tile, spectra per K stage, spectra per split-K slice, most replicas per device chunk."""
    v = [C.c_int32() for _ in range(5)]
    check(load().gpdla_bootstrap_tiling(*[C.byref(x) for x in v]))
    return dict(zip(("tile_m", "tile_n", "stage_k", "k_slice", "max_chunk"), (x.value for x in v)))


class DlaPrior(C.Structure):
    _fields_ = [("alpha", C.c_double), ("uniform_min", C.c_double), ("uniform_max", C.c_double),
                ("fit_min", C.c_double), ("fit_max", C.c_double), ("fit_upper", C.c_double)]


class PreloadParams(C.Structure):
    _fields_ = [("normalization_min_lambda", C.c_double), ("normalization_max_lambda", C.c_double),
                ("min_lambda", C.c_double), ("max_lambda", C.c_double),
                ("loading_min_lambda", C.c_double), ("loading_max_lambda", C.c_double),
                ("min_num_pixels", C.c_int32), ("brightsky_bit", C.c_int32)]


# every symbol include/gpdla.h declares, with its ctypes signature
SIGNATURES = {
    "gpdla_engine_create": (C.c_int, [C.c_int32, C.POINTER(Model), C.POINTER(Samples), C.POINTER(Params), C.POINTER(C.c_void_p)]),
    "gpdla_engine_process": (C.c_int, [C.c_void_p, C.POINTER(Spectra), C.POINTER(Results)]),
    "gpdla_engine_synchronize": (C.c_int, [C.c_void_p]),
    "gpdla_engine_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gpdla_engine_set_panel_streams": (C.c_int, [C.c_void_p, C.c_int32]),
    "gpdla_engine_use_null_stream": (C.c_int, [C.c_void_p]),
    "gpdla_engine_get_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "gpdla_engine_get_stats_n": (C.c_int, [C.c_void_p, C.POINTER(Stats), C.c_int64]),
    "gpdla_engine_reset_stats": (C.c_int, [C.c_void_p]),
    "gpdla_engine_destroy": (None, [C.c_void_p]),
    "gpdla_engine_process_multi": (C.c_int, [C.c_void_p, C.POINTER(Spectra), C.POINTER(MultiDla),
                                             C.POINTER(ResultsMulti)]),
    "gpdla_engine_get_multi_stats": (C.c_int, [C.c_void_p, C.POINTER(MultiStats)]),
    "gpdla_engine_process_summaries": (C.c_int, [C.c_void_p, C.POINTER(Spectra), C.POINTER(MultiDla),
                                                 C.POINTER(ResultsMulti), C.POINTER(SummarySpec),
                                                 C.POINTER(Summaries)]),
    "gpdla_engine_get_summary_stats": (C.c_int, [C.c_void_p, dp, i64p]),
    "gpdla_posterior_summary_f64": (C.c_int, [C.c_int32, dp, C.c_int64, C.c_int64, C.c_int64, dp, dp, dp, dp, dp, i32p,
                                              C.c_int32, C.POINTER(SummarySpec), i32p, dp, dp, dp, dp]),
    "gpdla_engine_process_intervals": (C.c_int, [C.c_void_p, C.POINTER(Spectra), C.POINTER(MultiDla),
                                                 C.POINTER(ResultsMulti), C.POINTER(SummarySpec),
                                                 C.POINTER(Summaries), C.POINTER(IntervalSpec), C.POINTER(Intervals)]),
    "gpdla_engine_get_interval_stats": (C.c_int, [C.c_void_p, dp, i64p]),
    "gpdla_posterior_intervals_f64": (C.c_int, [C.c_int32, dp, C.c_int64, C.c_int64, C.c_int64, dp, dp, dp, dp, i32p,
                                                C.c_int32, C.POINTER(IntervalSpec), C.POINTER(Intervals)]),
    "gpdla_engine_set_forest": (C.c_int, [C.c_void_p, C.POINTER(Forest)]),
    "gpdla_engine_set_forest_scoped": (C.c_int, [C.c_void_p, C.POINTER(Forest), C.c_int32]),
    "gpdla_forest_f64": (C.c_int, [C.c_int32, dp, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_int32, dp]),
    "gpdla_engine_process_models": (C.c_int, [C.c_void_p, C.POINTER(Spectra), C.POINTER(MultiDla), C.POINTER(SubDla),
                                              C.POINTER(ResultsMulti), C.POINTER(ResultsSub), C.POINTER(SummarySpec),
                                              C.POINTER(Summaries)]),
    "gpdla_engine_get_model_stats": (C.c_int, [C.c_void_p, C.POINTER(ModelStats)]),
    "gpdla_engine_process_population": (C.c_int, [C.c_void_p, C.POINTER(Spectra), C.POINTER(MultiDla), C.POINTER(SubDla),
                                                  C.POINTER(ResultsMulti), C.POINTER(ResultsSub), C.POINTER(SummarySpec),
                                                  C.POINTER(Summaries), C.POINTER(PopulationSpec), C.POINTER(Population)]),
    "gpdla_engine_get_population_stats": (C.c_int, [C.c_void_p, dp, i64p]),
    "gpdla_engine_process_levels": (C.c_int, [C.c_void_p, C.POINTER(Spectra), C.POINTER(MultiDla), C.POINTER(SubDla),
                                              C.POINTER(ResultsMulti), C.POINTER(ResultsSub), C.POINTER(SummarySpec),
                                              C.POINTER(Summaries), C.POINTER(PopulationSpec), C.POINTER(Population),
                                              C.POINTER(LevelPopulation)]),
    "gpdla_engine_get_level_population_stats": (C.c_int, [C.c_void_p, dp, i64p]),
    "gpdla_level_planes_f64": (C.c_int, [C.c_int32, dp, C.c_int64, C.c_int64, C.c_int64, dp, dp, dp, dp, dp, i32p,
                                         C.c_int32, C.POINTER(SummarySpec), dp]),
    "gpdla_population_split_levels_f64": (C.c_int, [C.c_int32, dp, C.c_int64, C.c_int64, C.c_int64, dp, dp, dp, dp, i32p,
                                                    C.c_int32, dp, C.POINTER(PopulationSpec), dp, i32p, dp, i32p]),
    "gpdla_population_split_f64": (C.c_int, [C.c_int32, dp, C.c_int64, C.c_int64, C.c_int64, dp, dp, dp, dp, dp,
                                             C.POINTER(PopulationSpec), dp, i32p, dp, i32p]),
    "gpdla_poisson_binomial_pmf_f64": (C.c_int, [C.c_int32, dp, i64p, C.c_int64, dp]),
    "gpdla_bootstrap_tiling": (C.c_int, [i32p, i32p, i32p, i32p, i32p]),
    "gpdla_bootstrap_counts_i32": (C.c_int, [C.c_int32, C.c_int64, C.POINTER(BootstrapSpec), i32p]),
    "gpdla_bootstrap_rows_f64": (C.c_int, [C.c_int32, dp, C.c_int32, dp, dp, u8p, C.c_int64, C.c_int32, C.c_int32,
                                           C.c_double, dp, C.c_int64]),
    "gpdla_bootstrap_sums_f64": (C.c_int, [C.c_int32, i32p, dp, C.c_int64, C.c_int64, C.c_int64, dp]),
    "gpdla_bootstrap_f64": (C.c_int, [C.c_int32, dp, C.c_int64, C.c_int64, C.POINTER(BootstrapSpec), dp]),
    "gpdla_spectrum_snrs_f32": (C.c_int, [C.c_int32, C.c_int64, i64p, fp, fp, fp, dp, dp, fp]),
    "gpdla_spectrum_snrs_f64": (C.c_int, [C.c_int32, C.c_int64, i64p, dp, dp, dp, dp, dp, dp]),
    "gpdla_search_cuts_f64": (C.c_int, [C.c_int32, C.c_int64, i64p, dp, dp, dp, dp, C.POINTER(SearchCuts),
                                        C.POINTER(SearchCutResults)]),
    "gpdla_engine_process_cuts": (C.c_int, [C.c_void_p, C.POINTER(Spectra), C.POINTER(MultiDla), C.POINTER(SubDla),
                                            C.POINTER(ResultsMulti), C.POINTER(ResultsSub), C.POINTER(SummarySpec),
                                            C.POINTER(Summaries), C.POINTER(PopulationSpec), C.POINTER(Population),
                                            C.POINTER(LevelPopulation), C.POINTER(SearchCuts),
                                            C.POINTER(SearchCutResults)]),
    "gpdla_engine_get_cut_stats": (C.c_int, [C.c_void_p, dp, i64p]),
    "gpdla_level_planes_cut_f64": (C.c_int, [C.c_int32, dp, C.c_int64, C.c_int64, C.c_int64, dp, dp, dp, dp, dp, i32p,
                                             C.c_int32, C.POINTER(SummarySpec), C.POINTER(SampleCuts), dp]),
    "gpdla_population_split_levels_cut_f64": (C.c_int, [C.c_int32, dp, C.c_int64, C.c_int64, C.c_int64, dp, dp, dp, dp,
                                                        i32p, C.c_int32, dp, C.POINTER(PopulationSpec),
                                                        C.POINTER(SampleCuts), dp, i32p, dp, i32p]),
    "gpdla_engine_model_spectra": (C.c_int, [C.c_void_p, C.POINTER(Spectra), C.POINTER(ModelAbsorbers),
                                             C.POINTER(ModelSpectra)]),
    "gpdla_engine_process_spectra_models": (C.c_int, [C.c_void_p, C.POINTER(Spectra), C.POINTER(MultiDla),
                                                      C.POINTER(ResultsMulti), C.POINTER(SummarySpec),
                                                      C.POINTER(Summaries), C.POINTER(IntervalSpec),
                                                      C.POINTER(Intervals), C.POINTER(ModelLevels),
                                                      C.POINTER(ModelSpectra)]),
    "gpdla_engine_get_model_spectra_stats": (C.c_int, [C.c_void_p, dp, i64p]),
    "gpdla_count_mixture_f64": (C.c_int, [C.c_int32, dp, i32p, i64p, i64p, C.c_int64, C.c_int64, dp, C.c_int32, i32p, i32p,
                                          dp, dp]),
    "gpdla_count_mixture_tiling": (C.c_int, [i32p, i32p, i32p]),
    "gpdla_resample_f64":(C.c_int, [C.c_int32, dp, C.c_int64, C.c_int64, C.c_int64, dp, i32p]),
    "gpdla_voigt_f64": (C.c_int, [dp, C.c_int64, C.c_double, C.c_double, C.c_int32, dp]),
    "gpdla_voigt_batch_f64": (C.c_int, [dp, C.c_int64, dp, dp, C.c_int64, C.c_int32, dp]),
    "gpdla_log_mvnpdf_low_rank_f64": (C.c_int, [dp, dp, dp, dp, C.c_int64, C.c_int32, dp]),
    "gpdla_objective_create": (C.c_int, [C.c_int32, C.c_int64, C.c_int64, C.c_int32, dp, dp, dp, C.c_int32,
                                         C.POINTER(C.c_void_p)]),
    "gpdla_objective_eval": (C.c_int, [C.c_void_p, dp, dp, dp]),
    "gpdla_objective_destroy": (None, [C.c_void_p]),
    "gpdla_spectrum_loss_f64": (C.c_int, [dp, dp, dp, dp, dp, C.c_int64, C.c_int32, C.c_double, C.c_double,
                                          C.c_double, dp, dp, dp, dp, dp, dp]),
    "gpdla_objective_set_forest": (C.c_int, [C.c_void_p, dp, C.c_int32, C.c_int32]),
    "gpdla_spectrum_loss_forest_f64": (C.c_int, [dp, dp, dp, dp, dp, C.c_int64, C.c_int32, C.c_double, C.c_double,
                                                 C.c_double, C.c_double, C.c_int32, dp, dp, dp, dp, dp, dp]),
    "gpdla_forest_rows_f64": (C.c_int, [C.c_int32, dp, dp, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_int32,
                                        dp]),
    "gpdla_halton_rr2_f64": (C.c_int, [C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.c_int32, dp]),
    "gpdla_generate_dla_samples_f64": (C.c_int, [C.c_int32, dp, C.c_int64, C.c_int64, C.POINTER(DlaPrior), dp, dp, dp,
                                                 dp]),
    "gpdla_read_spec_f32": (C.c_int, [C.c_int32, C.c_int64, fp, fp, i32p, fp, fp, u8p]),
    "gpdla_preload_qsos_f32": (C.c_int, [C.c_int32, C.c_int64, i64p, fp, fp, fp, i32p, dp, C.POINTER(PreloadParams),
                                         u8p, i64p, fp, fp, fp, u8p, dp, fp]),
    "gpdla_diag_faddeeva_w": (C.c_int, [C.c_double, C.c_double, dp, dp]),
    "gpdla_diag_line_table_error": (C.c_int, [C.c_int32, dp]),
    "gpdla_diag_raw_profile3": (C.c_int, [dp, C.c_int64, C.c_double, C.c_double, C.c_int32, dp]),
    "gpdla_device_malloc": (C.c_int, [C.c_int32, C.c_int64, C.POINTER(C.c_void_p)]),
    "gpdla_device_free": (C.c_int, [C.c_int32, C.c_void_p]),
    "gpdla_memcpy_htod": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64]),
    "gpdla_memcpy_dtoh": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64]),
    "gpdla_last_error": (C.c_char_p, []),
    "gpdla_version": (C.c_int32, []),
    "gpdla_last_call_kernel_ms": (C.c_int, [C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_int32)]),
    "gpdla_device_count": (C.c_int32, []),
    "gpdla_device_pci_bus_id": (C.c_int, [C.c_int32, C.c_char_p, C.c_int32]),
}

# GPDLA_ABI_VERSION of include/gpdla.h this binding is written against
ABI_VERSION = 5

_lib = None


class GpdlaError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"gpdla error {code}: {msg}")
        self.code = code


class GpdlaNumericError(GpdlaError):
    pass


def load() -> C.CDLL:
    """Load libgpdla.so (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise ImportError(f"{LIB_PATH} not built; run __graft_entry__.build() "
                              "(there is no CPU fallback for the GP-DLA hot path)")
        lib = C.CDLL(str(LIB_PATH))
        missing = [name for name in SIGNATURES if getattr(lib, name, None) is None]
        if missing:
            raise ImportError(f"{LIB_PATH} lacks {', '.join(missing)}: a stale or foreign build "
                              "(rebuild with __graft_entry__.build())")
        lib.gpdla_version.restype = C.c_int32
        if lib.gpdla_version() != ABI_VERSION:
            raise ImportError(f"{LIB_PATH} has ABI version {lib.gpdla_version()}, this binding needs "
                              f"{ABI_VERSION} (rebuild with __graft_entry__.build())")
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def pci_bus_id(device: int) -> str:
    """PCI bus id of a HIP device (which physical GPU a rank drives)."""
    buf = C.create_string_buffer(64)
    check(load().gpdla_device_pci_bus_id(device, buf, len(buf)))
    return buf.value.decode()


def last_call_kernel_ms() -> list[float]:
    """Per-launch kernel times (ms) of this thread's last ingest / sampler call (gpdla_last_call_kernel_ms)."""
    buf = (C.c_double * 8)()
    n = C.c_int32(0)
    check(load().gpdla_last_call_kernel_ms(buf, 8, C.byref(n)))
    return [buf[i] for i in range(min(n.value, 8))]


def check(rc: int) -> int:
    if rc == GPDLA_OK:
        return rc
    msg = load().gpdla_last_error().decode(errors="replace")
    if rc == GPDLA_ENUMERIC:
        raise GpdlaNumericError(rc, msg)
    raise GpdlaError(rc, msg)


def ptr(arr, ctype=C.c_double):
    """ctypes pointer to a numpy array's data (None -> NULL)."""
    if arr is None:
        return None
    return arr.ctypes.data_as(C.POINTER(ctype))


def dev_ptr(addr: int, ctype=C.c_double):
    """ctypes pointer from a raw device address (e.g. torch ``tensor.data_ptr()``)."""
    if addr is None:
        return None
    return C.cast(C.c_void_p(addr), C.POINTER(ctype))


class DeviceArray:
    """A device buffer owned by libgpdla (hipMalloc on the library's HIP runtime)."""

    def __init__(self, device: int, shape, dtype):
        import numpy as np
        self.device, self.shape, self.dtype = device, tuple(np.atleast_1d(shape)), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p()
        check(load().gpdla_device_malloc(device, self.nbytes, C.byref(p)))
        self.ptr = p.value

    @classmethod
    def from_numpy(cls, arr, device: int = 0):
        import numpy as np
        arr = np.ascontiguousarray(arr)
        out = cls(device, arr.shape, arr.dtype)
        check(load().gpdla_memcpy_htod(device, C.c_void_p(out.ptr), arr.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def numpy(self, rows: int | None = None, start: int = 0):
        """Copy to host; ``rows`` limits the copy to that many rows from row ``start`` (C order)."""
        import numpy as np
        nrow = self.shape[0] - start if rows is None else min(rows, self.shape[0] - start)
        shape = (max(nrow, 0),) + self.shape[1:]
        out = np.empty(shape, dtype=self.dtype)
        row_bytes = int(self.nbytes // self.shape[0]) if self.shape[0] else 0
        src = C.c_void_p(int(self.ptr) + int(start) * row_bytes)
        check(load().gpdla_memcpy_dtoh(self.device, out.ctypes.data_as(C.c_void_p), src, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            load().gpdla_device_free(self.device, C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
