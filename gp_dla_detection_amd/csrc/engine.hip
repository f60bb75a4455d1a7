// C-ABI of libgpdla.so (include/gpdla.h): engine lifecycle, device workspaces, batching,
// kernel-time accounting and the standalone voigt / log_mvnpdf_low_rank entry points.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/gpdla.h"
#include "internal.h"

using namespace gpdla;

namespace {
thread_local std::string g_last_error;
thread_local LaunchTimes g_launch_times;
}  // namespace

namespace gpdla {

int set_error(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

LaunchTimes& launch_times() { return g_launch_times; }

int check_device(int32_t device) {
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count == 0)
    return set_error(GPDLA_EDEVICE, "no HIP device available (%s): libgpdla has no CPU fallback",
                     hipGetErrorString(e));
  if (device < 0 || device >= count)
    return set_error(GPDLA_EINVAL, "device %d out of range (%d devices)", device, count);
  return GPDLA_OK;
}

}  // namespace gpdla

namespace {

// ---- line-profile data (fitted once per process on the host; layout in internal.h)
struct HostLineData {
  std::vector<double> buf;
};

const HostLineData& host_line_data() {
  static HostLineData d;
  static std::once_flag once;
  std::call_once(once, [] {
    d.buf.assign(kLineBufDoubles, 0.0);
    for (int j = 0; j < kMaxLines; ++j) {
      fit_core_table(j, d.buf.data() + (size_t)j * kCoreTable);
      fit_wing_line(j, d.buf.data() + kLineBufWing + (size_t)j * kWingStride);
    }
    for (int j = 0; j < kMaxLines; ++j) {
      // fac_j = c / (lambda_j 1e8) / (sigma sqrt 2): x_j = lambda fac_j / (1+z) - c / (sigma sqrt 2)
      const long double f = (long double)kCcgs / ((long double)kTransitionWavelengths[j] * 1e8L) /
                            ((long double)kSigma * std::sqrt(2.0L));
      d.buf[kLineBufFac + j] = (double)f;
    }
    for (int j = 0; j < 64; ++j) d.buf[kLineBufExp2 + j] = (double)std::exp2((long double)j / 64.0L);
    for (int j = 0; j < 128; ++j) d.buf[kLineBufExp128 + j] = (double)std::exp2((long double)j / 128.0L);
  });
  return d;
}

LineArgs make_line_args(const double* d_buf) {
  LineArgs l{};
  l.buf = d_buf;
  return l;
}

template <class T>
int grow(T** p, size_t* cap, size_t count) {
  if (count <= *cap && *p) return GPDLA_OK;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  size_t want = std::max<size_t>(count, 1);
  HIP_TRY(hipMalloc((void**)p, want * sizeof(T)));
  *cap = want;
  return GPDLA_OK;
}

struct TimedLaunch {
  hipEvent_t start, stop;
  int kind;  // 0 prep, 1 likelihood, 2 reduce, 3 contraction (panel-GEMM paths, inside 1);
             // gpdla_engine_process_multi only: 4 resample, 5 level >= 2 sweep, 6 its log-mean-exp;
             // 7 posterior summaries (gpdla_engine_process_summaries); 8 forest kernels; gpdla_engine_process_models
             // only: 9 sub-DLA sweep, 10 its log-mean-exp and MAP launches; 11 population launches
             // (gpdla_engine_process_population); 12 level-population launches (gpdla_engine_process_levels);
             // 13 posterior intervals (gpdla_engine_process_intervals); 14 search cuts (gpdla_engine_process_cuts);
             // 15 model spectra (gpdla_engine_model_spectra)
  int level; // multi-DLA level the span also counts for in gpdla_multi_stats (0: none)
};

// One of the two staging sets of the host-buffer pipeline (gpdla_engine_process with host inputs
// and host results): the batch's inputs and results on the device, and the events that order the
// copy stream against the compute stream.
struct HostStage {
  double *wl = nullptr, *flux = nullptr, *noise = nullptr, *z = nullptr;
  uint8_t* mask = nullptr;
  double *sll = nullptr, *llnull = nullptr, *lldla = nullptr, *zmin = nullptr, *zmax = nullptr;
  int32_t* npix = nullptr;
  size_t cap_wl = 0, cap_flux = 0, cap_noise = 0, cap_mask = 0, cap_z = 0, cap_sll = 0;
  size_t cap_o[5] = {0, 0, 0, 0, 0};
  hipEvent_t in_ready = nullptr;   // copy stream: this batch's inputs are on the device
  hipEvent_t in_free = nullptr;    // compute stream: prep_kernel has read them
  hipEvent_t out_ready = nullptr;  // compute stream: the batch's results are written
  hipEvent_t out_free = nullptr;   // copy stream: they are back on the host
};

}  // namespace

struct gpdla_engine {
  int device = 0;
  int K = 0;
  int64_t S = 0;
  bool gemm = false;                 // panel-GEMM path (gemm_path.hip + gemm_f64 / gemm_i8) instead of fused
  bool i8 = false;                   // fused path with the int8 Ozaki contraction (kernels_i8.hip)
  int i8_nd = 4;                     // int8 panel-GEMM digit planes: 4 (levels <= 3) or 3 (_I8_24)
  gpdla_params params{};
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;

  // resident model / samples / line data
  double *d_rest = nullptr, *d_mu = nullptr, *d_M = nullptr, *d_logom = nullptr;
  int32_t num_rest = 0;
  double c0 = 0, tau0 = 0, beta = 0;
  int32_t om2_hi_e = 0;  // binary exponent of max omega^2 (1 + c_0)^2 over the rest grid (prep units)
  double *d_off = nullptr, *d_nhi = nullptr;  // samples in ascending-offset (z_DLA) order
  int32_t* d_perm = nullptr;                   // sorted sample index -> caller's sample index
  double* d_lines = nullptr;
  int32_t* d_status = nullptr;

  // batch workspaces
  size_t cap_meta = 0, cap_q = 0, cap_slots = 0, cap_lam = 0, cap_sll = 0, cap_scr = 0;
  size_t cap_smap = 0, cap_wl = 0, cap_flux = 0, cap_noise = 0, cap_mask = 0, cap_z = 0;
  int64_t* d_meta = nullptr;  // [offsets(Q+1) | slot_base | lam_base | slot_cap]
  double *d_wl = nullptr, *d_flux = nullptr, *d_noise = nullptr;
  uint8_t* d_mask = nullptr;
  double* d_z = nullptr;
  SpecInfo* d_info = nullptr;
  double *d_panel = nullptr, *d_lam = nullptr;
  int32_t* d_smap = nullptr;
  double* d_scratch = nullptr;
  double *d_sll = nullptr, *d_llnull = nullptr, *d_lldla = nullptr, *d_zmin = nullptr,
         *d_zmax = nullptr;
  int32_t* d_npix = nullptr;
  size_t cap_qout = 0;
  // panel-GEMM path workspaces
  double *d_pm = nullptr, *d_srow = nullptr, *d_wg = nullptr, *d_wu = nullptr, *d_G = nullptr,
         *d_U = nullptr, *d_q1p = nullptr, *d_ldp = nullptr;
  size_t cap_pm = 0, cap_srow = 0, cap_wg = 0, cap_wu = 0, cap_G = 0, cap_U = 0, cap_q1p = 0,
         cap_ldp = 0;
  // int8 fused path workspaces
  uint8_t* d_pi8 = nullptr;          // fused: digit chunks; panel-GEMM: B digit planes per spectrum
  uint8_t* d_ai8 = nullptr;          // panel-GEMM int8: A digit planes of a sample chunk
  size_t cap_ai8 = 0;
  double *d_psc = nullptr, *d_pent = nullptr;
  size_t cap_pi8 = 0, cap_psc = 0, cap_pent = 0;

  // host-buffer pipeline: batch b's results are copied back, and batch b + 1's inputs copied in, on
  // copy_stream while batch b + 1 (resp. b) computes; the two stages alternate
  HostStage hs[2];
  hipStream_t copy_stream = nullptr;
  // the panel-GEMM paths' extra compute streams (panel_streams > 1): spectrum q of a batch runs on
  // stream q % panel_streams (0 = the engine's stream) with its own workspace set, so one spectrum's
  // kernels fill the last-round tails of the others'
  static constexpr int kMaxPanelStreams = 4;
  int panel_streams = 2;
  hipStream_t panel_stream[kMaxPanelStreams] = {};
  hipEvent_t panel_fork = nullptr, panel_join[kMaxPanelStreams] = {};
  int64_t ws_ai8 = 0, ws_G = 0, ws_U = 0, ws_wp = 0, ws_w = 0;  // per-set workspace sizes (bytes / doubles)

  // pinned host metadata (reused after meta_ready completes)
  int64_t* h_meta = nullptr;
  size_t cap_hmeta = 0;
  hipEvent_t meta_done = nullptr;


  // multi-DLA (gpdla_engine_process_multi): the samples in the caller's order, per-batch level
  // workspaces ([D][nq][S] sample rows, [D][nq] evidences, [D-1][nq][S] base indices, two chain tables
  // [nq][S][kMaxChain]), the uniforms and forced indices of a call, the resampler's global prefix sums
  double *d_off_c = nullptr, *d_nhi_c = nullptr;
  double *d_m_sll = nullptr, *d_m_lldla = nullptr, *d_m_null = nullptr, *d_m_zmin = nullptr, *d_m_zmax = nullptr;
  double *d_m_u = nullptr, *d_m_cws = nullptr;
  int32_t *d_m_npix = nullptr, *d_m_base = nullptr, *d_m_chain[2] = {nullptr, nullptr}, *d_m_forced = nullptr;
  size_t cap_m_sll = 0, cap_m_lldla = 0, cap_m_q[4] = {0, 0, 0, 0}, cap_m_u = 0, cap_m_cws = 0, cap_m_base = 0,
         cap_m_chain[2] = {0, 0}, cap_m_forced = 0;
  gpdla_multi_stats mstats{};

  // posterior summaries (gpdla_engine_process_summaries): the samples' log10 N_HI and the grid edges of
  // a call, and a batch's outputs ([D][nq] MAP index / value, [D][nq][kMaxDlas] pairs, [nq][5][bins])
  double *d_s_lognhi = nullptr, *d_s_edges = nullptr, *d_s_ll = nullptr, *d_s_z = nullptr, *d_s_n = nullptr,
         *d_s_planes = nullptr;
  int32_t* d_s_ind = nullptr;
  size_t cap_s_lognhi = 0, cap_s_edges = 0, cap_s_ll = 0, cap_s_z = 0, cap_s_n = 0, cap_s_planes = 0, cap_s_ind = 0;
  double summary_ms = 0.0;
  int64_t summary_launches = 0;

  // Lyman-series forest (gpdla_engine_set_forest): applied by every process* call while set
  bool forest_on = false;
  gpdla_forest forest{};
  int32_t forest_scope = 0;          // gpdla_engine_set_forest_scoped: 0 mu, 1 mu and M, 2 mu, M and omega^2
  // sub-DLA model (gpdla_engine_process_models): the call's column densities in sweep and in caller
  // order and their log10, a batch's [nq][S] sample rows, [nq] evidences, the sweep's discarded null
  // lane and the MAP outputs ([nq] index / value, [nq][kMaxDlas] pairs)
  std::vector<int32_t> h_perm;       // sorted sample index -> caller's sample index (d_perm)
  double *d_sub_nhi = nullptr, *d_sub_nhi_c = nullptr, *d_sub_lognhi = nullptr, *d_sub_sll = nullptr,
         *d_sub_ev = nullptr, *d_sub_null = nullptr, *d_sub_mll = nullptr, *d_sub_mz = nullptr, *d_sub_mn = nullptr;
  int32_t* d_sub_mind = nullptr;
  size_t cap_sub_nhi = 0, cap_sub_nhi_c = 0, cap_sub_lognhi = 0, cap_sub_sll = 0, cap_sub_ev = 0, cap_sub_null = 0,
         cap_sub_mll = 0, cap_sub_mz = 0, cap_sub_mn = 0, cap_sub_mind = 0;
  gpdla_model_stats model_stats{};

  // population statistics (gpdla_engine_process_population): the call's log priors ([Q], [D][Q], [Q]),
  // its samples' log10 N_HI and grid edges, and a batch's outputs ([nq] p_dla, [nq][bins] Poisson plane,
  // [nq][8] large samples)
  double *d_p_lpno = nullptr, *d_p_lpdla = nullptr, *d_p_lplls = nullptr, *d_p_lognhi = nullptr, *d_p_edges = nullptr,
         *d_p_pdla = nullptr, *d_p_plane = nullptr, *d_p_lprob = nullptr;
  int32_t *d_p_lind = nullptr, *d_p_lbin = nullptr;
  size_t cap_p_lpno = 0, cap_p_lpdla = 0, cap_p_lplls = 0, cap_p_lognhi = 0, cap_p_edges = 0, cap_p_pdla = 0,
         cap_p_plane = 0, cap_p_lprob = 0, cap_p_lind = 0, cap_p_lbin = 0;
  double population_ms = 0.0;
  int64_t population_launches = 0;

  // population statistics over every level (gpdla_engine_process_levels): a batch's outputs ([D][nq] level
  // posteriors, [nq][D][5][bins] planes, [nq][D][bins] Poisson planes, [nq][D][8] large samples with
  // [kMaxDlas] bins each)
  double *d_lv_post = nullptr, *d_lv_planes = nullptr, *d_lv_plane = nullptr, *d_lv_lprob = nullptr;
  int32_t *d_lv_lind = nullptr, *d_lv_lbin = nullptr;
  size_t cap_lv_post = 0, cap_lv_planes = 0, cap_lv_plane = 0, cap_lv_lprob = 0, cap_lv_lind = 0, cap_lv_lbin = 0;
  double level_population_ms = 0.0;
  int64_t level_population_launches = 0;

  // posterior intervals (gpdla_engine_process_intervals): the offsets in the caller's order, the call's log10
  // N_HI, the rank tables of both ([S] ranks, [S] values by rank), and a batch's outputs (one block:
  // [4][D][nq][kMaxDlas] moments, [2][D][nq][kMaxDlas][2] ranges, [2][D][nq][kMaxDlas][levels] quantiles; [D][nq] counts)
  std::vector<double> h_off_c;
  double *d_i_lognhi = nullptr, *d_i_uniq = nullptr, *d_i_out = nullptr;
  int32_t *d_i_rank = nullptr, *d_i_count = nullptr;
  size_t cap_i_lognhi = 0, cap_i_uniq = 0, cap_i_out = 0, cap_i_rank = 0, cap_i_count = 0;
  double interval_ms = 0.0;
  int64_t interval_launches = 0;
  // search cuts (gpdla_engine_process_cuts): a batch's upper ends, pixel counts, bitmap (the word offsets are those
  // of the whole call) and path columns, and the call's z edges [summary | population]
  double *d_c_zu = nullptr, *d_c_path[2] = {nullptr, nullptr}, *d_c_edges = nullptr;
  int32_t* d_c_np = nullptr;
  int64_t* d_c_wo = nullptr;
  uint32_t* d_c_words = nullptr;
  size_t cap_c_zu = 0, cap_c_path[2] = {0, 0}, cap_c_edges = 0, cap_c_np = 0, cap_c_wo = 0, cap_c_words = 0;
  double cut_ms = 0.0;
  int64_t cut_launches = 0;
  // model spectra (gpdla_engine_model_spectra): a batch's absorbers, capacity offsets and outputs in one block
  // carved in 256-byte steps, the kernel's per-pixel workspace ([3][slots]) and its status word
  char* d_ms = nullptr;
  double* d_ms_scratch = nullptr;
  int32_t* d_ms_status = nullptr;
  size_t cap_ms = 0, cap_ms_scratch = 0, cap_ms_status = 0;
  double model_spectra_ms = 0.0;
  int64_t model_spectra_launches = 0;

  std::vector<TimedLaunch> pending;
  gpdla_stats stats{};
};

namespace {

int record_start(gpdla_engine* e, TimedLaunch* t, int kind, hipStream_t s = nullptr) {
  HIP_TRY(hipEventCreate(&t->start));
  HIP_TRY(hipEventCreate(&t->stop));
  t->kind = kind;
  HIP_TRY(hipEventRecord(t->start, s ? s : e->stream));
  return GPDLA_OK;
}

int resolve_events(gpdla_engine* e) {
  for (auto& t : e->pending) {
    HIP_TRY(hipEventSynchronize(t.stop));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, t.start, t.stop));
    if (t.kind == 0) { e->stats.prep_ms += ms; e->stats.prep_launches++; }
    if (t.kind == 1) { e->stats.likelihood_ms += ms; e->stats.likelihood_launches++; }
    if (t.kind == 2) { e->stats.reduce_ms += ms; e->stats.reduce_launches++; }
    if (t.kind == 3) { e->stats.contraction_ms += ms; e->stats.contraction_launches++; }
    if (t.kind == 4) { e->mstats.resample_ms += ms; e->mstats.resample_launches++; }
    if (t.kind == 6) { e->mstats.multi_reduce_ms += ms; e->mstats.multi_reduce_launches++; }
    if (t.kind == 7) { e->summary_ms += ms; e->summary_launches++; }
    if (t.kind == 8) { e->model_stats.forest_ms += ms; e->model_stats.forest_launches++; }
    if (t.kind == 9) { e->model_stats.sub_dla_ms += ms; e->model_stats.sub_dla_launches++; }
    if (t.kind == 10) { e->model_stats.sub_dla_reduce_ms += ms; e->model_stats.sub_dla_reduce_launches++; }
    if (t.kind == 11) { e->population_ms += ms; e->population_launches++; }
    if (t.kind == 12) { e->level_population_ms += ms; e->level_population_launches++; }
    if (t.kind == 13) { e->interval_ms += ms; e->interval_launches++; }
    if (t.kind == 14) { e->cut_ms += ms; e->cut_launches++; }
    if (t.kind == 15) { e->model_spectra_ms += ms; e->model_spectra_launches++; }
    if (t.level >= 1 && t.level <= GPDLA_MAX_DLAS) {
      e->mstats.level_ms[t.level - 1] += ms;
      e->mstats.level_launches[t.level - 1]++;
    }
    (void)hipEventDestroy(t.start);
    (void)hipEventDestroy(t.stop);
  }
  e->pending.clear();
  return GPDLA_OK;
}

int validate_params(const gpdla_params* p) {
  if (p->num_lines < 1 || p->num_lines > kMaxLines)
    return set_error(GPDLA_EINVAL, "num_lines=%d outside [1, %d] (voigt.c:16)", p->num_lines, kMaxLines);
  if (p->width != kWidth)
    return set_error(GPDLA_EINVAL, "width=%d but the instrument profile is compiled for %d (voigt.c:229)",
                     p->width, kWidth);
  if (p->absorption_mode != GPDLA_ABSORPTION_REFERENCE && p->absorption_mode != GPDLA_ABSORPTION_UNMASKED)
    return set_error(GPDLA_EINVAL, "absorption_mode=%d", p->absorption_mode);
  if (!(p->max_lambda > p->min_lambda) || !(p->pixel_spacing > 0) || !(p->lya_wavelength > 0))
    return set_error(GPDLA_EINVAL, "invalid wavelength parameters");
  if (p->max_batch_spectra < 0) return set_error(GPDLA_EINVAL, "max_batch_spectra < 0");
  if (p->path != GPDLA_PATH_AUTO && p->path != GPDLA_PATH_FUSED && p->path != GPDLA_PATH_PANEL_GEMM &&
      p->path != GPDLA_PATH_FUSED_I8 && p->path != GPDLA_PATH_PANEL_GEMM_I8 && p->path != GPDLA_PATH_PANEL_GEMM_I8_24)
    return set_error(GPDLA_EINVAL, "path=%d", p->path);
  return GPDLA_OK;
}

int upload(void* dst, const void* src, size_t bytes, hipStream_t s) {
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
  return GPDLA_OK;
}

}  // namespace

extern "C" {

int32_t gpdla_version(void) { return GPDLA_ABI_VERSION; }

int gpdla_last_call_kernel_ms(double* ms, int32_t capacity, int32_t* count) {
  if (!count || capacity < 0 || (capacity > 0 && !ms))
    return set_error(GPDLA_EINVAL, "last_call_kernel_ms: null argument or negative capacity");
  const LaunchTimes& t = launch_times();
  *count = t.done;
  for (int i = 0; i < t.done && i < capacity; ++i) ms[i] = t.ms[i];
  return GPDLA_OK;
}

int32_t gpdla_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

int gpdla_device_pci_bus_id(int32_t device, char* buf, int32_t len) {
  if (!buf || len < 13) return set_error(GPDLA_EINVAL, "pci bus id buffer needs >= 13 bytes");
  int c = gpdla_device_count();
  if (c == 0) return set_error(GPDLA_EDEVICE, "no HIP device");
  if (device < 0 || device >= c) return set_error(GPDLA_EINVAL, "device %d outside [0, %d)", device, c);
  HIP_TRY(hipDeviceGetPCIBusId(buf, len, device));
  return GPDLA_OK;
}

const char* gpdla_last_error(void) { return g_last_error.c_str(); }

int gpdla_diag_faddeeva_w(double x, double y, double* re, double* im);  // faddeeva_host.cpp

int gpdla_diag_line_table_error(int32_t line, double* max_rel_err) {
  if (line < 0 || line >= kMaxLines || !max_rel_err) return set_error(GPDLA_EINVAL, "bad line");
  *max_rel_err = line_profile_error(line);  // core, wing and outer wing
  return GPDLA_OK;
}

void gpdla_engine_destroy(gpdla_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  (void)hipStreamSynchronize(e->stream);  // (the null stream too)
  if (e->copy_stream) (void)hipStreamSynchronize(e->copy_stream);
  for (auto& t : e->pending) { (void)hipEventDestroy(t.start); (void)hipEventDestroy(t.stop); }
  for (HostStage& h : e->hs) {
    void* hb[] = {h.wl, h.flux, h.noise, h.z, h.mask, h.sll, h.llnull, h.lldla, h.zmin, h.zmax, h.npix};
    for (void* b : hb)
      if (b) (void)hipFree(b);
    for (hipEvent_t ev : {h.in_ready, h.in_free, h.out_ready, h.out_free})
      if (ev) (void)hipEventDestroy(ev);
  }
  if (e->copy_stream) (void)hipStreamDestroy(e->copy_stream);
  for (int i = 1; i < gpdla_engine::kMaxPanelStreams; ++i) {
    if (e->panel_stream[i]) {
      (void)hipStreamSynchronize(e->panel_stream[i]);
      (void)hipStreamDestroy(e->panel_stream[i]);
    }
    if (e->panel_join[i]) (void)hipEventDestroy(e->panel_join[i]);
  }
  if (e->panel_fork) (void)hipEventDestroy(e->panel_fork);
  void* bufs[] = {e->d_rest, e->d_mu, e->d_M, e->d_logom, e->d_off, e->d_nhi, e->d_perm, e->d_lines,
                  e->d_status, e->d_meta, e->d_wl, e->d_flux, e->d_noise, e->d_mask, e->d_z,
                  e->d_info, e->d_panel, e->d_lam, e->d_smap, e->d_scratch, e->d_sll,
                  e->d_llnull, e->d_lldla, e->d_zmin, e->d_zmax, e->d_npix, e->d_pm, e->d_srow,
                  e->d_wg, e->d_wu, e->d_G, e->d_U, e->d_q1p, e->d_ldp, e->d_pi8, e->d_psc,
                  e->d_pent, e->d_ai8, e->d_off_c, e->d_nhi_c, e->d_m_sll, e->d_m_lldla, e->d_m_null,
                  e->d_m_zmin, e->d_m_zmax, e->d_m_u, e->d_m_cws, e->d_m_npix, e->d_m_base,
                  e->d_m_chain[0], e->d_m_chain[1], e->d_m_forced, e->d_s_lognhi, e->d_s_edges,
                  e->d_s_ll, e->d_s_z, e->d_s_n, e->d_s_planes, e->d_s_ind, e->d_sub_nhi, e->d_sub_nhi_c,
                  e->d_sub_lognhi, e->d_sub_sll, e->d_sub_ev, e->d_sub_null, e->d_sub_mll, e->d_sub_mz,
                  e->d_sub_mn, e->d_sub_mind, e->d_p_lpno, e->d_p_lpdla, e->d_p_lplls, e->d_p_lognhi, e->d_p_edges,
                  e->d_p_pdla, e->d_p_plane, e->d_p_lprob, e->d_p_lind, e->d_p_lbin,
                  e->d_lv_post, e->d_lv_planes, e->d_lv_plane, e->d_lv_lprob, e->d_lv_lind, e->d_lv_lbin,
                  e->d_i_lognhi, e->d_i_uniq, e->d_i_out, e->d_i_rank, e->d_i_count,
                  e->d_c_zu, e->d_c_path[0], e->d_c_path[1], e->d_c_edges, e->d_c_np, e->d_c_wo, e->d_c_words,
                  e->d_ms, e->d_ms_scratch, e->d_ms_status};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  if (e->h_meta) (void)hipHostFree(e->h_meta);
  if (e->meta_done) (void)hipEventDestroy(e->meta_done);

  if (e->own_stream) (void)hipStreamDestroy(e->own_stream);
  delete e;
}

int gpdla_engine_create(int32_t device, const gpdla_model* model, const gpdla_samples* samples,
                        const gpdla_params* params, gpdla_engine** out) {
  if (!model || !samples || !params || !out) return set_error(GPDLA_EINVAL, "null argument");
  *out = nullptr;
  int rc = check_device(device);
  if (rc) return rc;
  if ((rc = validate_params(params))) return rc;
  // fused paths: a rank between the compiled ones runs on the next compiled rank, M zero-padded
  // (fused_rank, kernels.hip: exact)
  const int k_fused = fused_rank(model->k), k_i8 = i8_fused_rank(model->k);
  const bool fused_ok = k_fused > 0;
  const bool gemm_i8 = params->path == GPDLA_PATH_PANEL_GEMM_I8 || params->path == GPDLA_PATH_PANEL_GEMM_I8_24;
  const bool use_gemm = params->path == GPDLA_PATH_PANEL_GEMM || gemm_i8 ||
                        (params->path == GPDLA_PATH_AUTO && !fused_ok);
  const bool use_i8 = params->path == GPDLA_PATH_FUSED_I8 || gemm_i8;
  if (gemm_i8 && params->num_lines != 3)
    return set_error(GPDLA_EUNSUPPORTED, "int8 panel-GEMM path needs num_lines=3 (num_lines=%d)", params->num_lines);
  if (params->path == GPDLA_PATH_FUSED_I8 && (k_i8 == 0 || params->num_lines != 3))
    return set_error(GPDLA_EUNSUPPORTED, "int8 fused path needs k<=20 and num_lines=3 (k=%d, num_lines=%d)",
                     model->k, params->num_lines);
  if (!use_gemm && !fused_ok)
    return set_error(GPDLA_EUNSUPPORTED, "rank k=%d above the fused path's compiled ranks (<= 24)", model->k);
  if (use_gemm && (model->k < 1 || model->k > kGemmMaxK))
    return set_error(GPDLA_EUNSUPPORTED, "rank k=%d outside the panel-GEMM path's 1..%d", model->k, kGemmMaxK);
  if (model->num_rest < 2 || !model->rest_wavelengths || !model->mu || !model->M || !model->log_omega)
    return set_error(GPDLA_EINVAL, "invalid model");
  for (int i = 1; i < model->num_rest; ++i)
    if (!(model->rest_wavelengths[i] > model->rest_wavelengths[i - 1]))
      return set_error(GPDLA_EINVAL, "rest_wavelengths must be strictly increasing");
  if (samples->num_samples < 1 || !samples->offset_samples || !samples->nhi_samples)
    return set_error(GPDLA_EINVAL, "invalid samples");
  // column densities: the sweeps' exp needs N >= 0 and finite (kernels.hip likelihood_kernel bounds
  // N tot by them); generate_dla_samples.m:20-53 only produces positive N_HI
  for (int64_t i = 0; i < samples->num_samples; ++i)
    if (!(samples->nhi_samples[i] >= 0.0 && samples->nhi_samples[i] < INFINITY))
      return set_error(GPDLA_EINVAL, "nhi_samples[%lld] = %g: column densities must be finite and >= 0",
                       (long long)i, samples->nhi_samples[i]);
  // offsets: any finite value (z_DLA = zmin + (zmax - zmin) offset, process_qsos.m:163-165, outside
  // [0, 1] included); a NaN would make the sort below compare without a strict weak order
  for (int64_t i = 0; i < samples->num_samples; ++i)
    if (!std::isfinite(samples->offset_samples[i]))
      return set_error(GPDLA_EINVAL, "offset_samples[%lld] = %g: offsets must be finite",
                       (long long)i, samples->offset_samples[i]);

  HIP_TRY(hipSetDevice(device));
  gpdla_engine* e = new gpdla_engine();
  e->device = device;
  e->K = use_gemm ? model->k : (use_i8 ? k_i8 : k_fused);  // the rank the kernels run at
  e->S = samples->num_samples;
  e->gemm = use_gemm;
  e->i8 = use_i8;
  e->i8_nd = params->path == GPDLA_PATH_PANEL_GEMM_I8_24 ? 3 : 4;
  e->params = *params;
  e->num_rest = model->num_rest;
  e->c0 = std::exp(model->log_c_0);     // process_qsos.m:84-86
  e->tau0 = std::exp(model->log_tau_0);
  e->beta = std::exp(model->log_beta);
  {  // omega^2 = exp(2 log omega) sf^2 with sf = 1 - exp(-tau_0 (1 + z)^beta) + c_0 in [c_0, 1 + c_0]
    double lo_max = -INFINITY;
    for (int i = 0; i < model->num_rest; ++i) lo_max = std::max(lo_max, model->log_omega[i]);
    const double om2_max = std::exp(2 * lo_max) * (1 + e->c0) * (1 + e->c0);
    e->om2_hi_e = (om2_max > 0 && om2_max < INFINITY) ? (int32_t)std::ilogb(om2_max) : 0;
  }
  auto fail = [&](int code) { gpdla_engine_destroy(e); return code; };
#define TRY_E(x) do { int r_ = (x); if (r_) return fail(r_); } while (0)
  if (hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking) != hipSuccess)
    return fail(set_error(GPDLA_EDEVICE, "hipStreamCreate failed"));
  e->stream = e->own_stream;
  if (hipEventCreateWithFlags(&e->meta_done, hipEventDisableTiming) != hipSuccess)
    return fail(set_error(GPDLA_EDEVICE, "hipEventCreate failed"));


  const size_t G = model->num_rest, K = e->K, k_model = model->k;
  std::vector<double> Mrow(G * K, 0.0);  // columns k_model..K-1: the fused paths' zero padding
  for (size_t g = 0; g < G; ++g)
    for (size_t c = 0; c < k_model; ++c) Mrow[g * K + c] = model->M[g + c * G];  // col-major -> row-major
  size_t dummy = 0;
  TRY_E(grow(&e->d_rest, &dummy, G)); dummy = 0;
  TRY_E(grow(&e->d_mu, &dummy, G)); dummy = 0;
  TRY_E(grow(&e->d_M, &dummy, G * K)); dummy = 0;
  TRY_E(grow(&e->d_logom, &dummy, G)); dummy = 0;
  TRY_E(grow(&e->d_off, &dummy, (size_t)e->S)); dummy = 0;
  TRY_E(grow(&e->d_nhi, &dummy, (size_t)e->S)); dummy = 0;
  TRY_E(grow(&e->d_perm, &dummy, (size_t)e->S)); dummy = 0;
  const std::vector<double>& lines = host_line_data().buf;
  TRY_E(grow(&e->d_lines, &dummy, lines.size())); dummy = 0;
  TRY_E(grow(&e->d_status, &dummy, 1));
  TRY_E(upload(e->d_rest, model->rest_wavelengths, G * 8, e->stream));
  TRY_E(upload(e->d_mu, model->mu, G * 8, e->stream));
  TRY_E(upload(e->d_M, Mrow.data(), G * K * 8, e->stream));
  TRY_E(upload(e->d_logom, model->log_omega, G * 8, e->stream));
  // Samples are swept in ascending offset order: z_DLA = zmin + (zmax - zmin) offset is then
  // ascending for every spectrum, so the 16 samples of a wave put their line centres on nearly
  // the same pixels and the divergent |x| < kCoreX branch is taken in few steps.  Each sample's
  // arithmetic is lane-independent, so results are unchanged; outputs scatter back via d_perm.
  std::vector<int32_t> perm((size_t)e->S);
  for (int64_t i = 0; i < e->S; ++i) perm[i] = (int32_t)i;
  std::stable_sort(perm.begin(), perm.end(), [&](int32_t a, int32_t b) {
    return samples->offset_samples[a] < samples->offset_samples[b];
  });
  std::vector<double> off_sorted((size_t)e->S), nhi_sorted((size_t)e->S);
  for (int64_t i = 0; i < e->S; ++i) {
    off_sorted[i] = samples->offset_samples[perm[i]];
    nhi_sorted[i] = samples->nhi_samples[perm[i]];
  }
  TRY_E(upload(e->d_off, off_sorted.data(), (size_t)e->S * 8, e->stream));
  TRY_E(upload(e->d_nhi, nhi_sorted.data(), (size_t)e->S * 8, e->stream));
  TRY_E(upload(e->d_perm, perm.data(), (size_t)e->S * 4, e->stream));
  e->h_perm = perm;
  TRY_E(upload(e->d_lines, lines.data(), lines.size() * 8, e->stream));
  if (hipMemsetAsync(e->d_status, 0, 4, e->stream) != hipSuccess ||
      hipStreamSynchronize(e->stream) != hipSuccess)
    return fail(set_error(GPDLA_EDEVICE, "engine upload failed"));
#undef TRY_E
  *out = e;
  return GPDLA_OK;
}

int gpdla_engine_set_stream(gpdla_engine* e, void* hip_stream) {
  if (!e) return set_error(GPDLA_EINVAL, "null engine");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->stream = hip_stream ? (hipStream_t)hip_stream : e->own_stream;
  return GPDLA_OK;
}

int gpdla_engine_use_null_stream(gpdla_engine* e) {
  if (!e) return set_error(GPDLA_EINVAL, "null engine");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->stream = nullptr;  // the null stream (HIP's stream 0)
  return GPDLA_OK;
}

int gpdla_engine_set_panel_streams(gpdla_engine* e, int32_t n) {
  if (!e) return set_error(GPDLA_EINVAL, "null engine");
  if (n < 1 || n > gpdla_engine::kMaxPanelStreams)
    return set_error(GPDLA_EINVAL, "panel streams must be 1..%d (got %d)", gpdla_engine::kMaxPanelStreams, (int)n);
  e->panel_streams = n;
  return GPDLA_OK;
}

// Panel-GEMM path for one batch: per spectrum and chunk of samples, weights -> GEMM on the matrix
// cores (int8 digits, gemm_i8.hip, or fp64, gemm_f64.hip) -> batched LDL^T (gemm_path.hip), in
// stream order.
// A batch's spectra alternate over two streams (gpdla_engine_set_panel_streams), which
// fills the last partial round of each spectrum's weights / LDL^T launches with the other spectrum's
// work: +3.6% on configs[4] (profiles/round5/ab/r11a).  (Earlier second-stream layouts, within one
// spectrum, measured no gain: the LDL^T beside the next chunk's weights and GEMM, 0% with the
// matrix-core LDL^T (profiles/r2f); the weights beside the previous chunk's GEMM, +0.5% (profiles/r2c).)
static int run_panel_gemm(gpdla_engine* e, bool i8, int64_t nq, const int64_t* h_sb, const int64_t* h_lb,
                          const int64_t* h_cap, const int64_t* h_cb, int64_t sc_max, double* o_sll,
                          int64_t ld, double* o_null, hipStream_t st) {
  const int K = e->K;
  const int64_t E = (int64_t)K * (K + 1) / 2;
  const int64_t rows = (sc_max + 127) / 128 * 128;
  // several compute streams: spectrum q on stream q % ns with workspace set q % ns, forked
  // from and joined back into st (the batch's prep / convert before, its reduce after)
  const int ns = (int)std::min<int64_t>(e->panel_streams, nq);
  if (ns > 1) {
    if (!e->panel_fork) HIP_TRY(hipEventCreateWithFlags(&e->panel_fork, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(e->panel_fork, st));
    for (int i = 1; i < ns; ++i) {
      if (!e->panel_stream[i]) HIP_TRY(hipStreamCreateWithFlags(&e->panel_stream[i], hipStreamNonBlocking));
      if (!e->panel_join[i]) HIP_TRY(hipEventCreateWithFlags(&e->panel_join[i], hipEventDisableTiming));
      HIP_TRY(hipStreamWaitEvent(e->panel_stream[i], e->panel_fork, 0));
    }
  }
  const hipStream_t st0 = st;
  auto enqueue = [&]() -> int {
    for (int64_t q = 0; q < nq; ++q) {
      const int set = (int)(q % ns);
      st = set ? e->panel_stream[set] : st0;
      double *G = e->d_G + set * e->ws_G, *U = e->d_U + set * e->ws_U;
      double *q1p = e->d_q1p + set * e->ws_wp, *ldp = e->d_ldp + set * e->ws_wp;
      for (int64_t s0 = 0; s0 <= e->S; s0 += sc_max) {
        const int32_t sc = (int32_t)std::min<int64_t>(sc_max, e->S + 1 - s0);
        if (i8) {  // int8 Ozaki contraction (gemm_i8.hip): weights digits -> exact GEMM -> Gram, u
          const int64_t ks = i8_gemm_kstride(h_cap[q]);
          const int nd = i8_spectrum_nd(e->i8_nd, h_cap[q]);  // short spectra: 32-bit digits (internal.h)
          uint8_t* adig = e->d_ai8 + set * e->ws_ai8;
          WeightsI8Args wi{};
          wi.info = e->d_info; wi.q = (int32_t)q;
          wi.srow = e->d_srow + h_sb[q] * 8; wi.lam_pad = e->d_lam + h_lb[q]; wi.kstride = ks;
          wi.offsets = e->d_off; wi.nhi = e->d_nhi; wi.S = e->S; wi.s0 = s0; wi.sc = sc; wi.rows = rows;
          wi.lines = make_line_args(e->d_lines); wi.nd = nd; wi.adig = adig; wi.q1p = q1p; wi.ldp = ldp;
          HIP_TRY(launch_weights_i8(wi, st));
          GemmI8Args gi{};
          gi.info = e->d_info; gi.q = (int32_t)q; gi.k = K; gi.kstride = ks; gi.rows = rows; gi.sc = sc; gi.nd = nd;
          gi.adig = adig; gi.bdig = e->d_pi8 + h_cb[q];
          gi.ent = e->d_pent + q * 2 * (int64_t)i8_gemm_entries(K); gi.G = G; gi.U = U;
          // the 24-bit path stores the Gram in fp32 (half the GEMM -> LDL^T round trip; adds ~1e-8
          // to its ~2e-7 from fp64, tests/support/emulate_i8.py), in the same workspace
          gi.G32 = nd == 3 ? reinterpret_cast<float*>(G) : nullptr;
          gi.ks_bound = i8_ks_bound(h_cap[q]);  // slot_cap = 4 ceil(lpix / 4) + 16
          TimedLaunch tg{};
          int rc;
          if ((rc = record_start(e, &tg, 3, st))) return rc;
          HIP_TRY(launch_gemm_i8(gi, st));
          HIP_TRY(hipEventRecord(tg.stop, st));
          e->pending.push_back(tg);
        } else {
          WeightsArgs wa{};
          wa.info = e->d_info; wa.q = (int32_t)q;
          wa.srow = e->d_srow + h_sb[q] * 8; wa.lam_pad = e->d_lam + h_lb[q]; wa.cap = h_cap[q];
          wa.offsets = e->d_off; wa.nhi = e->d_nhi; wa.S = e->S; wa.s0 = s0; wa.sc = sc;
          wa.num_lines = e->params.num_lines; wa.lines = make_line_args(e->d_lines);
          double *wg = e->d_wg + set * e->ws_w, *wu = e->d_wu + set * e->ws_w;
          wa.wg = wg; wa.wu = wu; wa.q1p = q1p; wa.ldp = ldp;
          HIP_TRY(launch_weights(wa, st));
          // Gram[s][e] = sum_t Wg[t][s] PG[t][e] (the slot-major Khatri-Rao rows), u[s][i] likewise
          // over the M rows, on the f64 matrix cores (gemm_f64.hip)
          GemmF64Args ga{};
          ga.seg[0] = GemmF64Seg{wg, e->d_panel + h_sb[q] * gemm_ldp(K), gemm_ldp(K), (int32_t)E, G};
          ga.seg[1] = GemmF64Seg{wu, e->d_pm + h_sb[q] * gemm_ldm(K), gemm_ldm(K), K, U};
          ga.nseg = 2;
          ga.cap = h_cap[q]; ga.cap16 = gemm_f64_cap16(h_cap[q]); ga.sc = sc;
          TimedLaunch tg{};
          int rc;
          if ((rc = record_start(e, &tg, 3, st))) return rc;
          HIP_TRY(launch_gemm_f64(ga, st));
          HIP_TRY(hipEventRecord(tg.stop, st));
          e->pending.push_back(tg);
        }
        LdlArgs da{};
        da.info = e->d_info; da.q = (int32_t)q; da.k = K;
        da.G = G; da.U = U; da.q1p = q1p; da.ldp = ldp;
        da.G32 = (i8 && i8_spectrum_nd(e->i8_nd, h_cap[q]) == 3) ? reinterpret_cast<const float*>(G) : nullptr;
        da.S = e->S; da.s0 = s0; da.sc = sc; da.perm = e->d_perm;
        da.sample_ll = o_sll ? o_sll + q * ld : nullptr; da.ll_null = o_null + q; da.status = e->d_status;
        HIP_TRY(launch_ldl_batch(da, st));
      }
    }
    return GPDLA_OK;
  };
  const int rc = enqueue();
  // joined even after a failed enqueue: later work on st0 (the next batch reusing the workspace sets,
  // the engine's synchronize) stays ordered after everything already on the other streams
  for (int i = 1; i < ns; ++i) {
    HIP_TRY(hipEventRecord(e->panel_join[i], e->panel_stream[i]));
    HIP_TRY(hipStreamWaitEvent(st0, e->panel_join[i], 0));
  }
  return rc;
}

// The host-buffer pipeline's stages, sized for the largest batch of this call (no reallocation
// while copies or kernels may still use a stage), its copy stream and events.
static int host_stages_prepare(gpdla_engine* e, int64_t max_pix, int64_t max_q) {
  if (!e->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
  for (HostStage& h : e->hs) {
    int rc;
    if ((rc = grow(&h.wl, &h.cap_wl, (size_t)max_pix))) return rc;
    if ((rc = grow(&h.flux, &h.cap_flux, (size_t)max_pix))) return rc;
    if ((rc = grow(&h.noise, &h.cap_noise, (size_t)max_pix))) return rc;
    if ((rc = grow(&h.mask, &h.cap_mask, (size_t)max_pix))) return rc;
    if ((rc = grow(&h.z, &h.cap_z, (size_t)max_q))) return rc;
    if ((rc = grow(&h.sll, &h.cap_sll, (size_t)(max_q * e->S)))) return rc;
    if ((rc = grow(&h.llnull, &h.cap_o[0], (size_t)max_q))) return rc;
    if ((rc = grow(&h.lldla, &h.cap_o[1], (size_t)max_q))) return rc;
    if ((rc = grow(&h.zmin, &h.cap_o[2], (size_t)max_q))) return rc;
    if ((rc = grow(&h.zmax, &h.cap_o[3], (size_t)max_q))) return rc;
    if ((rc = grow(&h.npix, &h.cap_o[4], (size_t)max_q))) return rc;
    for (hipEvent_t* ev : {&h.in_ready, &h.in_free, &h.out_ready, &h.out_free})
      if (!*ev) HIP_TRY(hipEventCreateWithFlags(ev, hipEventDisableTiming));
  }
  return GPDLA_OK;
}

// Batch [q0, q0 + nq)'s results from its stage back to the host, on the copy stream once the
// compute stream has written them.  With pageable host memory the call returns when the copy is
// done; the caller has already queued the next batch's kernels, so the device keeps computing.
static int host_stage_copy_out(gpdla_engine* e, const gpdla_results* res, int64_t bi, int64_t q0, int64_t nq) {
  HostStage& h = e->hs[bi & 1];
  hipStream_t cs = e->copy_stream;
  HIP_TRY(hipStreamWaitEvent(cs, h.out_ready, 0));
  HIP_TRY(hipMemcpyAsync(res->log_likelihoods_no_dla + q0, h.llnull, nq * 8, hipMemcpyDeviceToHost, cs));
  HIP_TRY(hipMemcpyAsync(res->log_likelihoods_dla + q0, h.lldla, nq * 8, hipMemcpyDeviceToHost, cs));
  if (res->min_z_dlas) HIP_TRY(hipMemcpyAsync(res->min_z_dlas + q0, h.zmin, nq * 8, hipMemcpyDeviceToHost, cs));
  if (res->max_z_dlas) HIP_TRY(hipMemcpyAsync(res->max_z_dlas + q0, h.zmax, nq * 8, hipMemcpyDeviceToHost, cs));
  if (res->num_pixels) HIP_TRY(hipMemcpyAsync(res->num_pixels + q0, h.npix, nq * 4, hipMemcpyDeviceToHost, cs));
  if (res->sample_log_likelihoods_dla)
    HIP_TRY(hipMemcpy2DAsync(res->sample_log_likelihoods_dla + q0 * res->sample_ld, res->sample_ld * 8, h.sll,
                             e->S * 8, e->S * 8, nq, hipMemcpyDeviceToHost, cs));
  HIP_TRY(hipEventRecord(h.out_free, cs));
  return GPDLA_OK;
}

int gpdla_engine_process(gpdla_engine* e, const gpdla_spectra* sp, const gpdla_results* res) {
  if (!e || !sp || !res) return set_error(GPDLA_EINVAL, "null argument");
  const int64_t Q = sp->num_spectra;
  if (Q < 0) return set_error(GPDLA_EINVAL, "num_spectra < 0");
  if (Q == 0) return GPDLA_OK;
  if (!sp->offsets || !sp->wavelengths || !sp->flux || !sp->noise_variance || !sp->pixel_mask || !sp->z_qsos)
    return set_error(GPDLA_EINVAL, "null spectra array");
  if (!res->log_likelihoods_no_dla || !res->log_likelihoods_dla)
    return set_error(GPDLA_EINVAL, "null result array");
  if (res->sample_log_likelihoods_dla && res->sample_ld < e->S)
    return set_error(GPDLA_EINVAL, "sample_ld (%lld) < num_samples (%lld)", (long long)res->sample_ld,
                     (long long)e->S);
  if (sp->offsets[0] < 0) return set_error(GPDLA_EINVAL, "offsets[0] < 0");
  for (int64_t q = 0; q < Q; ++q)
    if (sp->offsets[q + 1] < sp->offsets[q]) return set_error(GPDLA_EINVAL, "offsets not monotone at %lld", (long long)q);
  const bool in_dev = sp->memory == GPDLA_MEM_DEVICE, out_dev = res->memory == GPDLA_MEM_DEVICE;
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t st = e->stream;

  const int64_t QB = e->params.max_batch_spectra > 0 ? e->params.max_batch_spectra : (e->gemm ? 64 : 1024);
  // panel doubles per slot: fused layout row, or the Khatri-Rao row of the panel-GEMM layout
  const int64_t E = (int64_t)e->K * (e->K + 1) / 2;
  const int64_t row = e->gemm ? gemm_ldp(e->K) : panel_row_doubles(e->K);
  const int es = e->gemm ? 0 : scratch_doubles(e->K);
  // panel-GEMM sample chunks: the S + 1 samples (null model included) in equal chunks of at most
  // kMaxChunk.  configs[4] (S + 1 = 100,001) measured 46.2 Mevals/s with 16,384-sample chunks (6
  // full + a 1,697-sample tail that fills a sixth of the GPU), 47.4 with 7 equal chunks, 48.5 with
  // 2 and 49.1 with one (profiles/r2l); again after the round-2 GEMM work: 53.5 (6 equal chunks),
  // 58.8 (4), 61.7 (2), 63.1 (one; profiles/r2/c5_ab): smaller chunks keep the A digits in the
  // Infinity Cache (GEMM -10%) but cost more in the weights and LDL^T launches.  The chunk is also
  // capped per batch by a workspace budget (panel_chunk below): per sample, the A digits (8 B per
  // slot) or the fp64 weights (16 B per slot), plus the Gram and u (8 (k(k+1)/2 + k) B).
  constexpr int64_t kMaxChunk = GPDLA_MAX_CHUNK;
  const int64_t blocks_x = (e->S + 1 + kSamplesPerBlock - 1) / kSamplesPerBlock;

  // pinned metadata for every batch of this call: per batch (QB+1) + 4*QB int64
  const size_t per_batch = (size_t)(QB + 1) + 4 * (size_t)QB;
  const int64_t nbatch = (Q + QB - 1) / QB;
  HIP_TRY(hipEventSynchronize(e->meta_done));
  if (e->cap_hmeta < per_batch * nbatch) {
    if (e->h_meta) (void)hipHostFree(e->h_meta);
    e->h_meta = nullptr;
    e->cap_hmeta = 0;
    HIP_TRY(hipHostMalloc((void**)&e->h_meta, per_batch * nbatch * sizeof(int64_t)));
    e->cap_hmeta = per_batch * nbatch;
  }

  // host inputs and host results: the two-stage pipeline (copies beside the kernels)
  const bool pipe = !in_dev && !out_dev;
  if (pipe) {
    int64_t max_pix = 0;
    for (int64_t bi = 0; bi < nbatch; ++bi)
      max_pix = std::max(max_pix, sp->offsets[std::min(Q, (bi + 1) * QB)] - sp->offsets[bi * QB]);
    int rc;
    // no copy or kernel of an earlier call (one that returned an error mid-loop included) may still
    // use a stage that host_stages_prepare is about to free and grow
    if (e->copy_stream) HIP_TRY(hipStreamSynchronize(e->copy_stream));
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = host_stages_prepare(e, max_pix, std::min(Q, QB)))) return rc;
    // order this call after any other work on the engine's stream, then keep the two streams apart
    // except through the events
    HIP_TRY(hipStreamSynchronize(e->copy_stream));
    for (HostStage& h : e->hs) {
      HIP_TRY(hipEventRecord(h.in_free, st));
      HIP_TRY(hipEventRecord(h.out_free, e->copy_stream));
    }
  }

  for (int64_t bi = 0; bi < nbatch; ++bi) {
    const int64_t q0 = bi * QB, q1 = std::min(Q, q0 + QB), nq = q1 - q0;
    HostStage& hst = e->hs[bi & 1];
    int64_t* hm = e->h_meta + bi * per_batch;
    int64_t* h_off = hm;
    int64_t* h_sb = hm + (QB + 1);
    int64_t* h_lb = h_sb + QB;
    int64_t* h_cap = h_lb + QB;
    int64_t* h_cb = h_cap + QB;  // int8 path: first chunk of each spectrum
    int64_t slots = 0, lams = 0, cap_max = 0, chunks = 0, lpix_max = 0;
    for (int64_t q = 0; q < nq; ++q) {
      h_off[q] = sp->offsets[q0 + q] - sp->offsets[q0];
      const int64_t lpix = sp->offsets[q0 + q + 1] - sp->offsets[q0 + q];
      const int64_t cap = 4 * ((lpix + 3) / 4) + 4 * kChunkSteps;
      h_sb[q] = slots;
      h_lb[q] = lams;
      h_cap[q] = cap;
      if (e->gemm) {  // int8 panel-GEMM: byte base of the spectrum's B digit planes
        h_cb[q] = chunks;
        chunks += 4 * (int64_t)i8_gemm_entries(e->K) * i8_gemm_kstride(cap);
      } else {
        h_cb[q] = chunks;
        chunks += ((lpix + 3) / 4 + 15) / 16;  // >= ceil(L / 16) chunks of 16 steps per segment
      }
      lpix_max = std::max(lpix_max, lpix);
      cap_max = std::max(cap_max, cap);
      slots += cap;
      lams += cap + 8;
    }
    h_off[nq] = sp->offsets[q1] - sp->offsets[q0];
    const int64_t npix = h_off[nq];
    // int8 contraction for this batch: its int32 level sums are exact only up to kI8MaxSlots
    // slots, so a batch holding a longer spectrum runs the fp64 kernels (fused or dgemm) instead
    const bool i8_exact = lpix_max <= kI8MaxSlots;
    const bool batch_i8 = e->i8 && !e->gemm && i8_exact;
    const bool batch_gemm_i8 = e->i8 && e->gemm && i8_exact;
    // panel-GEMM sample chunk of this batch: equal chunks of at most kMaxChunk samples whose
    // workspaces fit the budget (a quarter of the free device memory, at most 16 GiB)
    int64_t sc_max = 0;
    if (e->gemm) {
      size_t free_b = 0, total_b = 0;
      HIP_TRY(hipMemGetInfo(&free_b, &total_b));
      const int64_t budget = (int64_t)std::min<size_t>(free_b / 4, (size_t)16 << 30);
      // (one workspace set per panel stream)
      const int64_t per_sample = e->panel_streams *
                                 ((batch_gemm_i8 ? 8 * i8_gemm_kstride(cap_max) : 16 * gemm_f64_cap16(cap_max)) +
                                  8 * (E + e->K + 2 * kWeightParts));
      const int64_t fit = std::max<int64_t>(128, budget / std::max<int64_t>(per_sample, 1) / 128 * 128);
      const int64_t cmax = std::min<int64_t>(kMaxChunk, fit);
      const int64_t nchunk = (e->S + 1 + cmax - 1) / cmax;
      sc_max = (e->S + 1 + nchunk - 1) / nchunk;
    }

    int rc;
    if ((rc = grow(&e->d_meta, &e->cap_meta, per_batch))) return rc;
    if ((rc = grow(&e->d_info, &e->cap_q, (size_t)QB))) return rc;
    // + one LDS row of slack: the staging DMA reads whole 1 KiB pieces (kernels.hip stage_chunk).  The
    // int8 panel batches never read the Khatri-Rao panel (prep skips it, convert_gemm_i8_kernel forms
    // the products from the M rows), so they do not grow it (a few hundred MB at k = 50)
    if (!batch_gemm_i8 &&
        (rc = grow(&e->d_panel, &e->cap_slots,
                   (size_t)(slots * row + (e->gemm ? gemm_panel_slack(row) : panel_lds_row_doubles(e->K)))))) return rc;
    if ((rc = grow(&e->d_lam, &e->cap_lam, (size_t)lams))) return rc;
    if (e->gemm) {
      const int64_t ldm = gemm_ldm(e->K);
      if ((rc = grow(&e->d_pm, &e->cap_pm, (size_t)(slots * ldm + gemm_panel_slack(ldm))))) return rc;
      // the rows gemm_f64 reads past the batch's last slot: zero (finite, against zero weights)
      if (!batch_gemm_i8) HIP_TRY(hipMemsetAsync(e->d_panel + slots * row, 0, gemm_panel_slack(row) * 8, st));
      HIP_TRY(hipMemsetAsync(e->d_pm + slots * ldm, 0, gemm_panel_slack(ldm) * 8, st));
      if ((rc = grow(&e->d_srow, &e->cap_srow, (size_t)slots * 8))) return rc;
      const int64_t sets = e->panel_streams;  // one workspace set per panel stream
      if (!batch_gemm_i8) {  // the fp64 weight tiles: only the fp64 GEMM reads them
        e->ws_w = gemm_f64_cap16(cap_max) * gemm_f64_rows(sc_max);
        if ((rc = grow(&e->d_wg, &e->cap_wg, (size_t)(sets * e->ws_w)))) return rc;
        if ((rc = grow(&e->d_wu, &e->cap_wu, (size_t)(sets * e->ws_w)))) return rc;
      }
      // the GEMMs store whole 128-sample tiles (quad_index layout, internal.h); + 64 elements of
      // slack: ldl_mfma_kernel's straight-line tile loads may address one entry past the last
      // sample's Gram when k is a multiple of 4 (the value is discarded)
      const int64_t grows = gemm_f64_rows(sc_max);
      e->ws_G = E * grows + 64;
      e->ws_U = e->K * grows + 64;
      e->ws_wp = kWeightParts * sc_max;
      if ((rc = grow(&e->d_G, &e->cap_G, (size_t)(sets * e->ws_G)))) return rc;
      if ((rc = grow(&e->d_U, &e->cap_U, (size_t)(sets * e->ws_U)))) return rc;
      if ((rc = grow(&e->d_q1p, &e->cap_q1p, (size_t)(sets * e->ws_wp)))) return rc;
      if ((rc = grow(&e->d_ldp, &e->cap_ldp, (size_t)(sets * e->ws_wp)))) return rc;
    }
    if (batch_gemm_i8) {
      if ((rc = grow(&e->d_pi8, &e->cap_pi8, (size_t)chunks))) return rc;
      if ((rc = grow(&e->d_pent, &e->cap_pent, (size_t)nq * 2 * i8_gemm_entries(e->K)))) return rc;
      e->ws_ai8 = (int64_t)8 * ((sc_max + 127) / 128 * 128) * i8_gemm_kstride(cap_max + 0);
      if ((rc = grow(&e->d_ai8, &e->cap_ai8, (size_t)(e->panel_streams * e->ws_ai8)))) return rc;
    }
    if (batch_i8) {  // (the fp64 fused kernel transposes its accumulators in registers: no scratch)
      if ((rc = grow(&e->d_scratch, &e->cap_scr, (size_t)blocks_x * nq * kSamplesPerBlock * es))) return rc;
      if ((rc = grow(&e->d_pi8, &e->cap_pi8, (size_t)chunks * i8_chunk_bytes(e->K)))) return rc;
      if ((rc = grow(&e->d_psc, &e->cap_psc, (size_t)chunks * 64 * 8))) return rc;
      if ((rc = grow(&e->d_pent, &e->cap_pent, (size_t)nq * 2 * i8_entries(e->K)))) return rc;
    }
    if ((rc = grow(&e->d_smap, &e->cap_smap, (size_t)slots))) return rc;
    HIP_TRY(hipMemcpyAsync(e->d_meta, hm, per_batch * sizeof(int64_t), hipMemcpyHostToDevice, st));

    const double *wl, *fl, *nv, *zq;
    const uint8_t* mk;
    const int64_t pbase = sp->offsets[q0];
    if (in_dev) {
      wl = sp->wavelengths + pbase; fl = sp->flux + pbase; nv = sp->noise_variance + pbase;
      mk = sp->pixel_mask + pbase; zq = sp->z_qsos + q0;
    } else if (pipe) {
      // into this batch's stage once batch bi - 2's prep_kernel has read it, beside batch bi - 1
      hipStream_t cs = e->copy_stream;
      HIP_TRY(hipStreamWaitEvent(cs, hst.in_free, 0));
      HIP_TRY(hipMemcpyAsync(hst.wl, sp->wavelengths + pbase, npix * 8, hipMemcpyHostToDevice, cs));
      HIP_TRY(hipMemcpyAsync(hst.flux, sp->flux + pbase, npix * 8, hipMemcpyHostToDevice, cs));
      HIP_TRY(hipMemcpyAsync(hst.noise, sp->noise_variance + pbase, npix * 8, hipMemcpyHostToDevice, cs));
      HIP_TRY(hipMemcpyAsync(hst.mask, sp->pixel_mask + pbase, npix, hipMemcpyHostToDevice, cs));
      HIP_TRY(hipMemcpyAsync(hst.z, sp->z_qsos + q0, nq * 8, hipMemcpyHostToDevice, cs));
      HIP_TRY(hipEventRecord(hst.in_ready, cs));
      HIP_TRY(hipStreamWaitEvent(st, hst.in_ready, 0));
      wl = hst.wl; fl = hst.flux; nv = hst.noise; mk = hst.mask; zq = hst.z;
    } else {
      if ((rc = grow(&e->d_wl, &e->cap_wl, (size_t)npix))) return rc;
      if ((rc = grow(&e->d_flux, &e->cap_flux, (size_t)npix))) return rc;
      if ((rc = grow(&e->d_noise, &e->cap_noise, (size_t)npix))) return rc;
      if ((rc = grow(&e->d_mask, &e->cap_mask, (size_t)npix))) return rc;
      if ((rc = grow(&e->d_z, &e->cap_z, (size_t)nq))) return rc;
      HIP_TRY(hipMemcpyAsync(e->d_wl, sp->wavelengths + pbase, npix * 8, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(e->d_flux, sp->flux + pbase, npix * 8, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(e->d_noise, sp->noise_variance + pbase, npix * 8, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(e->d_mask, sp->pixel_mask + pbase, npix, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(e->d_z, sp->z_qsos + q0, nq * 8, hipMemcpyHostToDevice, st));
      wl = e->d_wl; fl = e->d_flux; nv = e->d_noise; mk = e->d_mask; zq = e->d_z;
    }

    // outputs: device results are written in place; host results go through workspaces
    double *o_sll, *o_null, *o_dla, *o_zmin, *o_zmax;
    int32_t* o_npix;
    int64_t ld;
    const bool need_internal_sll = !pipe && (!out_dev || !res->sample_log_likelihoods_dla);
    if (need_internal_sll) {
      if ((rc = grow(&e->d_sll, &e->cap_sll, (size_t)nq * e->S))) return rc;
    }
    if (out_dev) {
      o_sll = res->sample_log_likelihoods_dla ? res->sample_log_likelihoods_dla + q0 * res->sample_ld : e->d_sll;
      ld = res->sample_log_likelihoods_dla ? res->sample_ld : e->S;
      o_null = res->log_likelihoods_no_dla + q0;
      o_dla = res->log_likelihoods_dla + q0;
      o_zmin = res->min_z_dlas ? res->min_z_dlas + q0 : nullptr;
      o_zmax = res->max_z_dlas ? res->max_z_dlas + q0 : nullptr;
      o_npix = res->num_pixels ? res->num_pixels + q0 : nullptr;
    } else if (pipe) {
      // this batch's stage, once batch bi - 2's results have left it
      HIP_TRY(hipStreamWaitEvent(st, hst.out_free, 0));
      o_sll = hst.sll; ld = e->S;
      o_null = hst.llnull; o_dla = hst.lldla; o_zmin = hst.zmin; o_zmax = hst.zmax; o_npix = hst.npix;
    } else {
      if (e->cap_qout < (size_t)QB) {
        for (double** p : {&e->d_llnull, &e->d_lldla, &e->d_zmin, &e->d_zmax})
          if (*p) { (void)hipFree(*p); *p = nullptr; }
        if (e->d_npix) { (void)hipFree(e->d_npix); e->d_npix = nullptr; }
        size_t a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0;
        if ((rc = grow(&e->d_llnull, &a1, (size_t)QB))) return rc;
        if ((rc = grow(&e->d_lldla, &a2, (size_t)QB))) return rc;
        if ((rc = grow(&e->d_zmin, &a3, (size_t)QB))) return rc;
        if ((rc = grow(&e->d_zmax, &a4, (size_t)QB))) return rc;
        if ((rc = grow(&e->d_npix, &a5, (size_t)QB))) return rc;
        e->cap_qout = QB;
      }
      o_sll = e->d_sll; ld = e->S;
      o_null = e->d_llnull; o_dla = e->d_lldla; o_zmin = e->d_zmin; o_zmax = e->d_zmax; o_npix = e->d_npix;
    }

    PrepArgs pa{};
    pa.q_count = (int32_t)nq;
    pa.offsets = e->d_meta;
    pa.wavelengths = wl; pa.flux = fl; pa.noise = nv; pa.mask = mk; pa.z_qsos = zq;
    pa.slot_base = e->d_meta + (QB + 1);
    pa.lam_base = pa.slot_base + QB;
    pa.slot_cap = pa.lam_base + QB;
    pa.num_rest = e->num_rest;
    pa.rest = e->d_rest; pa.mu = e->d_mu; pa.M_rowmajor = e->d_M; pa.log_omega = e->d_logom;
    pa.c_0 = e->c0; pa.tau_0 = e->tau0; pa.beta = e->beta;
    pa.min_lambda = e->params.min_lambda; pa.max_lambda = e->params.max_lambda;
    pa.lya = e->params.lya_wavelength; pa.lyman_limit = e->params.lyman_limit;
    pa.min_z_cut = e->params.min_z_cut; pa.max_z_cut = e->params.max_z_cut;
    pa.pixel_spacing = e->params.pixel_spacing;
    pa.absorption_mode = e->params.absorption_mode;
    pa.om2_hi_e = e->om2_hi_e;
    pa.info = e->d_info; pa.panel = e->d_panel; pa.lam_pad = e->d_lam; pa.slot_pixel = e->d_smap;
    pa.k = e->K; pa.panel_m = e->d_pm; pa.srow = e->d_srow;
    // the int8 panel paths form the Khatri-Rao entries from the M rows (convert_gemm_i8_kernel): prep
    // skips the k(k+1)/2 doubles per slot
    if (batch_gemm_i8) pa.panel = nullptr;

    LikelihoodArgs la{};
    la.q_count = (int32_t)nq;
    la.info = e->d_info; la.panel = e->d_panel; la.lam_pad = e->d_lam;
    la.offsets = e->d_off; la.nhi = e->d_nhi; la.perm = e->d_perm; la.S = e->S;
    la.num_lines = e->params.num_lines;
    la.lines = make_line_args(e->d_lines);
    la.sample_ll = o_sll; la.ld = ld; la.ll_null = o_null; la.status = e->d_status;

    ConvertI8Args ca{};
    LikelihoodI8Args li{};
    if (batch_i8) {
      ca.q_count = (int32_t)nq; ca.info = e->d_info; ca.panel = e->d_panel; ca.lam_pad = e->d_lam;
      ca.chunk_base = pa.slot_cap + QB; ca.panel_i8 = e->d_pi8; ca.scal = e->d_psc; ca.ent = e->d_pent;
      li.q_count = (int32_t)nq; li.info = e->d_info; li.panel_i8 = e->d_pi8; li.scal = e->d_psc;
      li.ent = e->d_pent; li.chunk_base = ca.chunk_base; li.lam_pad = e->d_lam;
      li.offsets = e->d_off; li.nhi = e->d_nhi; li.perm = e->d_perm; li.S = e->S;
      li.lines = la.lines; li.scratch = e->d_scratch;
      li.sample_ll = o_sll; li.ld = ld; li.ll_null = o_null; li.status = e->d_status;
    }

    ReduceArgs ra{};
    ra.q_count = (int32_t)nq; ra.info = e->d_info; ra.sample_ll = o_sll; ra.ld = ld; ra.S = e->S;
    ra.ll_dla = o_dla; ra.zmin = o_zmin; ra.zmax = o_zmax; ra.num_pixels = o_npix;

    TimedLaunch t0{}, t1{}, t2{};
    if ((rc = record_start(e, &t0, 0))) return rc;
    HIP_TRY(launch_prep(e->gemm ? 0 : e->K, pa, st));
    if (pipe && !e->forest_on) HIP_TRY(hipEventRecord(hst.in_free, st));
    if (batch_i8) HIP_TRY(launch_convert_i8(e->K, ca, st));
    if (batch_gemm_i8) {
      ConvertGemmI8Args cg{};
      cg.k = e->K; cg.info = e->d_info; cg.panel_m = e->d_pm; cg.srow = e->d_srow;
      cg.slot_base = pa.slot_base; cg.slot_cap = pa.slot_cap; cg.bbase = pa.slot_cap + QB;
      cg.bdig = e->d_pi8; cg.ent = e->d_pent; cg.nd = e->i8_nd;
      HIP_TRY(launch_convert_gemm_i8(cg, (int32_t)nq, st));
    }
    HIP_TRY(hipEventRecord(t0.stop, st));
    e->pending.push_back(t0);
    if (e->forest_on) {  // (fused fp64 engines only: gpdla_engine_set_forest)
      ForestArgs fa{};
      fa.q_count = (int32_t)nq; fa.info = e->d_info; fa.offsets = e->d_meta; fa.wavelengths = wl; fa.z_qsos = zq;
      fa.slot_cap = pa.slot_cap; fa.slot_pixel = e->d_smap;
      fa.num_rest = e->num_rest; fa.rest = e->d_rest; fa.log_omega = e->d_logom;
      fa.c_0 = e->c0; fa.tau_0 = e->tau0; fa.beta = e->beta;
      fa.mf_tau_0 = e->forest.mean_flux_tau_0; fa.mf_beta = e->forest.mean_flux_beta;
      fa.num_lines = e->forest.num_forest_lines;
      fa.variance_series = e->forest.variance_series != 0; fa.mean_flux = e->forest.mean_flux != 0;
      fa.mean_flux_scope = e->forest_scope;
      fa.panel = e->d_panel;
      TimedLaunch t8{};
      if ((rc = record_start(e, &t8, 8))) return rc;
      HIP_TRY(launch_forest(e->K, fa, st));
      HIP_TRY(hipEventRecord(t8.stop, st));
      e->pending.push_back(t8);
      if (e->forest_scope != 0) {  // the mean flux on the M rows (and omega^2): gpdla_engine_set_forest_scoped
        TimedLaunch t8c{};
        if ((rc = record_start(e, &t8c, 8))) return rc;
        HIP_TRY(launch_forest_covariance(e->K, fa, st));
        HIP_TRY(hipEventRecord(t8c.stop, st));
        e->pending.push_back(t8c);
      }
      if (pipe) HIP_TRY(hipEventRecord(hst.in_free, st));  // the forest kernels read the wavelengths too
    }
    if ((rc = record_start(e, &t1, 1))) return rc;
    if (batch_i8) {
      HIP_TRY(launch_likelihood_i8(e->K, li, st));
    } else if (!e->gemm) {
      HIP_TRY(launch_likelihood(e->K, la, st));
    } else if ((rc = run_panel_gemm(e, batch_gemm_i8, nq, h_sb, h_lb, h_cap, h_cb, sc_max, o_sll, ld, o_null, st))) {
      return rc;
    }
    HIP_TRY(hipEventRecord(t1.stop, st));
    e->pending.push_back(t1);

    if ((rc = record_start(e, &t2, 2))) return rc;
    HIP_TRY(launch_reduce(ra, st));
    HIP_TRY(hipEventRecord(t2.stop, st));
    e->pending.push_back(t2);

    e->stats.spectra += nq;
    e->stats.sample_evals += nq * e->S;

    if (pipe) {
      HIP_TRY(hipEventRecord(hst.out_ready, st));
      // the previous batch's results, now that this batch is queued behind it
      if (bi > 0 && (rc = host_stage_copy_out(e, res, bi - 1, q0 - QB, QB))) return rc;
    } else if (!out_dev) {
      HIP_TRY(hipMemcpyAsync(res->log_likelihoods_no_dla + q0, o_null, nq * 8, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(res->log_likelihoods_dla + q0, o_dla, nq * 8, hipMemcpyDeviceToHost, st));
      if (res->min_z_dlas) HIP_TRY(hipMemcpyAsync(res->min_z_dlas + q0, o_zmin, nq * 8, hipMemcpyDeviceToHost, st));
      if (res->max_z_dlas) HIP_TRY(hipMemcpyAsync(res->max_z_dlas + q0, o_zmax, nq * 8, hipMemcpyDeviceToHost, st));
      if (res->num_pixels) HIP_TRY(hipMemcpyAsync(res->num_pixels + q0, o_npix, nq * 4, hipMemcpyDeviceToHost, st));
      if (res->sample_log_likelihoods_dla)
        HIP_TRY(hipMemcpy2DAsync(res->sample_log_likelihoods_dla + q0 * res->sample_ld, res->sample_ld * 8,
                                 o_sll, e->S * 8, e->S * 8, nq, hipMemcpyDeviceToHost, st));
      // host results: the workspaces are reused by the next batch, so drain here
      HIP_TRY(hipStreamSynchronize(st));
    } else if (!in_dev) {
      // host inputs were staged in reusable workspaces
      HIP_TRY(hipStreamSynchronize(st));
    }
    // otherwise the next batch reuses the panel workspace in stream order
  }
  if (pipe) {
    const int64_t bl = nbatch - 1;
    const int rc = host_stage_copy_out(e, res, bl, bl * QB, Q - bl * QB);
    if (rc) return rc;
  }
  HIP_TRY(hipEventRecord(e->meta_done, st));
  if (pipe) HIP_TRY(hipStreamSynchronize(e->copy_stream));
  if (!out_dev) return gpdla_engine_synchronize(e);
  return GPDLA_OK;
}

int gpdla_engine_synchronize(gpdla_engine* e) {
  if (!e) return set_error(GPDLA_EINVAL, "null engine");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  int rc = resolve_events(e);
  if (rc) return rc;
  int32_t status = 0;
  HIP_TRY(hipMemcpy(&status, e->d_status, 4, hipMemcpyDeviceToHost));
  if (status) {
    HIP_TRY(hipMemset(e->d_status, 0, 4));
    return set_error(GPDLA_ENUMERIC, "non-positive pivot or non-finite likelihood (outputs NaN)");
  }
  return GPDLA_OK;
}

int gpdla_engine_get_stats_n(gpdla_engine* e, gpdla_stats* s, int64_t stats_bytes) {
  if (!e || !s || stats_bytes < 0) return set_error(GPDLA_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  int rc = resolve_events(e);
  if (rc) return rc;
  std::memcpy(s, &e->stats, std::min<size_t>((size_t)stats_bytes, sizeof(gpdla_stats)));
  return GPDLA_OK;
}

int gpdla_engine_get_stats(gpdla_engine* e, gpdla_stats* s) {
  return gpdla_engine_get_stats_n(e, s, (int64_t)sizeof(gpdla_stats));
}

int gpdla_engine_reset_stats(gpdla_engine* e) {
  if (!e) return set_error(GPDLA_EINVAL, "null engine");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  int rc = resolve_events(e);
  if (rc) return rc;
  e->stats = gpdla_stats{};
  e->mstats = gpdla_multi_stats{};
  e->summary_ms = 0.0;
  e->summary_launches = 0;
  e->population_ms = 0.0;
  e->population_launches = 0;
  e->level_population_ms = 0.0;
  e->level_population_launches = 0;
  e->interval_ms = 0.0;
  e->interval_launches = 0;
  e->cut_ms = 0.0;
  e->cut_launches = 0;
  e->model_spectra_ms = 0.0;
  e->model_spectra_launches = 0;
  e->model_stats = gpdla_model_stats{};
  return GPDLA_OK;
}

// ---------------------------------------------------------------------------------------------
// multi-DLA search (include/gpdla.h "Multi-DLA search"; kernels in multi_dla.hip)
// ---------------------------------------------------------------------------------------------
int gpdla_engine_get_multi_stats(gpdla_engine* e, gpdla_multi_stats* s) {
  if (!e || !s) return set_error(GPDLA_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  int rc = resolve_events(e);
  if (rc) return rc;
  *s = e->mstats;
  return GPDLA_OK;
}

// the samples in the caller's order (the engine keeps them in ascending-offset order, d_perm)
static int multi_caller_samples(gpdla_engine* e) {
  if (e->d_off_c) return GPDLA_OK;
  const size_t S = (size_t)e->S;
  std::vector<double> off(S), nhi(S), off_c(S), nhi_c(S);
  std::vector<int32_t> perm(S);
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(off.data(), e->d_off, S * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(nhi.data(), e->d_nhi, S * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(perm.data(), e->d_perm, S * 4, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < S; ++i) {
    off_c[perm[i]] = off[i];
    nhi_c[perm[i]] = nhi[i];
  }
  size_t dummy = 0;
  int rc;
  if ((rc = grow(&e->d_nhi_c, &dummy, S))) return rc;
  HIP_TRY(hipMemcpy(e->d_nhi_c, nhi_c.data(), S * 8, hipMemcpyHostToDevice));
  dummy = 0;
  if ((rc = grow(&e->d_off_c, &dummy, S))) return rc;
  HIP_TRY(hipMemcpy(e->d_off_c, off_c.data(), S * 8, hipMemcpyHostToDevice));
  e->h_off_c = off_c;
  return GPDLA_OK;
}

// the grid of a summary call: GPDLA_EINVAL unless it is absent (0 x 0) or well formed
static int validate_summary_grid(const gpdla_summary_spec* spec) {
  const int64_t nz = spec->num_z_bins, nn = spec->num_nhi_bins;
  if (nz < 0 || nn < 0 || (nz == 0) != (nn == 0))
    return set_error(GPDLA_EINVAL, "summary grid %lld x %lld: both bin counts must be positive, or both 0", (long long)nz,
                     (long long)nn);
  if (nz * nn > GPDLA_SUMMARY_MAX_BINS)
    return set_error(GPDLA_EINVAL, "summary grid %lld x %lld exceeds %d bins", (long long)nz, (long long)nn,
                     GPDLA_SUMMARY_MAX_BINS);
  if (nz == 0) return GPDLA_OK;
  if (!spec->z_edges || !spec->log_nhi_edges) return set_error(GPDLA_EINVAL, "null summary edge array");
  return validate_grid_edges("", nz, nn, spec->z_edges, spec->log_nhi_edges);
}

// gpdla_engine_process_multi, and with spec / sums gpdla_engine_process_summaries: the summary kernel
// runs per batch after the last level, on the level workspaces the batch leaves on the device
// With sub / rsub (gpdla_engine_process_models) the sub-DLA sweep runs per batch after its level 1: the
// level-1 likelihood launch again with the sub-DLA column densities, into workspaces of its own.
// With pspec / pop (gpdla_engine_process_population) the posterior and split launches of population.hip
// run per batch after the last level, on the batch's evidences and level-1 rows.
// With lv (gpdla_engine_process_levels) the launches of level_population.hip follow them, on every level's
// rows and base indices: the planes when spec has a grid, the posteriors and the split when pspec is given.
// With cuts / cres (gpdla_engine_process_cuts) the search-cut launch runs per batch once its search ranges
// exist and before the first grid reduction, which then all apply the cuts' sample tests.
// One batch's model launch on the panel, padded wavelengths and SpecInfo resident in the engine: the absorbers
// come from the caller (ab) or, in a search call, from the batch's evidences and MAP pairs (sel filled but for its
// outputs, with the call's host levels / log priors).  Ends synchronised: its host staging is reused.
struct ModelBatch {
  int64_t q0, nq, slots;             // first spectrum, spectra, slot capacity of the batch
  const gpdla_model_spectra* res;
  const gpdla_model_absorbers* ab;   // stand-alone entry, or nullptr
  ModelLevelArgs sel;                // search call: rows, levels, ll_dla, map_z, map_n
  const int32_t* h_levels;           // search call: host [Q] given levels, or nullptr (best)
  const double* h_lp;                // search call: host [D][Q] log priors, or nullptr
  int64_t Q;
};

static int model_spectra_batch(gpdla_engine* e, const ModelBatch& b) {
  const gpdla_model_spectra* res = b.res;
  const int64_t q0 = b.q0, nq = b.nq, q1 = q0 + nq;
  const bool out_dev = res->memory == GPDLA_MEM_DEVICE;
  hipStream_t st = e->stream;
  int rc;
  const int D = b.ab ? 0 : b.sel.levels;
  const int64_t c0 = res->cap_offsets[q0], ncap = res->cap_offsets[q1] - c0;
  size_t off = 0;
  auto carve = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
  const size_t o_cnt = carve((size_t)nq * 4), o_z = carve((size_t)nq * kMaxDlas * 8), o_n = carve((size_t)nq * kMaxDlas * 8),
               o_lin = carve((size_t)nq * kMaxDlas * 8), o_cap = carve((size_t)(nq + 1) * 8),
               o_giv = carve((size_t)nq * 4), o_lp = carve((size_t)nq * (D > 0 ? D : 1) * 8);
  const size_t o_out = off;
  const size_t o_pi = carve((size_t)ncap * 4), o_a = carve((size_t)ncap * 8), o_mm = carve((size_t)ncap * 8),
               o_cm = carve((size_t)ncap * 8), o_sd = carve((size_t)ncap * 8), o_chi = carve((size_t)nq * 8),
               o_ll = carve((size_t)nq * 8), o_np = carve((size_t)nq * 4), o_lv = carve((size_t)nq * 4);
  if ((rc = grow(&e->d_ms, &e->cap_ms, off))) return rc;
  if ((rc = grow(&e->d_ms_scratch, &e->cap_ms_scratch, (size_t)(3 * b.slots)))) return rc;
  std::vector<int64_t> h_cap((size_t)nq + 1);
  for (int64_t q = 0; q <= nq; ++q) h_cap[q] = res->cap_offsets[q0 + q] - c0;
  HIP_TRY(hipMemcpyAsync(e->d_ms + o_cap, h_cap.data(), (size_t)(nq + 1) * 8, hipMemcpyHostToDevice, st));
  // host results: the slots a spectrum does not fill come back as NaN / -1
  if (!out_dev) HIP_TRY(hipMemsetAsync(e->d_ms + o_out, 0xFF, off - o_out, st));
  bool lin = false;
  if (b.ab) {
    HIP_TRY(hipMemcpyAsync(e->d_ms + o_cnt, b.ab->counts + q0, (size_t)nq * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(e->d_ms + o_z, b.ab->z_dlas + q0 * kMaxDlas, (size_t)nq * kMaxDlas * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(e->d_ms + o_n, b.ab->log_nhis + q0 * kMaxDlas, (size_t)nq * kMaxDlas * 8, hipMemcpyHostToDevice, st));
    if ((lin = b.ab->nhis != nullptr))
      HIP_TRY(hipMemcpyAsync(e->d_ms + o_lin, b.ab->nhis + q0 * kMaxDlas, (size_t)nq * kMaxDlas * 8, hipMemcpyHostToDevice, st));
  } else {
    ModelLevelArgs sel = b.sel;
    if (b.h_levels) {
      HIP_TRY(hipMemcpyAsync(e->d_ms + o_giv, b.h_levels + q0, (size_t)nq * 4, hipMemcpyHostToDevice, st));
      sel.given = (const int32_t*)(e->d_ms + o_giv);
    }
    if (b.h_lp) {
      for (int d = 0; d < D; ++d)
        HIP_TRY(hipMemcpyAsync(e->d_ms + o_lp + (size_t)d * nq * 8, b.h_lp + (int64_t)d * b.Q + q0, (size_t)nq * 8,
                               hipMemcpyHostToDevice, st));
      sel.lp_dla = (const double*)(e->d_ms + o_lp);
    }
    sel.counts = (int32_t*)(e->d_ms + o_cnt); sel.z_dlas = (double*)(e->d_ms + o_z); sel.log_nhis = (double*)(e->d_ms + o_n);
    sel.level_out = out_dev ? (res->levels ? res->levels + q0 : nullptr) : (int32_t*)(e->d_ms + o_lv);
    HIP_TRY(launch_model_levels(sel, st));
  }

  ModelSpectraArgs ma{};
  ma.q_count = (int32_t)nq; ma.info = e->d_info; ma.panel = e->d_panel; ma.lam_pad = e->d_lam; ma.slot_pixel = e->d_smap;
  ma.num_lines = e->params.num_lines; ma.lines = make_line_args(e->d_lines);
  ma.counts = (const int32_t*)(e->d_ms + o_cnt); ma.z_dlas = (const double*)(e->d_ms + o_z);
  ma.log_nhis = (const double*)(e->d_ms + o_n); ma.nhis = lin ? (const double*)(e->d_ms + o_lin) : nullptr;
  ma.cap_offsets = (const int64_t*)(e->d_ms + o_cap);
  ma.scratch = e->d_ms_scratch; ma.scratch_plane = b.slots;
  if (out_dev) {
    ma.pixel_inds = res->pixel_inds + c0; ma.absorption = res->absorption + c0; ma.model_mean = res->model_mean + c0;
    ma.continuum_mean = res->continuum_mean + c0; ma.continuum_sd = res->continuum_sd + c0;
    ma.chi2 = res->chi2 + q0; ma.log_likelihood = res->log_likelihoods + q0; ma.num_pixels = res->num_pixels + q0;
  } else {
    ma.pixel_inds = (int32_t*)(e->d_ms + o_pi); ma.absorption = (double*)(e->d_ms + o_a);
    ma.model_mean = (double*)(e->d_ms + o_mm); ma.continuum_mean = (double*)(e->d_ms + o_cm);
    ma.continuum_sd = (double*)(e->d_ms + o_sd); ma.chi2 = (double*)(e->d_ms + o_chi);
    ma.log_likelihood = (double*)(e->d_ms + o_ll); ma.num_pixels = (int32_t*)(e->d_ms + o_np);
  }
  ma.status = e->d_ms_status;
  TimedLaunch t15{};
  if ((rc = record_start(e, &t15, 15))) return rc;
  HIP_TRY(launch_model_spectra(e->K, ma, st));
  HIP_TRY(hipEventRecord(t15.stop, st));
  e->pending.push_back(t15);
  if (!out_dev) {
    const hipMemcpyKind k = hipMemcpyDeviceToHost;
    if (ncap) {
      HIP_TRY(hipMemcpyAsync(res->pixel_inds + c0, e->d_ms + o_pi, (size_t)ncap * 4, k, st));
      HIP_TRY(hipMemcpyAsync(res->absorption + c0, e->d_ms + o_a, (size_t)ncap * 8, k, st));
      HIP_TRY(hipMemcpyAsync(res->model_mean + c0, e->d_ms + o_mm, (size_t)ncap * 8, k, st));
      HIP_TRY(hipMemcpyAsync(res->continuum_mean + c0, e->d_ms + o_cm, (size_t)ncap * 8, k, st));
      HIP_TRY(hipMemcpyAsync(res->continuum_sd + c0, e->d_ms + o_sd, (size_t)ncap * 8, k, st));
    }
    HIP_TRY(hipMemcpyAsync(res->chi2 + q0, e->d_ms + o_chi, (size_t)nq * 8, k, st));
    HIP_TRY(hipMemcpyAsync(res->log_likelihoods + q0, e->d_ms + o_ll, (size_t)nq * 8, k, st));
    HIP_TRY(hipMemcpyAsync(res->num_pixels + q0, e->d_ms + o_np, (size_t)nq * 4, k, st));
    if (!b.ab && res->levels) HIP_TRY(hipMemcpyAsync(res->levels + q0, e->d_ms + o_lv, (size_t)nq * 4, k, st));
  }
  HIP_TRY(hipStreamSynchronize(st));   // the staging vector and the block are reused by the next batch
  return GPDLA_OK;
}

// the call's status word after its last batch: GPDLA_EINVAL naming a spectrum over its capacity, GPDLA_ENUMERIC
static int model_spectra_finish(gpdla_engine* e, int64_t Q, const gpdla_model_spectra* res) {
  int32_t status = 0;
  HIP_TRY(hipMemcpy(&status, e->d_ms_status, 4, hipMemcpyDeviceToHost));
  if (status) HIP_TRY(hipMemset(e->d_ms_status, 0, 4));
  if (status & 2) {
    const bool out_dev = res->memory == GPDLA_MEM_DEVICE;
    std::vector<int32_t> np((size_t)Q);
    if (out_dev) HIP_TRY(hipMemcpy(np.data(), res->num_pixels, (size_t)Q * 4, hipMemcpyDeviceToHost));
    int64_t over_q = -1;
    for (int64_t q = 0; q < Q && over_q < 0; ++q)
      if ((out_dev ? np[q] : res->num_pixels[q]) > res->cap_offsets[q + 1] - res->cap_offsets[q]) over_q = q;
    return set_error(GPDLA_EINVAL, "model spectra: spectrum %lld has more likelihood pixels than its capacity %lld (nothing written for it)",
                     (long long)over_q, (long long)(over_q >= 0 ? res->cap_offsets[over_q + 1] - res->cap_offsets[over_q] : -1));
  }
  if (status & 1) return set_error(GPDLA_ENUMERIC, "model spectra: non-positive pivot (outputs NaN)");
  return GPDLA_OK;
}

// the arrays of a gpdla_model_spectra and its capacity offsets over Q spectra
static int model_spectra_check_results(const gpdla_model_spectra* res, int64_t Q) {
  if (res->memory != GPDLA_MEM_HOST && res->memory != GPDLA_MEM_DEVICE)
    return set_error(GPDLA_EINVAL, "model spectra: results memory=%d", res->memory);
  if (!res->cap_offsets || !res->pixel_inds || !res->absorption || !res->model_mean || !res->continuum_mean ||
      !res->continuum_sd || !res->chi2 || !res->log_likelihoods || !res->num_pixels)
    return set_error(GPDLA_EINVAL, "model spectra: null result array");
  if (res->cap_offsets[0] < 0) return set_error(GPDLA_EINVAL, "model spectra: cap_offsets[0] < 0");
  for (int64_t q = 0; q < Q; ++q)
    if (res->cap_offsets[q + 1] < res->cap_offsets[q])
      return set_error(GPDLA_EINVAL, "model spectra: cap_offsets not monotone at %lld", (long long)q);
  return GPDLA_OK;
}


static int process_multi_impl(gpdla_engine* e, const gpdla_spectra* sp, const gpdla_multi_dla* mu,
                              const gpdla_results_multi* res, const gpdla_summary_spec* spec,
                              const gpdla_summaries* sums, const gpdla_sub_dla* sub = nullptr,
                              const gpdla_results_sub* rsub = nullptr, const gpdla_population_spec* pspec = nullptr,
                              const gpdla_population* pop = nullptr, const gpdla_level_population* lv = nullptr,
                              const gpdla_interval_spec* ispec = nullptr, const gpdla_intervals* iv = nullptr,
                              const gpdla_search_cuts* cuts = nullptr, const gpdla_search_cut_results* cres = nullptr,
                              const gpdla_model_levels* mlev = nullptr, const gpdla_model_spectra* mres = nullptr) {
  if (!e || !sp || !mu || !res) return set_error(GPDLA_EINVAL, "null argument");
  if (cuts) {   // (gpdla_engine_process_cuts: cres is set)
    if (!cres->z_uppers || !cres->pixel_counts || !cres->bitmap_offsets || !cres->bitmap_words)
      return set_error(GPDLA_EINVAL, "search cuts: null result array");
    if (cres->memory != GPDLA_MEM_HOST && cres->memory != GPDLA_MEM_DEVICE)
      return set_error(GPDLA_EINVAL, "search cuts: results memory=%d", cres->memory);
    int rcc = validate_search_cuts(cuts, cres->path_summary, cres->path_population);
    if (rcc) return rcc;
    if (!(spec && spec->num_z_bins > 0) && !pspec)
      return set_error(GPDLA_EINVAL, "search cuts: no summary or population grid to cut");
    if (sub) return set_error(GPDLA_EUNSUPPORTED, "search cuts: the sub-DLA model is not covered");
    if (e->gemm || e->i8)
      return set_error(GPDLA_EUNSUPPORTED, "the search cuts need the fused fp64 path (this engine runs a panel-GEMM or int8 path)");
  }
  if (ispec) {   // (gpdla_engine_process_intervals: iv is set)
    if (!ispec->log_nhi_samples) return set_error(GPDLA_EINVAL, "null interval log_nhi_samples");
    if (!iv->z_means || !iv->z_sds || !iv->log_nhi_means || !iv->log_nhi_sds || !iv->z_lr_ranges || !iv->log_nhi_lr_ranges ||
        !iv->z_quantiles || !iv->log_nhi_quantiles || !iv->lr_counts)
      return set_error(GPDLA_EINVAL, "null interval array");
    if (iv->memory != GPDLA_MEM_HOST && iv->memory != GPDLA_MEM_DEVICE)
      return set_error(GPDLA_EINVAL, "intervals memory=%d", iv->memory);
    int rci = validate_interval_levels(ispec->lr_delta, ispec->num_levels, ispec->levels, e->S);
    if (rci) return rci;
  }
  // a half is asked for by its arrays: the planes by bin_planes, the posteriors and the split by the rest
  const bool lv_planes = lv && lv->bin_planes;
  const bool lv_split = lv && (lv->level_posteriors || lv->poisson_plane || lv->large_inds || lv->large_probs || lv->large_bins);
  if (lv) {
    if (!lv_planes && !lv_split) return set_error(GPDLA_EINVAL, "level population without an output array");
    if (lv->memory != GPDLA_MEM_HOST && lv->memory != GPDLA_MEM_DEVICE)
      return set_error(GPDLA_EINVAL, "level population memory=%d", lv->memory);
    if (lv_planes && !(spec && spec->num_z_bins > 0)) return set_error(GPDLA_EINVAL, "level bin_planes need a summary grid");
    if (lv_split && !pspec) return set_error(GPDLA_EINVAL, "the level population arrays need a population spec");
    if (lv_split && (!lv->level_posteriors || !lv->poisson_plane || !lv->large_inds || !lv->large_probs || !lv->large_bins))
      return set_error(GPDLA_EINVAL, "null level population array");
    if (e->gemm || e->i8)
      return set_error(GPDLA_EUNSUPPORTED, "the level population needs the fused fp64 path (this engine runs a panel-GEMM or int8 path)");
  }
  if (pspec) {
    if (!pop) return set_error(GPDLA_EINVAL, "null argument");
    int rcp = validate_population_grid(pspec->num_z_bins, pspec->num_nhi_bins, pspec->z_edges, pspec->log_nhi_edges,
                                       pspec->p_thresh_sample, pspec->p_switch);
    if (rcp) return rcp;
    if (!pspec->log_nhi_samples) return set_error(GPDLA_EINVAL, "null population log_nhi_samples");
    if (!pspec->log_priors_no_dla || !pspec->log_priors_dla || (sub && !pspec->log_priors_lls))
      return set_error(GPDLA_EINVAL, "null population prior array");
    if (!pop->poisson_plane || !pop->large_inds || !pop->large_probs || !pop->large_bins || !pop->p_dlas)
      return set_error(GPDLA_EINVAL, "null population array");
    if (pop->memory != GPDLA_MEM_HOST && pop->memory != GPDLA_MEM_DEVICE)
      return set_error(GPDLA_EINVAL, "population memory=%d", pop->memory);
  }
  bool sub_map = false;
  if (sub) {
    if (!rsub || !rsub->log_likelihoods_lls) return set_error(GPDLA_EINVAL, "null sub-DLA result array");
    if (rsub->memory != GPDLA_MEM_HOST && rsub->memory != GPDLA_MEM_DEVICE)
      return set_error(GPDLA_EINVAL, "results_sub memory=%d", rsub->memory);
    if (!sub->nhi_samples) return set_error(GPDLA_EINVAL, "null sub-DLA nhi_samples");
    for (int64_t i = 0; i < e->S; ++i)
      if (!(sub->nhi_samples[i] > 0.0 && sub->nhi_samples[i] < INFINITY))
        return set_error(GPDLA_EINVAL, "sub-DLA nhi_samples[%lld] = %g: column densities must be finite and > 0",
                         (long long)i, sub->nhi_samples[i]);
    if (rsub->sample_log_likelihoods_lls && rsub->sample_ld < e->S)
      return set_error(GPDLA_EINVAL, "sub-DLA sample_ld (%lld) < num_samples (%lld)", (long long)rsub->sample_ld,
                       (long long)e->S);
    if (e->gemm || e->i8)
      return set_error(GPDLA_EUNSUPPORTED, "the sub-DLA model needs the fused fp64 path (this engine runs a panel-GEMM or int8 path)");
    sub_map = spec && (rsub->map_sample_inds || rsub->map_log_likelihoods || rsub->map_z_lls || rsub->map_log_nhi_lls);
    if (sub_map && !rsub->log_nhi_samples) return set_error(GPDLA_EINVAL, "sub-DLA MAP outputs need log_nhi_samples");
  }
  if (spec) {
    if (!sums) return set_error(GPDLA_EINVAL, "null argument");
    int rcv = validate_summary_grid(spec);
    if (rcv) return rcv;
    if (!spec->log_nhi_samples) return set_error(GPDLA_EINVAL, "null log_nhi_samples");
    if (!sums->map_sample_inds || !sums->map_log_likelihoods || !sums->map_z_dlas || !sums->map_log_nhis)
      return set_error(GPDLA_EINVAL, "null summary array");
    if (spec->num_z_bins > 0 && !sums->bin_planes) return set_error(GPDLA_EINVAL, "null bin_planes with a grid");
    if (sums->memory != GPDLA_MEM_HOST && sums->memory != GPDLA_MEM_DEVICE)
      return set_error(GPDLA_EINVAL, "summaries memory=%d", sums->memory);
  }
  const int D = mu->max_dlas;
  if (D < 1 || D > GPDLA_MAX_DLAS) return set_error(GPDLA_EINVAL, "max_dlas=%d outside 1..%d", D, GPDLA_MAX_DLAS);
  if (D > 1 && (e->gemm || e->i8))
    return set_error(GPDLA_EUNSUPPORTED, "max_dlas=%d needs the fused fp64 path (this engine runs a panel-GEMM or int8 path)", D);
  if (D > 1 && (e->params.num_lines != 3 || !multi_level_supported(e->K)))
    return set_error(GPDLA_EUNSUPPORTED, "max_dlas=%d needs num_lines=3 (num_lines=%d)", D, e->params.num_lines);
  const int64_t Q = sp->num_spectra, S = e->S;
  if (Q < 0) return set_error(GPDLA_EINVAL, "num_spectra < 0");
  if (D > 1 && !(mu->min_z_separation >= 0.0) ) return set_error(GPDLA_EINVAL, "min_z_separation must be >= 0");
  if (D > 1 && !std::isfinite(mu->occam_log_penalty)) return set_error(GPDLA_EINVAL, "occam_log_penalty not finite");
  if (D > 1 && !mu->resample_uniforms && !mu->forced_base_inds)
    return set_error(GPDLA_EINVAL, "max_dlas=%d needs resample_uniforms or forced_base_inds", D);
  if (D > 1 && mu->resample_uniforms)
    for (int64_t i = 0; i < (D - 1) * S; ++i)
      if (!(mu->resample_uniforms[i] >= 0.0 && mu->resample_uniforms[i] < 1.0))
        return set_error(GPDLA_EINVAL, "resample_uniforms[%lld] = %g outside [0, 1)", (long long)i, mu->resample_uniforms[i]);
  if (D > 1 && mu->forced_base_inds)
    for (int64_t i = 0; i < (D - 1) * Q * S; ++i)
      if (mu->forced_base_inds[i] < -1 || mu->forced_base_inds[i] >= S)
        return set_error(GPDLA_EINVAL, "forced_base_inds[%lld] = %d outside -1..%lld", (long long)i,
                         (int)mu->forced_base_inds[i], (long long)(S - 1));
  if (Q == 0) return GPDLA_OK;
  if (!sp->offsets || !sp->z_qsos) return set_error(GPDLA_EINVAL, "null spectra array");
  if (!res->log_likelihoods_no_dla || !res->log_likelihoods_dla) return set_error(GPDLA_EINVAL, "null result array");
  if ((res->sample_log_likelihoods_dla || res->base_sample_inds) && res->sample_ld < S)
    return set_error(GPDLA_EINVAL, "sample_ld (%lld) < num_samples (%lld)", (long long)res->sample_ld, (long long)S);
  HIP_TRY(hipSetDevice(e->device));
  int rc;
  if ((D > 1 || spec || pspec || ispec) && (rc = multi_caller_samples(e))) return rc;
  hipStream_t st = e->stream;
  if (sub) {  // the column densities in the sweep's (ascending-offset) order, as the engine's own are kept
    const size_t Ss = (size_t)S;
    std::vector<double> sorted(Ss);
    for (size_t i = 0; i < Ss; ++i) sorted[i] = sub->nhi_samples[e->h_perm[i]];
    if ((rc = grow(&e->d_sub_nhi, &e->cap_sub_nhi, Ss))) return rc;
    // (pageable host memory: the copy has left `sorted` when the call returns)
    HIP_TRY(hipMemcpyAsync(e->d_sub_nhi, sorted.data(), Ss * 8, hipMemcpyHostToDevice, st));
    if (sub_map) {
      if ((rc = grow(&e->d_sub_nhi_c, &e->cap_sub_nhi_c, Ss))) return rc;
      if ((rc = grow(&e->d_sub_lognhi, &e->cap_sub_lognhi, Ss))) return rc;
      HIP_TRY(hipMemcpyAsync(e->d_sub_nhi_c, sub->nhi_samples, Ss * 8, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(e->d_sub_lognhi, rsub->log_nhi_samples, Ss * 8, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
  }
  const int nzb = spec ? spec->num_z_bins : 0, nnb = spec ? spec->num_nhi_bins : 0;
  const size_t nbins = (size_t)nzb * nnb;
  if (spec) {
    if ((rc = grow(&e->d_s_lognhi, &e->cap_s_lognhi, (size_t)S))) return rc;
    HIP_TRY(hipMemcpyAsync(e->d_s_lognhi, spec->log_nhi_samples, (size_t)S * 8, hipMemcpyHostToDevice, st));
    if (nbins) {
      if ((rc = grow(&e->d_s_edges, &e->cap_s_edges, (size_t)(nzb + nnb + 2)))) return rc;
      HIP_TRY(hipMemcpyAsync(e->d_s_edges, spec->z_edges, (size_t)(nzb + 1) * 8, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(e->d_s_edges + nzb + 1, spec->log_nhi_edges, (size_t)(nnb + 1) * 8, hipMemcpyHostToDevice, st));
    }
  }
  if (ispec) {   // the rank tables of the call's samples: [offset | log N_HI]
    const size_t Ss = (size_t)S;
    std::vector<int32_t> rank(2 * Ss);
    std::vector<double> uniq(2 * Ss);
    build_rank_table(e->h_off_c.data(), S, rank.data(), uniq.data());
    build_rank_table(ispec->log_nhi_samples, S, rank.data() + Ss, uniq.data() + Ss);
    if ((rc = grow(&e->d_i_lognhi, &e->cap_i_lognhi, Ss))) return rc;
    if ((rc = grow(&e->d_i_rank, &e->cap_i_rank, 2 * Ss))) return rc;
    if ((rc = grow(&e->d_i_uniq, &e->cap_i_uniq, 2 * Ss))) return rc;
    HIP_TRY(hipMemcpyAsync(e->d_i_lognhi, ispec->log_nhi_samples, Ss * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(e->d_i_rank, rank.data(), 2 * Ss * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(e->d_i_uniq, uniq.data(), 2 * Ss * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));   // pageable host memory: the copies have left the vectors
  }
  const int pnz = pspec ? pspec->num_z_bins : 0, pnn = pspec ? pspec->num_nhi_bins : 0;
  const size_t pbins = (size_t)pnz * pnn;
  if (pspec) {
    const size_t Qs = (size_t)Q;
    if ((rc = grow(&e->d_p_lognhi, &e->cap_p_lognhi, (size_t)S))) return rc;
    if ((rc = grow(&e->d_p_edges, &e->cap_p_edges, (size_t)(pnz + pnn + 2)))) return rc;
    if ((rc = grow(&e->d_p_lpno, &e->cap_p_lpno, Qs))) return rc;
    if ((rc = grow(&e->d_p_lpdla, &e->cap_p_lpdla, Qs * D))) return rc;
    HIP_TRY(hipMemcpyAsync(e->d_p_lognhi, pspec->log_nhi_samples, (size_t)S * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(e->d_p_edges, pspec->z_edges, (size_t)(pnz + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(e->d_p_edges + pnz + 1, pspec->log_nhi_edges, (size_t)(pnn + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(e->d_p_lpno, pspec->log_priors_no_dla, Qs * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(e->d_p_lpdla, pspec->log_priors_dla, Qs * D * 8, hipMemcpyHostToDevice, st));
    if (sub) {
      if ((rc = grow(&e->d_p_lplls, &e->cap_p_lplls, Qs))) return rc;
      HIP_TRY(hipMemcpyAsync(e->d_p_lplls, pspec->log_priors_lls, Qs * 8, hipMemcpyHostToDevice, st));
    }
  }
  // search cuts: the bitmap's word offsets over the whole call, and the edges of the path grids
  std::vector<int64_t> cut_woff;
  const int cnz[2] = {cuts ? cuts->num_z_bins_summary : 0, cuts ? cuts->num_z_bins_population : 0};
  if (cuts) {
    cut_woff.assign((size_t)Q + 1, 0);
    for (int64_t q = 0; q < Q; ++q) {
      const int64_t len = sp->offsets[q + 1] - sp->offsets[q];
      if (len < 0 || len > INT32_MAX - 64) return set_error(GPDLA_EINVAL, "offsets not monotone at %lld", (long long)q);
      cut_woff[q + 1] = cut_woff[q] + (len + 31) / 32;
    }
    if (cres->memory == GPDLA_MEM_DEVICE)
      HIP_TRY(hipMemcpyAsync(cres->bitmap_offsets, cut_woff.data(), (size_t)(Q + 1) * 8, hipMemcpyHostToDevice, st));
    else
      std::memcpy(cres->bitmap_offsets, cut_woff.data(), (size_t)(Q + 1) * 8);
    // the call-wide offsets go to the device once; cut_woff is not written again before the call's last sync
    if ((rc = grow(&e->d_c_wo, &e->cap_c_wo, (size_t)Q + 1))) return rc;
    HIP_TRY(hipMemcpyAsync(e->d_c_wo, cut_woff.data(), (size_t)(Q + 1) * 8, hipMemcpyHostToDevice, st));
    if (cnz[0] + cnz[1] > 0) {
      if ((rc = grow(&e->d_c_edges, &e->cap_c_edges, (size_t)(cnz[0] + cnz[1] + 2)))) return rc;
      if (cnz[0]) HIP_TRY(hipMemcpyAsync(e->d_c_edges, cuts->z_edges_summary, (size_t)(cnz[0] + 1) * 8, hipMemcpyHostToDevice, st));
      if (cnz[1])
        HIP_TRY(hipMemcpyAsync(e->d_c_edges + cnz[0] + 1, cuts->z_edges_population, (size_t)(cnz[1] + 1) * 8,
                               hipMemcpyHostToDevice, st));
    }
  }
  const bool out_dev = res->memory == GPDLA_MEM_DEVICE;
  const hipMemcpyKind out_kind = out_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const bool forced = D > 1 && mu->forced_base_inds;
  // the batch of gpdla_engine_process: one call of it below is exactly one of its device batches,
  // whose panel, padded wavelengths and spectrum infos then stay in the engine for the deeper levels
  const int64_t QB = e->params.max_batch_spectra > 0 ? e->params.max_batch_spectra : (e->gemm ? 64 : 1024);
  if (D > 1 && mu->resample_uniforms) {
    if ((rc = grow(&e->d_m_u, &e->cap_m_u, (size_t)((D - 1) * S)))) return rc;
    HIP_TRY(hipMemcpyAsync(e->d_m_u, mu->resample_uniforms, (size_t)(D - 1) * S * 8, hipMemcpyHostToDevice, st));
  }
  for (int64_t q0 = 0; q0 < Q; q0 += QB) {
    const int64_t nq = std::min(QB, Q - q0);
    const size_t plane = (size_t)nq * S;
    if ((rc = grow(&e->d_m_sll, &e->cap_m_sll, plane * D))) return rc;
    if ((rc = grow(&e->d_m_lldla, &e->cap_m_lldla, (size_t)nq * D))) return rc;
    if ((rc = grow(&e->d_m_null, &e->cap_m_q[0], (size_t)nq))) return rc;
    if ((rc = grow(&e->d_m_zmin, &e->cap_m_q[1], (size_t)nq))) return rc;
    if ((rc = grow(&e->d_m_zmax, &e->cap_m_q[2], (size_t)nq))) return rc;
    if ((rc = grow(&e->d_m_npix, &e->cap_m_q[3], (size_t)nq))) return rc;
    if (D > 1) {
      if ((rc = grow(&e->d_m_base, &e->cap_m_base, plane * (D - 1)))) return rc;
      for (int i = 0; i < 2; ++i)
        if ((rc = grow(&e->d_m_chain[i], &e->cap_m_chain[i], plane * kMaxChain))) return rc;
      if (S > GPDLA_RESAMPLE_LDS && !forced && (rc = grow(&e->d_m_cws, &e->cap_m_cws, plane))) return rc;
      if (forced) {
        if ((rc = grow(&e->d_m_forced, &e->cap_m_forced, plane * (D - 1)))) return rc;
        for (int d = 2; d <= D; ++d)
          HIP_TRY(hipMemcpyAsync(e->d_m_forced + (size_t)(d - 2) * plane,
                                 mu->forced_base_inds + ((int64_t)(d - 2) * Q + q0) * S, plane * 4,
                                 hipMemcpyHostToDevice, st));
      }
    }
    // level 1: the single-DLA engine itself, into the level workspaces
    gpdla_spectra bsp = *sp;
    bsp.num_spectra = nq;
    bsp.offsets = sp->offsets + q0;
    bsp.z_qsos = sp->z_qsos + q0;
    gpdla_results r1{};
    r1.memory = GPDLA_MEM_DEVICE;
    r1.log_likelihoods_no_dla = e->d_m_null;
    r1.sample_log_likelihoods_dla = e->d_m_sll;
    r1.sample_ld = S;
    r1.log_likelihoods_dla = e->d_m_lldla;
    r1.min_z_dlas = e->d_m_zmin; r1.max_z_dlas = e->d_m_zmax; r1.num_pixels = e->d_m_npix;
    const size_t p0 = e->pending.size();
    if ((rc = gpdla_engine_process(e, &bsp, &r1)) < 0) return rc;
    for (size_t i = p0; i < e->pending.size(); ++i)
      if (e->pending[i].kind == 1) e->pending[i].level = 1;

    if (sub) {
      // the sub-DLA sweep on the batch's resident panel: likelihood_kernel with the sub-DLA column
      // densities; its null lane goes to a workspace nobody reads, and nothing is added to gpdla_stats
      if ((rc = grow(&e->d_sub_sll, &e->cap_sub_sll, plane))) return rc;
      if ((rc = grow(&e->d_sub_ev, &e->cap_sub_ev, (size_t)nq))) return rc;
      if ((rc = grow(&e->d_sub_null, &e->cap_sub_null, (size_t)nq))) return rc;
      LikelihoodArgs la{};
      la.q_count = (int32_t)nq; la.info = e->d_info; la.panel = e->d_panel; la.lam_pad = e->d_lam;
      la.offsets = e->d_off; la.nhi = e->d_sub_nhi; la.perm = e->d_perm; la.S = S;
      la.num_lines = e->params.num_lines; la.lines = make_line_args(e->d_lines);
      la.sample_ll = e->d_sub_sll; la.ld = S; la.ll_null = e->d_sub_null; la.status = e->d_status;
      TimedLaunch t9{}, t10{};
      if ((rc = record_start(e, &t9, 9))) return rc;
      HIP_TRY(launch_likelihood(e->K, la, st));
      HIP_TRY(hipEventRecord(t9.stop, st));
      e->pending.push_back(t9);
      ReduceArgs ra{};
      ra.q_count = (int32_t)nq; ra.info = e->d_info; ra.sample_ll = e->d_sub_sll; ra.ld = S; ra.S = S;
      ra.ll_dla = e->d_sub_ev;
      if ((rc = record_start(e, &t10, 10))) return rc;
      HIP_TRY(launch_reduce(ra, st));
      if (sub_map) {
        if ((rc = grow(&e->d_sub_mind, &e->cap_sub_mind, (size_t)nq))) return rc;
        if ((rc = grow(&e->d_sub_mll, &e->cap_sub_mll, (size_t)nq))) return rc;
        if ((rc = grow(&e->d_sub_mz, &e->cap_sub_mz, (size_t)nq * kMaxDlas))) return rc;
        if ((rc = grow(&e->d_sub_mn, &e->cap_sub_mn, (size_t)nq * kMaxDlas))) return rc;
        SummaryArgs sa{};
        sa.r.rows = (int32_t)nq; sa.r.levels = 1; sa.r.ll = e->d_sub_sll; sa.r.ld = S; sa.r.S = S;
        sa.r.base = nullptr; sa.r.ld_base = S;
        sa.r.offset = e->d_off_c; sa.r.log_nhi = e->d_sub_lognhi; sa.nhi = e->d_sub_nhi_c;
        sa.r.zmin = e->d_m_zmin; sa.r.zmax = e->d_m_zmax;
        sa.map_ind = e->d_sub_mind; sa.map_ll = e->d_sub_mll; sa.map_z = e->d_sub_mz; sa.map_n = e->d_sub_mn;
        HIP_TRY(launch_posterior_summary(sa, st));
      }
      HIP_TRY(hipEventRecord(t10.stop, st));
      e->pending.push_back(t10);
      const hipMemcpyKind sk = rsub->memory == GPDLA_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
      HIP_TRY(hipMemcpyAsync(rsub->log_likelihoods_lls + q0, e->d_sub_ev, nq * 8, sk, st));
      if (rsub->sample_log_likelihoods_lls)
        HIP_TRY(hipMemcpy2DAsync(rsub->sample_log_likelihoods_lls + q0 * rsub->sample_ld, rsub->sample_ld * 8,
                                 e->d_sub_sll, S * 8, S * 8, nq, sk, st));
      if (sub_map) {
        if (rsub->map_sample_inds) HIP_TRY(hipMemcpyAsync(rsub->map_sample_inds + q0, e->d_sub_mind, nq * 4, sk, st));
        if (rsub->map_log_likelihoods) HIP_TRY(hipMemcpyAsync(rsub->map_log_likelihoods + q0, e->d_sub_mll, nq * 8, sk, st));
        // the first of each row's kMaxDlas pairs (levels = 1)
        if (rsub->map_z_lls)
          HIP_TRY(hipMemcpy2DAsync(rsub->map_z_lls + q0, 8, e->d_sub_mz, kMaxDlas * 8, 8, nq, sk, st));
        if (rsub->map_log_nhi_lls)
          HIP_TRY(hipMemcpy2DAsync(rsub->map_log_nhi_lls + q0, 8, e->d_sub_mn, kMaxDlas * 8, 8, nq, sk, st));
      }
    }

    for (int d = 2; d <= D; ++d) {
      int32_t* chain_prev = e->d_m_chain[d & 1];        // built at level d - 1 (unused at d = 2)
      int32_t* chain_next = e->d_m_chain[(d + 1) & 1];
      ResampleArgs ra{};
      ra.rows = (int32_t)nq; ra.ll = e->d_m_sll + (size_t)(d - 2) * plane; ra.ld = S; ra.S = S;
      ra.u = forced ? nullptr : e->d_m_u + (size_t)(d - 2) * S;
      ra.forced = forced ? e->d_m_forced + (size_t)(d - 2) * plane : nullptr;
      ra.cws = e->d_m_cws;
      ra.chain_prev = chain_prev; ra.prev_len = d - 2; ra.chain_next = chain_next;
      ra.base_inds = e->d_m_base + (size_t)(d - 2) * plane;
      TimedLaunch t4{}, t5{}, t6{};
      if ((rc = record_start(e, &t4, 4))) return rc;
      HIP_TRY(launch_resample(ra, st));
      HIP_TRY(hipEventRecord(t4.stop, st));
      e->pending.push_back(t4);

      MultiLevelArgs la{};
      la.q_count = (int32_t)nq; la.info = e->d_info; la.panel = e->d_panel; la.lam_pad = e->d_lam;
      la.offsets = e->d_off; la.nhi = e->d_nhi; la.perm = e->d_perm;
      la.offsets_c = e->d_off_c; la.nhi_c = e->d_nhi_c;
      la.chain = chain_next; la.chain_len = d - 1; la.S = S;
      la.lines = make_line_args(e->d_lines);
      la.min_z_separation = mu->min_z_separation;
      la.sample_ll = e->d_m_sll + (size_t)(d - 1) * plane; la.ld = S; la.status = e->d_status;
      if ((rc = record_start(e, &t5, 5))) return rc;
      t5.level = d;
      HIP_TRY(launch_multi_level(e->K, la, st));
      HIP_TRY(hipEventRecord(t5.stop, st));
      e->pending.push_back(t5);

      MultiReduceArgs ma{};
      ma.q_count = (int32_t)nq; ma.sample_ll = la.sample_ll; ma.ld = S; ma.S = S;
      ma.penalty = (d - 1) * mu->occam_log_penalty;
      ma.ll_dla = e->d_m_lldla + (size_t)(d - 1) * nq;
      if ((rc = record_start(e, &t6, 6))) return rc;
      HIP_TRY(launch_multi_reduce(ma, st));
      HIP_TRY(hipEventRecord(t6.stop, st));
      e->pending.push_back(t6);
    }

    // the batch's rows as the summary and population launches read them, on the grid of each
    SampleRowsArgs rows_b{};
    rows_b.rows = (int32_t)nq; rows_b.levels = D; rows_b.ll = e->d_m_sll; rows_b.ld = S; rows_b.S = S;
    rows_b.base = D > 1 ? e->d_m_base : nullptr; rows_b.ld_base = S;
    rows_b.offset = e->d_off_c; rows_b.zmin = e->d_m_zmin; rows_b.zmax = e->d_m_zmax;
    if (cuts) {
      // the cut launch on the batch's resident pixels (the copies gpdla_engine_process made, or the caller's
      // device arrays) and search ranges; the reductions below read its upper ends and bitmap
      const int64_t nwb = cut_woff[q0 + nq] - cut_woff[q0];
      if ((rc = grow(&e->d_c_zu, &e->cap_c_zu, (size_t)nq))) return rc;
      if ((rc = grow(&e->d_c_np, &e->cap_c_np, (size_t)nq))) return rc;
      if ((rc = grow(&e->d_c_words, &e->cap_c_words, (size_t)std::max<int64_t>(nwb, 1)))) return rc;
      for (int g = 0; g < 2; ++g)
        if (cnz[g] && (rc = grow(&e->d_c_path[g], &e->cap_c_path[g], (size_t)nq * (cnz[g] + 1)))) return rc;
      // the batch's rows index the call-wide offsets from q0; the words pointer is moved back by the batch's
      // first word, so offset[q0 + i] lands inside d_c_words
      const int64_t* batch_wo = e->d_c_wo + q0;
      uint32_t* batch_words = e->d_c_words - cut_woff[q0];
      const bool in_dev = sp->memory == GPDLA_MEM_DEVICE;
      SearchCutArgs ca{};
      ca.offsets = e->d_meta;   // the batch's pixel offsets, relative to its first pixel
      ca.wavelengths = in_dev ? sp->wavelengths + sp->offsets[q0] : e->d_wl;
      ca.noise = in_dev ? sp->noise_variance + sp->offsets[q0] : e->d_noise;
      ca.zmin = e->d_m_zmin; ca.zmax = e->d_m_zmax;
      ca.proximity_zone = cuts->proximity_zone; ca.noise_thresh = cuts->noise_thresh; ca.omega_m = cuts->omega_m;
      ca.word_off = batch_wo; ca.words = batch_words; ca.npix = e->d_c_np; ca.z_upper = e->d_c_zu;
      ca.nz[0] = cnz[0]; ca.nz[1] = cnz[1];
      ca.z_edges[0] = e->d_c_edges; ca.z_edges[1] = e->d_c_edges ? e->d_c_edges + cnz[0] + 1 : nullptr;
      ca.path[0] = e->d_c_path[0]; ca.path[1] = e->d_c_path[1];
      TimedLaunch t14{};
      if ((rc = record_start(e, &t14, 14))) return rc;
      HIP_TRY(launch_search_cuts(ca, nq, st));
      HIP_TRY(hipEventRecord(t14.stop, st));
      e->pending.push_back(t14);
      if (cuts->proximity_zone == cuts->proximity_zone) rows_b.cut_z_upper = e->d_c_zu;
      if (cuts->noise_thresh == cuts->noise_thresh) {
        rows_b.cut_npix = e->d_c_np; rows_b.cut_word_off = batch_wo; rows_b.cut_words = batch_words;
      }
      const hipMemcpyKind ck = cres->memory == GPDLA_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
      HIP_TRY(hipMemcpyAsync(cres->z_uppers + q0, e->d_c_zu, nq * 8, ck, st));
      HIP_TRY(hipMemcpyAsync(cres->pixel_counts + q0, e->d_c_np, nq * 4, ck, st));
      if (nwb) HIP_TRY(hipMemcpyAsync(cres->bitmap_words + cut_woff[q0], e->d_c_words, (size_t)nwb * 4, ck, st));
      double* cpaths[2] = {cres->path_summary, cres->path_population};
      for (int g = 0; g < 2; ++g)
        if (cnz[g])
          HIP_TRY(hipMemcpyAsync(cpaths[g] + (size_t)q0 * (cnz[g] + 1), e->d_c_path[g], (size_t)nq * (cnz[g] + 1) * 8, ck, st));
    }
    auto on_grid = [&](const double* log_nhi, int nz, int nn, const double* edges) {
      SampleRowsArgs r = rows_b;
      r.log_nhi = log_nhi; r.nz = nz; r.nn = nn; r.z_edges = edges; r.n_edges = nz ? edges + nz + 1 : nullptr;
      return r;
    };

    if (spec) {
      if ((rc = grow(&e->d_s_ind, &e->cap_s_ind, (size_t)nq * D))) return rc;
      if ((rc = grow(&e->d_s_ll, &e->cap_s_ll, (size_t)nq * D))) return rc;
      if ((rc = grow(&e->d_s_z, &e->cap_s_z, (size_t)nq * D * kMaxDlas))) return rc;
      if ((rc = grow(&e->d_s_n, &e->cap_s_n, (size_t)nq * D * kMaxDlas))) return rc;
      if (nbins && (rc = grow(&e->d_s_planes, &e->cap_s_planes, (size_t)nq * kSummaryPlanes * nbins))) return rc;
      SummaryArgs sa{};
      sa.r = on_grid(e->d_s_lognhi, nzb, nnb, e->d_s_edges); sa.nhi = e->d_nhi_c;
      sa.map_ind = e->d_s_ind; sa.map_ll = e->d_s_ll; sa.map_z = e->d_s_z; sa.map_n = e->d_s_n;
      sa.planes = nbins ? e->d_s_planes : nullptr;
      TimedLaunch t7{};
      if ((rc = record_start(e, &t7, 7))) return rc;
      HIP_TRY(launch_posterior_summary(sa, st));
      HIP_TRY(hipEventRecord(t7.stop, st));
      e->pending.push_back(t7);
      const hipMemcpyKind sk = sums->memory == GPDLA_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
      for (int d = 0; d < D; ++d) {
        const int64_t o = (int64_t)d * Q + q0;
        HIP_TRY(hipMemcpyAsync(sums->map_sample_inds + o, e->d_s_ind + (size_t)d * nq, nq * 4, sk, st));
        HIP_TRY(hipMemcpyAsync(sums->map_log_likelihoods + o, e->d_s_ll + (size_t)d * nq, nq * 8, sk, st));
        HIP_TRY(hipMemcpyAsync(sums->map_z_dlas + o * kMaxDlas, e->d_s_z + (size_t)d * nq * kMaxDlas, nq * kMaxDlas * 8, sk, st));
        HIP_TRY(hipMemcpyAsync(sums->map_log_nhis + o * kMaxDlas, e->d_s_n + (size_t)d * nq * kMaxDlas, nq * kMaxDlas * 8, sk, st));
      }
      if (nbins)
        HIP_TRY(hipMemcpyAsync(sums->bin_planes + (size_t)q0 * kSummaryPlanes * nbins, e->d_s_planes,
                               (size_t)nq * kSummaryPlanes * nbins * 8, sk, st));
    }

    if (mlev) {   // (gpdla_engine_process_spectra_models: spec and mres are set) on the batch the sweeps just used
      ModelBatch mb{};
      mb.q0 = q0; mb.nq = nq; mb.Q = Q; mb.res = mres;
      for (int64_t q = 0; q < nq; ++q)   // the batch's slot capacity, as gpdla_engine_process laid it out
        mb.slots += 4 * ((sp->offsets[q0 + q + 1] - sp->offsets[q0 + q] + 3) / 4) + 4 * kChunkSteps;
      mb.sel.rows = (int32_t)nq; mb.sel.levels = D; mb.sel.ll_dla = e->d_m_lldla;
      mb.sel.map_z = e->d_s_z; mb.sel.map_n = e->d_s_n;
      mb.h_levels = mlev->level_mode == GPDLA_MODEL_LEVEL_GIVEN ? mlev->levels : nullptr;
      mb.h_lp = mlev->level_mode == GPDLA_MODEL_LEVEL_BEST ? mlev->log_priors_dla : nullptr;
      if ((rc = model_spectra_batch(e, mb))) return rc;
    }

    if (ispec) {
      const size_t Ss = (size_t)S, slots = (size_t)nq * D * kMaxDlas, nlev = (size_t)ispec->num_levels;
      if ((rc = grow(&e->d_i_out, &e->cap_i_out, slots * (8 + 2 * nlev)))) return rc;
      if ((rc = grow(&e->d_i_count, &e->cap_i_count, (size_t)nq * D))) return rc;
      IntervalArgs ia{};
      ia.r = on_grid(e->d_i_lognhi, 0, 0, nullptr);
      ia.rank_z = e->d_i_rank; ia.rank_n = e->d_i_rank + Ss; ia.uniq_off = e->d_i_uniq; ia.uniq_n = e->d_i_uniq + Ss;
      ia.lr_delta = ispec->lr_delta; ia.num_levels = ispec->num_levels;
      for (size_t i = 0; i < nlev; ++i) ia.levels[i] = ispec->levels[i];
      double* io = e->d_i_out;
      ia.z_mean = io; ia.z_sd = io + slots; ia.n_mean = io + 2 * slots; ia.n_sd = io + 3 * slots;
      ia.z_lr = io + 4 * slots; ia.n_lr = io + 6 * slots;
      ia.z_q = io + 8 * slots; ia.n_q = ia.z_q + slots * nlev;
      ia.lr_count = e->d_i_count;
      TimedLaunch t13{};
      if ((rc = record_start(e, &t13, 13))) return rc;
      HIP_TRY(launch_posterior_intervals(ia, st));
      HIP_TRY(hipEventRecord(t13.stop, st));
      e->pending.push_back(t13);
      const hipMemcpyKind ik = iv->memory == GPDLA_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
      const size_t per = (size_t)nq * kMaxDlas;   // slots of one level of the batch
      for (int d = 0; d < D; ++d) {
        const size_t src = (size_t)d * per, dst = ((size_t)d * Q + q0) * kMaxDlas;
        HIP_TRY(hipMemcpyAsync(iv->z_means + dst, ia.z_mean + src, per * 8, ik, st));
        HIP_TRY(hipMemcpyAsync(iv->z_sds + dst, ia.z_sd + src, per * 8, ik, st));
        HIP_TRY(hipMemcpyAsync(iv->log_nhi_means + dst, ia.n_mean + src, per * 8, ik, st));
        HIP_TRY(hipMemcpyAsync(iv->log_nhi_sds + dst, ia.n_sd + src, per * 8, ik, st));
        HIP_TRY(hipMemcpyAsync(iv->z_lr_ranges + dst * 2, ia.z_lr + src * 2, per * 2 * 8, ik, st));
        HIP_TRY(hipMemcpyAsync(iv->log_nhi_lr_ranges + dst * 2, ia.n_lr + src * 2, per * 2 * 8, ik, st));
        HIP_TRY(hipMemcpyAsync(iv->z_quantiles + dst * nlev, ia.z_q + src * nlev, per * nlev * 8, ik, st));
        HIP_TRY(hipMemcpyAsync(iv->log_nhi_quantiles + dst * nlev, ia.n_q + src * nlev, per * nlev * 8, ik, st));
        HIP_TRY(hipMemcpyAsync(iv->lr_counts + (size_t)d * Q + q0, e->d_i_count + (size_t)d * nq, nq * 4, ik, st));
      }
    }

    ModelPosteriorArgs ma{};   // the posterior launches of both population halves
    if (pspec) {
      const size_t NL = kPopulationMaxLarge;
      if ((rc = grow(&e->d_p_pdla, &e->cap_p_pdla, (size_t)nq))) return rc;
      if ((rc = grow(&e->d_p_plane, &e->cap_p_plane, (size_t)nq * pbins))) return rc;
      if ((rc = grow(&e->d_p_lind, &e->cap_p_lind, (size_t)nq * NL))) return rc;
      if ((rc = grow(&e->d_p_lprob, &e->cap_p_lprob, (size_t)nq * NL))) return rc;
      if ((rc = grow(&e->d_p_lbin, &e->cap_p_lbin, (size_t)nq * NL))) return rc;
      ma.rows = (int32_t)nq; ma.levels = D; ma.ll_null = e->d_m_null; ma.ll_dla = e->d_m_lldla;
      ma.ll_lls = sub ? e->d_sub_ev : nullptr;
      ma.lp_no = e->d_p_lpno + q0; ma.lp_dla = e->d_p_lpdla + q0; ma.lp_lls = sub ? e->d_p_lplls + q0 : nullptr;
      ma.ld_prior = Q; ma.p_dla = e->d_p_pdla;
      PopulationSplitArgs pa{};
      pa.r = on_grid(e->d_p_lognhi, pnz, pnn, e->d_p_edges);
      pa.r.levels = 1; pa.r.base = nullptr;   // the level-1 rows alone
      pa.level_post = e->d_p_pdla; pa.ld_post = nq;
      pa.p_thresh_sample = pspec->p_thresh_sample; pa.p_switch = pspec->p_switch;
      pa.poisson = e->d_p_plane; pa.large_inds = e->d_p_lind; pa.large_probs = e->d_p_lprob; pa.large_bins = e->d_p_lbin;
      TimedLaunch t11{};
      if ((rc = record_start(e, &t11, 11))) return rc;
      HIP_TRY(launch_model_posterior(ma, st));
      HIP_TRY(launch_population_split(pa, st));
      HIP_TRY(hipEventRecord(t11.stop, st));
      e->pending.push_back(t11);
      const hipMemcpyKind pk = pop->memory == GPDLA_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
      HIP_TRY(hipMemcpyAsync(pop->p_dlas + q0, e->d_p_pdla, nq * 8, pk, st));
      HIP_TRY(hipMemcpyAsync(pop->poisson_plane + (size_t)q0 * pbins, e->d_p_plane, (size_t)nq * pbins * 8, pk, st));
      HIP_TRY(hipMemcpyAsync(pop->large_inds + (size_t)q0 * NL, e->d_p_lind, (size_t)nq * NL * 4, pk, st));
      HIP_TRY(hipMemcpyAsync(pop->large_probs + (size_t)q0 * NL, e->d_p_lprob, (size_t)nq * NL * 8, pk, st));
      HIP_TRY(hipMemcpyAsync(pop->large_bins + (size_t)q0 * NL, e->d_p_lbin, (size_t)nq * NL * 4, pk, st));
    }

    if (lv) {
      const size_t NL = kPopulationMaxLarge, Ds = (size_t)D;
      if (lv_planes && (rc = grow(&e->d_lv_planes, &e->cap_lv_planes, (size_t)nq * Ds * kSummaryPlanes * nbins))) return rc;
      if (lv_split) {
        if ((rc = grow(&e->d_lv_post, &e->cap_lv_post, (size_t)nq * Ds))) return rc;
        if ((rc = grow(&e->d_lv_plane, &e->cap_lv_plane, (size_t)nq * Ds * pbins))) return rc;
        if ((rc = grow(&e->d_lv_lind, &e->cap_lv_lind, (size_t)nq * Ds * NL))) return rc;
        if ((rc = grow(&e->d_lv_lprob, &e->cap_lv_lprob, (size_t)nq * Ds * NL))) return rc;
        if ((rc = grow(&e->d_lv_lbin, &e->cap_lv_lbin, (size_t)nq * Ds * NL * kMaxDlas))) return rc;
      }
      TimedLaunch t12{};
      if ((rc = record_start(e, &t12, 12))) return rc;
      if (lv_planes) {
        LevelPlanesArgs la{};
        la.r = on_grid(e->d_s_lognhi, nzb, nnb, e->d_s_edges);
        la.nhi = e->d_nhi_c; la.planes = e->d_lv_planes;
        HIP_TRY(launch_level_planes(la, st));
      }
      if (lv_split) {                      // with a population spec: ma is filled
        ma.level_post = e->d_lv_post;
        LevelSplitArgs la{};
        la.r = on_grid(e->d_p_lognhi, pnz, pnn, e->d_p_edges);
        la.level_post = e->d_lv_post; la.ld_post = nq;
        la.p_thresh_sample = pspec->p_thresh_sample; la.p_switch = pspec->p_switch;
        la.poisson = e->d_lv_plane; la.large_inds = e->d_lv_lind; la.large_probs = e->d_lv_lprob; la.large_bins = e->d_lv_lbin;
        HIP_TRY(launch_level_posterior(ma, st));
        HIP_TRY(launch_level_split(la, st));
      }
      HIP_TRY(hipEventRecord(t12.stop, st));
      e->pending.push_back(t12);
      const hipMemcpyKind lk = lv->memory == GPDLA_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
      if (lv_planes)
        HIP_TRY(hipMemcpyAsync(lv->bin_planes + (size_t)q0 * Ds * kSummaryPlanes * nbins, e->d_lv_planes,
                               (size_t)nq * Ds * kSummaryPlanes * nbins * 8, lk, st));
      if (lv_split) {
        for (int d = 0; d < D; ++d)
          HIP_TRY(hipMemcpyAsync(lv->level_posteriors + (int64_t)d * Q + q0, e->d_lv_post + (size_t)d * nq, nq * 8, lk, st));
        HIP_TRY(hipMemcpyAsync(lv->poisson_plane + (size_t)q0 * Ds * pbins, e->d_lv_plane, (size_t)nq * Ds * pbins * 8, lk, st));
        HIP_TRY(hipMemcpyAsync(lv->large_inds + (size_t)q0 * Ds * NL, e->d_lv_lind, (size_t)nq * Ds * NL * 4, lk, st));
        HIP_TRY(hipMemcpyAsync(lv->large_probs + (size_t)q0 * Ds * NL, e->d_lv_lprob, (size_t)nq * Ds * NL * 8, lk, st));
        HIP_TRY(hipMemcpyAsync(lv->large_bins + (size_t)q0 * Ds * NL * kMaxDlas, e->d_lv_lbin,
                               (size_t)nq * Ds * NL * kMaxDlas * 4, lk, st));
      }
    }

    HIP_TRY(hipMemcpyAsync(res->log_likelihoods_no_dla + q0, e->d_m_null, nq * 8, out_kind, st));
    if (res->min_z_dlas) HIP_TRY(hipMemcpyAsync(res->min_z_dlas + q0, e->d_m_zmin, nq * 8, out_kind, st));
    if (res->max_z_dlas) HIP_TRY(hipMemcpyAsync(res->max_z_dlas + q0, e->d_m_zmax, nq * 8, out_kind, st));
    if (res->num_pixels) HIP_TRY(hipMemcpyAsync(res->num_pixels + q0, e->d_m_npix, nq * 4, out_kind, st));
    for (int d = 1; d <= D; ++d) {
      HIP_TRY(hipMemcpyAsync(res->log_likelihoods_dla + (int64_t)(d - 1) * Q + q0, e->d_m_lldla + (size_t)(d - 1) * nq,
                             nq * 8, out_kind, st));
      if (res->sample_log_likelihoods_dla)
        HIP_TRY(hipMemcpy2DAsync(res->sample_log_likelihoods_dla + ((int64_t)(d - 1) * Q + q0) * res->sample_ld,
                                 res->sample_ld * 8, e->d_m_sll + (size_t)(d - 1) * plane, S * 8, S * 8, nq, out_kind, st));
      if (res->base_sample_inds && d >= 2)
        HIP_TRY(hipMemcpy2DAsync(res->base_sample_inds + ((int64_t)(d - 2) * Q + q0) * res->sample_ld,
                                 res->sample_ld * 4, e->d_m_base + (size_t)(d - 2) * plane, S * 4, S * 4, nq, out_kind, st));
    }
    // the level workspaces are reused by the next batch: drain
    HIP_TRY(hipStreamSynchronize(st));
  }
  return gpdla_engine_synchronize(e);
}

int gpdla_engine_process_multi(gpdla_engine* e, const gpdla_spectra* sp, const gpdla_multi_dla* mu,
                               const gpdla_results_multi* res) {
  return process_multi_impl(e, sp, mu, res, nullptr, nullptr);
}

int gpdla_engine_process_summaries(gpdla_engine* e, const gpdla_spectra* sp, const gpdla_multi_dla* mu,
                                   const gpdla_results_multi* res, const gpdla_summary_spec* spec,
                                   const gpdla_summaries* sums) {
  if (!spec || !sums) return set_error(GPDLA_EINVAL, "null argument");
  return process_multi_impl(e, sp, mu, res, spec, sums);
}

int gpdla_engine_process_intervals(gpdla_engine* e, const gpdla_spectra* sp, const gpdla_multi_dla* mu,
                                   const gpdla_results_multi* res, const gpdla_summary_spec* spec,
                                   const gpdla_summaries* sums, const gpdla_interval_spec* ispec,
                                   const gpdla_intervals* iv) {
  if (!spec || !sums || !ispec || !iv) return set_error(GPDLA_EINVAL, "null argument");
  return process_multi_impl(e, sp, mu, res, spec, sums, nullptr, nullptr, nullptr, nullptr, nullptr, ispec, iv);
}

int gpdla_engine_get_interval_stats(gpdla_engine* e, double* ms, int64_t* launches) {
  if (!e || !ms || !launches) return set_error(GPDLA_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  int rc = resolve_events(e);
  if (rc) return rc;
  *ms = e->interval_ms;
  *launches = e->interval_launches;
  return GPDLA_OK;
}

// ---------------------------------------------------------------------------------------------
// sub-DLA model and Lyman-series forest (include/gpdla.h; kernels in forest.hip)
// ---------------------------------------------------------------------------------------------
int gpdla_engine_process_models(gpdla_engine* e, const gpdla_spectra* sp, const gpdla_multi_dla* mu,
                                const gpdla_sub_dla* sub, const gpdla_results_multi* res,
                                const gpdla_results_sub* rsub, const gpdla_summary_spec* spec,
                                const gpdla_summaries* sums) {
  if (spec && !sums) return set_error(GPDLA_EINVAL, "null argument");
  if (sub && !rsub) return set_error(GPDLA_EINVAL, "null sub-DLA results");
  return process_multi_impl(e, sp, mu, res, spec, spec ? sums : nullptr, sub, sub ? rsub : nullptr);
}

int gpdla_engine_process_population(gpdla_engine* e, const gpdla_spectra* sp, const gpdla_multi_dla* mu,
                                    const gpdla_sub_dla* sub, const gpdla_results_multi* res,
                                    const gpdla_results_sub* rsub, const gpdla_summary_spec* spec,
                                    const gpdla_summaries* sums, const gpdla_population_spec* pspec,
                                    const gpdla_population* pop) {
  if (spec && !sums) return set_error(GPDLA_EINVAL, "null argument");
  if (sub && !rsub) return set_error(GPDLA_EINVAL, "null sub-DLA results");
  if ((pspec == nullptr) != (pop == nullptr)) return set_error(GPDLA_EINVAL, "population spec and outputs go together");
  return process_multi_impl(e, sp, mu, res, spec, spec ? sums : nullptr, sub, sub ? rsub : nullptr, pspec, pop);
}

int gpdla_engine_process_levels(gpdla_engine* e, const gpdla_spectra* sp, const gpdla_multi_dla* mu,
                                const gpdla_sub_dla* sub, const gpdla_results_multi* res,
                                const gpdla_results_sub* rsub, const gpdla_summary_spec* spec,
                                const gpdla_summaries* sums, const gpdla_population_spec* pspec,
                                const gpdla_population* pop, const gpdla_level_population* lv) {
  if (spec && !sums) return set_error(GPDLA_EINVAL, "null argument");
  if (sub && !rsub) return set_error(GPDLA_EINVAL, "null sub-DLA results");
  if ((pspec == nullptr) != (pop == nullptr)) return set_error(GPDLA_EINVAL, "population spec and outputs go together");
  return process_multi_impl(e, sp, mu, res, spec, spec ? sums : nullptr, sub, sub ? rsub : nullptr, pspec, pop, lv);
}

int gpdla_engine_process_cuts(gpdla_engine* e, const gpdla_spectra* sp, const gpdla_multi_dla* mu,
                              const gpdla_sub_dla* sub, const gpdla_results_multi* res,
                              const gpdla_results_sub* rsub, const gpdla_summary_spec* spec,
                              const gpdla_summaries* sums, const gpdla_population_spec* pspec,
                              const gpdla_population* pop, const gpdla_level_population* lv,
                              const gpdla_search_cuts* cuts, const gpdla_search_cut_results* cres) {
  if (spec && !sums) return set_error(GPDLA_EINVAL, "null argument");
  if (sub && !rsub) return set_error(GPDLA_EINVAL, "null sub-DLA results");
  if ((pspec == nullptr) != (pop == nullptr)) return set_error(GPDLA_EINVAL, "population spec and outputs go together");
  if ((cuts == nullptr) != (cres == nullptr)) return set_error(GPDLA_EINVAL, "search cuts: spec and results go together");
  return process_multi_impl(e, sp, mu, res, spec, spec ? sums : nullptr, sub, sub ? rsub : nullptr, pspec, pop, lv, nullptr,
                            nullptr, cuts, cres);
}

int gpdla_engine_get_cut_stats(gpdla_engine* e, double* ms, int64_t* launches) {
  if (!e || !ms || !launches) return set_error(GPDLA_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  int rc = resolve_events(e);
  if (rc) return rc;
  *ms = e->cut_ms;
  *launches = e->cut_launches;
  return GPDLA_OK;
}

// ---------------------------------------------------------------------------------------------
// model spectra (include/gpdla.h "Model spectra"; kernel in model_spectra.hip)
// ---------------------------------------------------------------------------------------------
int gpdla_engine_get_model_spectra_stats(gpdla_engine* e, double* ms, int64_t* launches) {
  if (!e || !ms || !launches) return set_error(GPDLA_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  int rc = resolve_events(e);
  if (rc) return rc;
  *ms = e->model_spectra_ms;
  *launches = e->model_spectra_launches;
  return GPDLA_OK;
}

int gpdla_engine_process_spectra_models(gpdla_engine* e, const gpdla_spectra* sp, const gpdla_multi_dla* mu,
                                        const gpdla_results_multi* res, const gpdla_summary_spec* spec,
                                        const gpdla_summaries* sums, const gpdla_interval_spec* ispec,
                                        const gpdla_intervals* iv, const gpdla_model_levels* mspec,
                                        const gpdla_model_spectra* mres) {
  if (!e || !sp || !mu || !spec || !sums || !mspec || !mres) return set_error(GPDLA_EINVAL, "null argument");
  if ((ispec == nullptr) != (iv == nullptr)) return set_error(GPDLA_EINVAL, "interval spec and arrays go together");
  if (e->gemm || e->i8)
    return set_error(GPDLA_EUNSUPPORTED, "the model spectra need the fused fp64 path (this engine runs a panel-GEMM or int8 path)");
  if (!model_spectra_supported(e->K)) return set_error(GPDLA_EUNSUPPORTED, "model spectra: rank %d is not compiled", e->K);
  const int64_t Q = sp->num_spectra;
  if (Q < 0) return set_error(GPDLA_EINVAL, "num_spectra < 0");
  if (mspec->level_mode != GPDLA_MODEL_LEVEL_BEST && mspec->level_mode != GPDLA_MODEL_LEVEL_GIVEN)
    return set_error(GPDLA_EINVAL, "model spectra: level_mode=%d", mspec->level_mode);
  if (mspec->level_mode == GPDLA_MODEL_LEVEL_GIVEN) {
    if (!mspec->levels) return set_error(GPDLA_EINVAL, "model spectra: null levels");
    for (int64_t q = 0; q < Q; ++q)
      if (mspec->levels[q] < 0 || mspec->levels[q] > mu->max_dlas)
        return set_error(GPDLA_EINVAL, "model spectra: levels[%lld] = %d outside 0..%d", (long long)q, (int)mspec->levels[q],
                         mu->max_dlas);
  } else if (mu->max_dlas > 1 && !mspec->log_priors_dla) {
    return set_error(GPDLA_EINVAL, "model spectra: the best level of max_dlas=%d needs log_priors_dla", mu->max_dlas);
  }
  if (Q > 0) {
    if (!sp->offsets) return set_error(GPDLA_EINVAL, "null spectra array");
    int rcr = model_spectra_check_results(mres, Q);
    if (rcr) return rcr;
    HIP_TRY(hipSetDevice(e->device));
    int rcg = grow(&e->d_ms_status, &e->cap_ms_status, 1);
    if (rcg) return rcg;
    HIP_TRY(hipMemsetAsync(e->d_ms_status, 0, 4, e->stream));
  }
  const int rc = process_multi_impl(e, sp, mu, res, spec, sums, nullptr, nullptr, nullptr, nullptr, nullptr, ispec, iv,
                                    nullptr, nullptr, mspec, mres);
  if (rc < 0 || Q == 0) return rc;
  const int rcm = model_spectra_finish(e, Q, mres);
  return rcm ? rcm : rc;
}

int gpdla_engine_model_spectra(gpdla_engine* e, const gpdla_spectra* sp, const gpdla_model_absorbers* ab,
                               const gpdla_model_spectra* res) {
  if (!e || !sp || !ab || !res) return set_error(GPDLA_EINVAL, "null argument");
  if (e->gemm || e->i8)
    return set_error(GPDLA_EUNSUPPORTED, "the model spectra need the fused fp64 path (this engine runs a panel-GEMM or int8 path)");
  if (!model_spectra_supported(e->K)) return set_error(GPDLA_EUNSUPPORTED, "model spectra: rank %d is not compiled", e->K);
  const int64_t Q = sp->num_spectra;
  if (Q < 0) return set_error(GPDLA_EINVAL, "num_spectra < 0");
  if (Q == 0) return GPDLA_OK;
  if (!sp->offsets || !sp->wavelengths || !sp->flux || !sp->noise_variance || !sp->pixel_mask || !sp->z_qsos)
    return set_error(GPDLA_EINVAL, "null spectra array");
  if (sp->memory != GPDLA_MEM_HOST && sp->memory != GPDLA_MEM_DEVICE) return set_error(GPDLA_EINVAL, "spectra memory=%d", sp->memory);
  { const int rcr = model_spectra_check_results(res, Q); if (rcr) return rcr; }
  if (!ab->counts || !ab->z_dlas || !ab->log_nhis) return set_error(GPDLA_EINVAL, "model spectra: null absorber array");
  if (sp->offsets[0] < 0) return set_error(GPDLA_EINVAL, "offsets[0] < 0");
  for (int64_t q = 0; q < Q; ++q) {
    if (sp->offsets[q + 1] < sp->offsets[q]) return set_error(GPDLA_EINVAL, "offsets not monotone at %lld", (long long)q);
    if (ab->counts[q] < 0 || ab->counts[q] > GPDLA_MAX_DLAS)
      return set_error(GPDLA_EINVAL, "model spectra: counts[%lld] = %d outside 0..%d", (long long)q, (int)ab->counts[q],
                       GPDLA_MAX_DLAS);
  }
  const bool in_dev = sp->memory == GPDLA_MEM_DEVICE, out_dev = res->memory == GPDLA_MEM_DEVICE;
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t st = e->stream;
  int rc;
  // (pageable host staging below: every batch ends with a synchronisation)
  HIP_TRY(hipStreamSynchronize(st));
  if ((rc = grow(&e->d_ms_status, &e->cap_ms_status, 1))) return rc;
  HIP_TRY(hipMemsetAsync(e->d_ms_status, 0, 4, st));

  const int64_t QB = e->params.max_batch_spectra > 0 ? e->params.max_batch_spectra : 1024;
  const int64_t row = panel_row_doubles(e->K);
  const size_t per_batch = (size_t)(QB + 1) + 4 * (size_t)QB;   // gpdla_engine_process's metadata layout
  std::vector<int64_t> hm(per_batch);
  for (int64_t q0 = 0; q0 < Q; q0 += QB) {
    const int64_t q1 = std::min(Q, q0 + QB), nq = q1 - q0;
    int64_t* h_off = hm.data();
    int64_t* h_sb = h_off + (QB + 1);
    int64_t* h_lb = h_sb + QB;
    int64_t* h_sc = h_lb + QB;
    int64_t slots = 0, lams = 0;
    for (int64_t q = 0; q < nq; ++q) {   // (as gpdla_engine_process lays a batch out)
      h_off[q] = sp->offsets[q0 + q] - sp->offsets[q0];
      const int64_t lpix = sp->offsets[q0 + q + 1] - sp->offsets[q0 + q];
      const int64_t cap = 4 * ((lpix + 3) / 4) + 4 * kChunkSteps;
      h_sb[q] = slots; h_lb[q] = lams; h_sc[q] = cap;
      slots += cap;
      lams += cap + 8;
    }
    h_off[nq] = sp->offsets[q1] - sp->offsets[q0];
    const int64_t npix = h_off[nq], pbase = sp->offsets[q0];
    if ((rc = grow(&e->d_meta, &e->cap_meta, per_batch))) return rc;
    if ((rc = grow(&e->d_info, &e->cap_q, (size_t)QB))) return rc;
    if ((rc = grow(&e->d_panel, &e->cap_slots, (size_t)(slots * row + panel_lds_row_doubles(e->K))))) return rc;
    if ((rc = grow(&e->d_lam, &e->cap_lam, (size_t)lams))) return rc;
    if ((rc = grow(&e->d_smap, &e->cap_smap, (size_t)slots))) return rc;
    HIP_TRY(hipMemcpyAsync(e->d_meta, hm.data(), per_batch * sizeof(int64_t), hipMemcpyHostToDevice, st));
    const double *wl, *fl, *nv, *zq;
    const uint8_t* mk;
    if (in_dev) {
      wl = sp->wavelengths + pbase; fl = sp->flux + pbase; nv = sp->noise_variance + pbase;
      mk = sp->pixel_mask + pbase; zq = sp->z_qsos + q0;
    } else {
      if ((rc = grow(&e->d_wl, &e->cap_wl, (size_t)npix))) return rc;
      if ((rc = grow(&e->d_flux, &e->cap_flux, (size_t)npix))) return rc;
      if ((rc = grow(&e->d_noise, &e->cap_noise, (size_t)npix))) return rc;
      if ((rc = grow(&e->d_mask, &e->cap_mask, (size_t)npix))) return rc;
      if ((rc = grow(&e->d_z, &e->cap_z, (size_t)nq))) return rc;
      HIP_TRY(hipMemcpyAsync(e->d_wl, sp->wavelengths + pbase, npix * 8, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(e->d_flux, sp->flux + pbase, npix * 8, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(e->d_noise, sp->noise_variance + pbase, npix * 8, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(e->d_mask, sp->pixel_mask + pbase, npix, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(e->d_z, sp->z_qsos + q0, nq * 8, hipMemcpyHostToDevice, st));
      wl = e->d_wl; fl = e->d_flux; nv = e->d_noise; mk = e->d_mask; zq = e->d_z;
    }
    PrepArgs pa{};
    pa.q_count = (int32_t)nq;
    pa.offsets = e->d_meta;
    pa.wavelengths = wl; pa.flux = fl; pa.noise = nv; pa.mask = mk; pa.z_qsos = zq;
    pa.slot_base = e->d_meta + (QB + 1);
    pa.lam_base = pa.slot_base + QB;
    pa.slot_cap = pa.lam_base + QB;
    pa.num_rest = e->num_rest;
    pa.rest = e->d_rest; pa.mu = e->d_mu; pa.M_rowmajor = e->d_M; pa.log_omega = e->d_logom;
    pa.c_0 = e->c0; pa.tau_0 = e->tau0; pa.beta = e->beta;
    pa.min_lambda = e->params.min_lambda; pa.max_lambda = e->params.max_lambda;
    pa.lya = e->params.lya_wavelength; pa.lyman_limit = e->params.lyman_limit;
    pa.min_z_cut = e->params.min_z_cut; pa.max_z_cut = e->params.max_z_cut;
    pa.pixel_spacing = e->params.pixel_spacing;
    pa.absorption_mode = e->params.absorption_mode;
    pa.om2_hi_e = e->om2_hi_e;
    pa.info = e->d_info; pa.panel = e->d_panel; pa.lam_pad = e->d_lam; pa.slot_pixel = e->d_smap;
    pa.k = e->K;
    TimedLaunch t0{};
    if ((rc = record_start(e, &t0, 0))) return rc;
    HIP_TRY(launch_prep(e->K, pa, st));
    HIP_TRY(hipEventRecord(t0.stop, st));
    e->pending.push_back(t0);
    if (e->forest_on) {   // as gpdla_engine_process applies it
      ForestArgs fa{};
      fa.q_count = (int32_t)nq; fa.info = e->d_info; fa.offsets = e->d_meta; fa.wavelengths = wl; fa.z_qsos = zq;
      fa.slot_cap = pa.slot_cap; fa.slot_pixel = e->d_smap;
      fa.num_rest = e->num_rest; fa.rest = e->d_rest; fa.log_omega = e->d_logom;
      fa.c_0 = e->c0; fa.tau_0 = e->tau0; fa.beta = e->beta;
      fa.mf_tau_0 = e->forest.mean_flux_tau_0; fa.mf_beta = e->forest.mean_flux_beta;
      fa.num_lines = e->forest.num_forest_lines;
      fa.variance_series = e->forest.variance_series != 0; fa.mean_flux = e->forest.mean_flux != 0;
      fa.mean_flux_scope = e->forest_scope;
      fa.panel = e->d_panel;
      TimedLaunch t8{};
      if ((rc = record_start(e, &t8, 8))) return rc;
      HIP_TRY(launch_forest(e->K, fa, st));
      if (e->forest_scope != 0) HIP_TRY(launch_forest_covariance(e->K, fa, st));
      HIP_TRY(hipEventRecord(t8.stop, st));
      e->pending.push_back(t8);
    }

    ModelBatch mb{};
    mb.q0 = q0; mb.nq = nq; mb.slots = slots; mb.res = res; mb.ab = ab;
    if ((rc = model_spectra_batch(e, mb))) return rc;
  }
  if ((rc = resolve_events(e))) return rc;
  return model_spectra_finish(e, Q, res);
}

int gpdla_engine_get_level_population_stats(gpdla_engine* e, double* ms, int64_t* launches) {
  if (!e || !ms || !launches) return set_error(GPDLA_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  int rc = resolve_events(e);
  if (rc) return rc;
  *ms = e->level_population_ms;
  *launches = e->level_population_launches;
  return GPDLA_OK;
}

int gpdla_engine_get_population_stats(gpdla_engine* e, double* ms, int64_t* launches) {
  if (!e || !ms || !launches) return set_error(GPDLA_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  int rc = resolve_events(e);
  if (rc) return rc;
  *ms = e->population_ms;
  *launches = e->population_launches;
  return GPDLA_OK;
}

int gpdla_engine_set_forest(gpdla_engine* e, const gpdla_forest* f) { return gpdla_engine_set_forest_scoped(e, f, 0); }

int gpdla_engine_set_forest_scoped(gpdla_engine* e, const gpdla_forest* f, int32_t scope) {
  if (!e) return set_error(GPDLA_EINVAL, "null engine");
  if (scope < 0 || scope > 2) return set_error(GPDLA_EINVAL, "mean_flux_scope=%d outside [0, 2]", scope);
  if (!f) {
    if (scope != 0) return set_error(GPDLA_EINVAL, "mean_flux_scope=%d without a forest", scope);
    e->forest_on = false;
    e->forest = gpdla_forest{};
    e->forest_scope = 0;
    return GPDLA_OK;
  }
  if (scope != 0 && f->mean_flux == 0)
    return set_error(GPDLA_EINVAL, "mean_flux_scope=%d needs mean_flux (there is no mean flux to multiply by)", scope);
  if (f->num_forest_lines < 1 || f->num_forest_lines > kMaxLines)
    return set_error(GPDLA_EINVAL, "num_forest_lines=%d outside [1, %d]", f->num_forest_lines, kMaxLines);
  if (!(f->mean_flux_tau_0 >= 0.0 && f->mean_flux_tau_0 < INFINITY))
    return set_error(GPDLA_EINVAL, "mean_flux_tau_0 = %g: must be finite and >= 0", f->mean_flux_tau_0);
  if (!std::isfinite(f->mean_flux_beta)) return set_error(GPDLA_EINVAL, "mean_flux_beta = %g: must be finite", f->mean_flux_beta);
  if (e->gemm || e->i8)
    return set_error(GPDLA_EUNSUPPORTED, "the forest needs the fused fp64 path (this engine runs a panel-GEMM or int8 path)");
  e->forest = *f;
  e->forest_on = f->variance_series != 0 || f->mean_flux != 0;
  e->forest_scope = scope;
  return GPDLA_OK;
}

int gpdla_engine_get_model_stats(gpdla_engine* e, gpdla_model_stats* s) {
  if (!e || !s) return set_error(GPDLA_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  int rc = resolve_events(e);
  if (rc) return rc;
  *s = e->model_stats;
  return GPDLA_OK;
}

int gpdla_forest_f64(int32_t device, const double* wavelengths, int64_t n, double z_qso, double tau_0,
                     double beta, int32_t num_forest_lines, double* out) {
  if (!wavelengths || !out || n < 0) return set_error(GPDLA_EINVAL, "null argument or n < 0");
  if (num_forest_lines < 1 || num_forest_lines > kMaxLines)
    return set_error(GPDLA_EINVAL, "num_forest_lines=%d outside [1, %d]", num_forest_lines, kMaxLines);
  if (!(tau_0 >= 0.0 && tau_0 < INFINITY) || !std::isfinite(beta) || !std::isfinite(z_qso))
    return set_error(GPDLA_EINVAL, "tau_0 = %g, beta = %g, z_qso = %g: must be finite, tau_0 >= 0", tau_0, beta, z_qso);
  int rc = check_device(device);
  if (rc) return rc;
  if (n == 0) return GPDLA_OK;
  HIP_TRY(hipSetDevice(device));
  DeviceStage st;
  const size_t o_wl = st.carve((size_t)n * 8), o_out = st.carve((size_t)n * 8);
  HIP_TRY_IN("forest", st.alloc());
  HIP_TRY_IN("forest", st.upload(o_wl, wavelengths, (size_t)n * 8));
  HIP_TRY_IN("forest", launch_forest_f64(st.ptr<const double>(o_wl), n, z_qso, tau_0, beta, num_forest_lines,
                                         st.ptr<double>(o_out), nullptr));
  HIP_TRY_IN("forest", st.download(out, o_out, (size_t)n * 8));
  return GPDLA_OK;
}

int gpdla_engine_get_summary_stats(gpdla_engine* e, double* ms, int64_t* launches) {
  if (!e || !ms || !launches) return set_error(GPDLA_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  int rc = resolve_events(e);
  if (rc) return rc;
  *ms = e->summary_ms;
  *launches = e->summary_launches;
  return GPDLA_OK;
}

int gpdla_posterior_summary_f64(int32_t device, const double* ll, int64_t rows, int64_t S, int64_t ld,
                                const double* offset_samples, const double* log_nhi_samples,
                                const double* nhi_samples, const double* min_z, const double* max_z,
                                const int32_t* base_inds, int32_t levels, const gpdla_summary_spec* spec,
                                int32_t* map_sample_inds, double* map_log_likelihoods, double* map_z_dlas,
                                double* map_log_nhis, double* bin_planes) {
  HostSampleRows h{ll, rows, S, ld, offset_samples, log_nhi_samples, nhi_samples, min_z, max_z, base_inds, levels};
  int rc = h.check(nhi_samples && spec && map_sample_inds && map_log_likelihoods && map_z_dlas && map_log_nhis);
  if (rc) return rc;
  if ((rc = validate_summary_grid(spec))) return rc;
  h.nz = spec->num_z_bins; h.nn = spec->num_nhi_bins; h.z_edges = spec->z_edges; h.n_edges = spec->log_nhi_edges;
  const size_t nbins = (size_t)h.nz * h.nn;
  if (nbins && !bin_planes) return set_error(GPDLA_EINVAL, "null bin_planes with a grid");
  if ((rc = check_device(device))) return rc;
  if (rows == 0) return GPDLA_OK;
  HIP_TRY(hipSetDevice(device));
  const size_t LR = (size_t)levels * rows;
  DeviceStage st;
  h.carve(st);
  const size_t o_ind = st.carve(LR * 4), o_mll = st.carve(LR * 8), o_mz = st.carve(LR * kMaxDlas * 8);
  const size_t o_mn = st.carve(LR * kMaxDlas * 8), o_pl = st.carve((size_t)rows * kSummaryPlanes * nbins * 8);
  SummaryArgs sa{};
  HIP_TRY_IN("posterior_summary", st.alloc());
  HIP_TRY_IN("posterior_summary", h.upload(st, &sa.r, &sa.nhi));
  sa.map_ind = st.ptr<int32_t>(o_ind); sa.map_ll = st.ptr<double>(o_mll);
  sa.map_z = st.ptr<double>(o_mz); sa.map_n = st.ptr<double>(o_mn);
  sa.planes = nbins ? st.ptr<double>(o_pl) : nullptr;
  HIP_TRY_IN("posterior_summary", launch_posterior_summary(sa, nullptr));
  HIP_TRY_IN("posterior_summary", st.download(map_sample_inds, o_ind, LR * 4));
  HIP_TRY_IN("posterior_summary", st.download(map_log_likelihoods, o_mll, LR * 8));
  HIP_TRY_IN("posterior_summary", st.download(map_z_dlas, o_mz, LR * kMaxDlas * 8));
  HIP_TRY_IN("posterior_summary", st.download(map_log_nhis, o_mn, LR * kMaxDlas * 8));
  if (nbins) HIP_TRY_IN("posterior_summary", st.download(bin_planes, o_pl, (size_t)rows * kSummaryPlanes * nbins * 8));
  return GPDLA_OK;
}

int gpdla_resample_f64(int32_t device, const double* ll, int64_t rows, int64_t S, int64_t ld, const double* u,
                       int32_t* out_inds) {
  if (!ll || !u || !out_inds) return set_error(GPDLA_EINVAL, "null argument");
  if (rows < 0 || S < 1 || ld < S || rows > INT32_MAX || S > INT32_MAX)
    return set_error(GPDLA_EINVAL, "rows=%lld S=%lld ld=%lld", (long long)rows, (long long)S, (long long)ld);
  for (int64_t j = 0; j < S; ++j)
    if (!(u[j] >= 0.0 && u[j] < 1.0)) return set_error(GPDLA_EINVAL, "u[%lld] = %g outside [0, 1)", (long long)j, u[j]);
  int rc = check_device(device);
  if (rc) return rc;
  if (rows == 0) return GPDLA_OK;
  HIP_TRY(hipSetDevice(device));
  DeviceStage st;
  const size_t o_ll = st.carve((size_t)rows * ld * 8), o_u = st.carve((size_t)S * 8), o_b = st.carve((size_t)rows * S * 4);
  const size_t o_c = st.carve(S > GPDLA_RESAMPLE_LDS ? (size_t)rows * S * 8 : 0);
  HIP_TRY_IN("resample", st.alloc());
  HIP_TRY_IN("resample", st.upload(o_ll, ll, (size_t)rows * ld * 8));
  HIP_TRY_IN("resample", st.upload(o_u, u, (size_t)S * 8));
  ResampleArgs ra{};
  ra.rows = (int32_t)rows; ra.ll = st.ptr<const double>(o_ll); ra.ld = ld; ra.S = S; ra.u = st.ptr<const double>(o_u);
  ra.cws = S > GPDLA_RESAMPLE_LDS ? st.ptr<double>(o_c) : nullptr; ra.base_inds = st.ptr<int32_t>(o_b);
  HIP_TRY_IN("resample", launch_resample(ra, nullptr));
  HIP_TRY_IN("resample", st.download(out_inds, o_b, (size_t)rows * S * 4));
  return GPDLA_OK;
}


// ---------------------------------------------------------------------------------------------
// device buffer helpers
// ---------------------------------------------------------------------------------------------
int gpdla_device_malloc(int32_t device, int64_t bytes, void** ptr) {
  if (!ptr || bytes < 0) return set_error(GPDLA_EINVAL, "bad argument");
  *ptr = nullptr;
  int rc = check_device(device);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipMalloc(ptr, bytes > 0 ? bytes : 1));
  return GPDLA_OK;
}

int gpdla_device_free(int32_t device, void* ptr) {
  int rc = check_device(device);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  if (ptr) HIP_TRY(hipFree(ptr));
  return GPDLA_OK;
}

int gpdla_memcpy_htod(int32_t device, void* dst, const void* src, int64_t bytes) {
  int rc = check_device(device);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return GPDLA_OK;
}

int gpdla_memcpy_dtoh(int32_t device, void* dst, const void* src, int64_t bytes) {
  int rc = check_device(device);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return GPDLA_OK;
}

// ---------------------------------------------------------------------------------------------
// standalone entry points (host buffers)
// ---------------------------------------------------------------------------------------------
static int lines_on_device(double** d_lines) {
  static std::mutex mu;
  static std::vector<double*> per_dev;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  if ((int)per_dev.size() <= dev) per_dev.resize(dev + 1, nullptr);
  if (!per_dev[dev]) {
    const std::vector<double>& lines = host_line_data().buf;
    double* p = nullptr;
    HIP_TRY(hipMalloc((void**)&p, lines.size() * 8));
    HIP_TRY(hipMemcpy(p, lines.data(), lines.size() * 8, hipMemcpyHostToDevice));
    per_dev[dev] = p;
  }
  *d_lines = per_dev[dev];
  return GPDLA_OK;
}

// Device and pinned host buffers of the standalone entry points, cached per device and grown on
// demand, plus a non-blocking stream: the MEX drop-ins are called once per
// sample from a MATLAB loop, so a call is one memcpy into pinned memory, one H2D copy, the kernel,
// one D2H copy and a stream synchronisation -- no allocation, no pageable copies, no memset.
// Calls are serialised per device.
struct StandaloneBufs {
  std::mutex mu;
  char* buf = nullptr;    // device
  char* host = nullptr;   // pinned host staging
  size_t cap = 0, hcap = 0;
  hipStream_t stream = nullptr;
};

static StandaloneBufs& standalone_bufs(int dev) {
  static std::mutex mu;
  static std::vector<StandaloneBufs*> per_dev;
  std::lock_guard<std::mutex> lock(mu);
  if ((int)per_dev.size() <= dev) per_dev.resize(dev + 1, nullptr);
  if (!per_dev[dev]) per_dev[dev] = new StandaloneBufs();
  return *per_dev[dev];
}

static hipError_t standalone_reserve(StandaloneBufs& b, size_t bytes, size_t host_bytes) {
  hipError_t e = hipSuccess;
  if (!b.stream) e = hipStreamCreateWithFlags(&b.stream, hipStreamNonBlocking);
  if (e == hipSuccess && (bytes > b.cap || !b.buf)) {
    if (b.buf) (void)hipFree(b.buf);
    b.buf = nullptr;
    b.cap = 0;
    e = hipMalloc((void**)&b.buf, bytes);
    if (e == hipSuccess) b.cap = bytes;
  }
  if (e == hipSuccess && (host_bytes > b.hcap || !b.host)) {
    if (b.host) (void)hipHostFree(b.host);
    b.host = nullptr;
    b.hcap = 0;
    e = hipHostMalloc((void**)&b.host, host_bytes);
    if (e == hipSuccess) b.hcap = host_bytes;
  }
  return e;
}

int gpdla_voigt_batch_f64(const double* lambdas, int64_t n_padded, const double* z, const double* N,
                          int64_t count, int32_t num_lines, double* out) {
  if (!lambdas || !z || !N || !out) return set_error(GPDLA_EINVAL, "null argument");
  if (n_padded <= 2 * kWidth) return set_error(GPDLA_EINVAL, "need more than %d wavelengths", 2 * kWidth);
  if (num_lines < 1 || num_lines > kMaxLines) return set_error(GPDLA_EINVAL, "num_lines=%d outside [1, 31]", num_lines);
  if (count < 1) return GPDLA_OK;
  int rc = check_device(0);
  if (rc) return rc;
  double* d_lines = nullptr;
  if ((rc = lines_on_device(&d_lines))) return rc;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  StandaloneBufs& sb = standalone_bufs(dev);
  std::lock_guard<std::mutex> lock(sb.mu);
  const int64_t n_out = n_padded - 2 * kWidth;
  const size_t n_in = (size_t)(n_padded + 2 * count);          // [lambdas | z | N]
  const size_t bytes = (n_in + (size_t)count * n_out) * 8;
  hipError_t err = standalone_reserve(sb, bytes, n_in * 8);
  if (err != hipSuccess) return set_error(GPDLA_EDEVICE, "voigt: %s", hipGetErrorString(err));
  double* h = (double*)sb.host;
  std::memcpy(h, lambdas, n_padded * 8);
  std::memcpy(h + n_padded, z, count * 8);
  std::memcpy(h + n_padded + count, N, count * 8);
  double* d_lam = (double*)sb.buf;
  double* d_z = d_lam + n_padded;
  double* d_N = d_z + count;
  double* d_out = d_N + count;
  err = hipMemcpyAsync(d_lam, h, n_in * 8, hipMemcpyHostToDevice, sb.stream);
  if (err == hipSuccess) err = launch_voigt_batch(d_lam, n_padded, d_z, d_N, count, num_lines, make_line_args(d_lines), d_out, sb.stream);
  // the profiles straight into the caller's buffer (the pinned staging is write-combined: reading
  // it back on the host is slow)
  if (err == hipSuccess) err = hipMemcpyAsync(out, d_out, count * n_out * 8, hipMemcpyDeviceToHost, sb.stream);
  if (err == hipSuccess) err = hipStreamSynchronize(sb.stream);
  if (err != hipSuccess) return set_error(GPDLA_EDEVICE, "voigt: %s", hipGetErrorString(err));
  return GPDLA_OK;
}

int gpdla_diag_raw_profile3(const double* lambdas, int64_t n, double z, double N, int32_t f32, double* out) {
  if (!lambdas || !out) return set_error(GPDLA_EINVAL, "null argument");
  if (n < 1) return GPDLA_OK;
  int rc = check_device(0);
  if (rc) return rc;
  double* d_lines = nullptr;
  if ((rc = lines_on_device(&d_lines))) return rc;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  StandaloneBufs& sb = standalone_bufs(dev);
  std::lock_guard<std::mutex> lock(sb.mu);
  hipError_t err = standalone_reserve(sb, (size_t)n * 16, (size_t)n * 8);
  if (err != hipSuccess) return set_error(GPDLA_EDEVICE, "raw profile: %s", hipGetErrorString(err));
  double* d_lam = (double*)sb.buf;
  double* d_out = d_lam + n;
  std::memcpy(sb.host, lambdas, (size_t)n * 8);
  err = hipMemcpyAsync(d_lam, sb.host, (size_t)n * 8, hipMemcpyHostToDevice, sb.stream);
  if (err == hipSuccess) err = launch_diag_raw_profile(d_lam, n, z, N, f32 ? 1 : 0, make_line_args(d_lines), d_out, sb.stream);
  if (err == hipSuccess) err = hipMemcpyAsync(out, d_out, (size_t)n * 8, hipMemcpyDeviceToHost, sb.stream);
  if (err == hipSuccess) err = hipStreamSynchronize(sb.stream);
  if (err != hipSuccess) return set_error(GPDLA_EDEVICE, "raw profile: %s", hipGetErrorString(err));
  return GPDLA_OK;
}

int gpdla_voigt_f64(const double* lambdas, int64_t n_padded, double z, double N, int32_t num_lines,
                    double* out) {
  return gpdla_voigt_batch_f64(lambdas, n_padded, &z, &N, 1, num_lines, out);
}

int gpdla_log_mvnpdf_low_rank_f64(const double* y, const double* mu, const double* M, const double* d,
                                  int64_t n, int32_t k, double* out) {
  if (!y || !mu || !M || !d || !out) return set_error(GPDLA_EINVAL, "null argument");
  if (n < 1 || k < 1) return set_error(GPDLA_EINVAL, "n=%lld k=%d", (long long)n, k);
  if (k > 64) return set_error(GPDLA_EUNSUPPORTED, "k=%d > 64 in the standalone entry point", k);
  int rc = check_device(0);
  if (rc) return rc;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  StandaloneBufs& sb = standalone_bufs(dev);
  std::lock_guard<std::mutex> lock(sb.mu);
  // one staging copy: [y | mu | d | M | out | status]
  const size_t nin = (size_t)n * (3 + k);
  hipError_t err = standalone_reserve(sb, (nin + 2) * 8, (nin + 2) * 8);
  if (err != hipSuccess) return set_error(GPDLA_EDEVICE, "log_mvnpdf_low_rank: %s", hipGetErrorString(err));
  double* h = (double*)sb.host;
  std::memcpy(h, y, n * 8);
  std::memcpy(h + n, mu, n * 8);
  std::memcpy(h + 2 * n, d, n * 8);
  std::memcpy(h + 3 * n, M, (size_t)n * k * 8);
  double* dy = (double*)sb.buf;
  double* dmu = dy + n;
  double* dd = dmu + n;
  double* dM = dd + n;
  double* dout = dy + nin;
  int32_t* dst = (int32_t*)(dout + 1);
  err = hipMemcpyAsync(dy, h, nin * 8, hipMemcpyHostToDevice, sb.stream);
  if (err == hipSuccess) err = launch_mvn_single(dy, dmu, dM, dd, n, k, dout, dst, sb.stream);
  if (err == hipSuccess) err = hipMemcpyAsync(h + nin, dout, 16, hipMemcpyDeviceToHost, sb.stream);
  if (err == hipSuccess) err = hipStreamSynchronize(sb.stream);
  if (err != hipSuccess) return set_error(GPDLA_EDEVICE, "log_mvnpdf_low_rank: %s", hipGetErrorString(err));
  *out = h[nin];
  int32_t status = 0;
  std::memcpy(&status, h + nin + 1, 4);
  if (status) return set_error(GPDLA_ENUMERIC, "B = I + M'D^-1M is not positive definite");
  return GPDLA_OK;
}

}  // extern "C"
