// Population statistics over every multi-DLA level (include/gpdla.h "Population statistics over every
// multi-DLA level"): what posterior_summary.hip's bin planes and population.hip's
// split reduce from the level-1 rows, for every level of a max_dlas = D run and with every absorber a
// sample carries -- its own and those of its base chain -- counted.
//
//   level_posterior_kernel  one thread per spectrum: P_d, the posterior of "exactly d DLAs", from the terms
//                           model_posterior_kernel derives p_dla from (row_posterior.h)
//   level_planes_kernel     one 256-thread workgroup per (row, level): planes_rows<NS, 256>
//   level_split_kernel      the same shape on the population grid with p = P_d pi_{d,j}: split_rows<NS, 256,
//                           kMaxDlas>
// The bodies are row_posterior.h's, which the level-1 kernels instantiate with one slot and a tile of 512: a
// bin's sum is the sequential sum in (sample index, slot) order at either tile size, so level 1 here is
// posterior_summary_kernel's planes and population_split_kernel's split bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/gpdla.h"
#include "internal.h"
#include "row_posterior.h"

namespace gpdla {
namespace {

static_assert(kMaxDlas == GPDLA_MAX_DLAS && kMaxDlas == 4, "the kernels dispatch on 1..4 slots");

template <int NS>
__device__ __forceinline__ void level_planes_body(const LevelPlanesArgs& a, char* smem) {
  const SampleRowsArgs& r = a.r;
  const int row = blockIdx.x;
  const RowLds L = planes_lds(r.nz, r.nn, kRowTileLevels, r.levels);
  const double* ll = r.ll + ((int64_t)(NS - 1) * r.rows + row) * r.ld;
  const double m = row_first_max(ll, (int32_t)r.S, threadIdx.x, (double*)(smem + L.red_v), (int32_t*)(smem + L.red_i)).v;
  planes_rows<NS, kRowTileLevels>(r, a.nhi, row, ll, m, L, smem,
                                  a.planes + ((int64_t)row * r.levels + (NS - 1)) * kSummaryPlanes * r.nz * r.nn);
}

__global__ __launch_bounds__(kRowThreads) void level_planes_kernel(LevelPlanesArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  switch (blockIdx.y) {   // uniform over the workgroup
    case 0: level_planes_body<1>(a, smem); break;
    case 1: level_planes_body<2>(a, smem); break;
    case 2: level_planes_body<3>(a, smem); break;
    default: level_planes_body<4>(a, smem); break;
  }
}

template <int NS>
__device__ __forceinline__ void level_split_body(const LevelSplitArgs& a, char* smem) {
  const int row = blockIdx.x;
  split_rows<NS, kRowTileLevels, kMaxDlas>(a, row, (int64_t)row * a.r.levels + (NS - 1), a.level_post[(int64_t)(NS - 1) * a.ld_post + row],
                                           split_lds(a.r.nz, a.r.nn, kRowTileLevels, a.r.levels, kMaxDlas), smem);
}

__global__ __launch_bounds__(kRowThreads) void level_split_kernel(LevelSplitArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  switch (blockIdx.y) {   // uniform over the workgroup
    case 0: level_split_body<1>(a, smem); break;
    case 1: level_split_body<2>(a, smem); break;
    case 2: level_split_body<3>(a, smem); break;
    default: level_split_body<4>(a, smem); break;
  }
}

__global__ __launch_bounds__(kRowThreads) void level_posterior_kernel(ModelPosteriorArgs a) {
#pragma clang fp contract(off)
  const int q = blockIdx.x * kRowThreads + threadIdx.x;
  if (q >= a.rows) return;
  double e[kMaxDlas + 2], sum;
  int n;
  if (!model_posterior_terms(a, q, e, sum, n)) {
    for (int d = 0; d < a.levels; ++d) a.level_post[(int64_t)d * a.rows + q] = NAN;
    return;
  }
  for (int d = 0; d < a.levels; ++d) a.level_post[(int64_t)d * a.rows + q] = e[1 + d] / sum;
}

}  // namespace

hipError_t launch_level_posterior(const ModelPosteriorArgs& a, hipStream_t s) {
  if (a.rows < 1) return hipSuccess;
  if (a.levels < 1 || a.levels > kMaxDlas) return hipErrorInvalidValue;
  hipLaunchKernelGGL(level_posterior_kernel, dim3((unsigned)((a.rows + kRowThreads - 1) / kRowThreads)),
                     dim3(kRowThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_level_planes(const LevelPlanesArgs& a, hipStream_t s) {
  if (a.r.rows < 1) return hipSuccess;
  if (!sample_rows_ok(a.r)) return hipErrorInvalidValue;
  const RowLds L = planes_lds(a.r.nz, a.r.nn, kRowTileLevels, a.r.levels);
  hipLaunchKernelGGL(level_planes_kernel, dim3((unsigned)a.r.rows, (unsigned)a.r.levels), dim3(kRowThreads), L.total,
                     s, a);
  return hipGetLastError();
}

hipError_t launch_level_split(const LevelSplitArgs& a, hipStream_t s) {
  if (a.r.rows < 1) return hipSuccess;
  if (!sample_rows_ok(a.r)) return hipErrorInvalidValue;
  const RowLds L = split_lds(a.r.nz, a.r.nn, kRowTileLevels, a.r.levels, kMaxDlas);
  hipLaunchKernelGGL(level_split_kernel, dim3((unsigned)a.r.rows, (unsigned)a.r.levels), dim3(kRowThreads), L.total,
                     s, a);
  return hipGetLastError();
}

// The host arrays of gpdla_sample_cuts behind the cut fields of SampleRowsArgs: check() before the device is
// touched, carve() before alloc(), upload() after HostSampleRows::upload (which clears the fields)
struct HostSampleCuts {
  const gpdla_sample_cuts* c;
  int64_t rows;
  size_t o_zu = 0, o_np = 0, o_wo = 0, o_w = 0;
  int check() const {
    if (!c) return GPDLA_OK;
    if (!c->z_uppers && !c->pixel_counts) return set_error(GPDLA_EINVAL, "cuts: neither test is on");
    if (!c->pixel_counts) return GPDLA_OK;
    if (!c->bitmap_offsets || (c->bitmap_offsets[rows] > 0 && !c->bitmap_words) || c->bitmap_offsets[0] != 0)
      return set_error(GPDLA_EINVAL, "cuts: pixel_counts needs the bitmap, its offsets starting at 0");
    for (int64_t r = 0; r < rows; ++r) {
      const int64_t w = c->bitmap_offsets[r + 1] - c->bitmap_offsets[r];
      if (w < 0 || w > INT32_MAX / 32 || c->pixel_counts[r] < 0 || c->pixel_counts[r] > 32 * w)
        return set_error(GPDLA_EINVAL, "cuts: row %lld has %d pixels in %lld bitmap words", (long long)r, c->pixel_counts[r],
                         (long long)w);
    }
    return GPDLA_OK;
  }
  void carve(DeviceStage& st) {
    if (!c) return;
    const size_t R = (size_t)rows;
    o_zu = st.carve(c->z_uppers ? R * 8 : 0);
    if (c->pixel_counts) { o_np = st.carve(R * 4); o_wo = st.carve((R + 1) * 8); o_w = st.carve((size_t)c->bitmap_offsets[rows] * 4); }
  }
  hipError_t upload(DeviceStage& st, SampleRowsArgs* r) const {
    if (!c) return hipSuccess;
    const size_t R = (size_t)rows;
    if (c->z_uppers) {
      if (hipError_t e = st.upload(o_zu, c->z_uppers, R * 8)) return e;
      r->cut_z_upper = st.ptr<const double>(o_zu);
    }
    if (c->pixel_counts) {
      const size_t NW = (size_t)c->bitmap_offsets[rows];
      if (hipError_t e = st.upload(o_np, c->pixel_counts, R * 4)) return e;
      if (hipError_t e = st.upload(o_wo, c->bitmap_offsets, (R + 1) * 8)) return e;
      if (NW)
        if (hipError_t e = st.upload(o_w, c->bitmap_words, NW * 4)) return e;
      r->cut_npix = st.ptr<const int32_t>(o_np); r->cut_word_off = st.ptr<const int64_t>(o_wo);
      r->cut_words = st.ptr<const uint32_t>(o_w);
    }
    return hipSuccess;
  }
};

}  // namespace gpdla

using namespace gpdla;


static int level_planes_host(int32_t device, const double* ll, int64_t rows, int64_t S, int64_t ld,
                             const double* offset_samples, const double* log_nhi_samples, const double* nhi_samples,
                             const double* min_z, const double* max_z, const int32_t* base_inds, int32_t levels,
                             const gpdla_summary_spec* spec, const gpdla_sample_cuts* cuts, double* bin_planes) {
  HostSampleRows h{ll, rows, S, ld, offset_samples, log_nhi_samples, nhi_samples, min_z, max_z, base_inds, levels};
  int rc = h.check(true);
  if (rc) return rc;
  HostSampleCuts hc{cuts, rows};
  if ((rc = hc.check())) return rc;
  if (!nhi_samples || !spec || !bin_planes) return set_error(GPDLA_EINVAL, "null argument");
  // the edge rules of both grids are the same; the thresholds here are placeholders that always pass
  if ((rc = validate_population_grid(spec->num_z_bins, spec->num_nhi_bins, spec->z_edges, spec->log_nhi_edges, 0.0, 1.0)))
    return rc;
  if ((rc = check_device(device))) return rc;
  if (rows == 0) return GPDLA_OK;
  HIP_TRY(hipSetDevice(device));
  h.nz = spec->num_z_bins; h.nn = spec->num_nhi_bins; h.z_edges = spec->z_edges; h.n_edges = spec->log_nhi_edges;
  const size_t planes_bytes = (size_t)rows * levels * kSummaryPlanes * h.nz * h.nn * 8;
  DeviceStage st;
  h.carve(st);
  hc.carve(st);
  const size_t o_pl = st.carve(planes_bytes);
  LevelPlanesArgs a{};
  HIP_TRY_IN("level population", st.alloc());
  HIP_TRY_IN("level population", h.upload(st, &a.r, &a.nhi));
  HIP_TRY_IN("level population", hc.upload(st, &a.r));
  a.planes = st.ptr<double>(o_pl);
  HIP_TRY_IN("level population", launch_level_planes(a, nullptr));
  HIP_TRY_IN("level population", st.download(bin_planes, o_pl, planes_bytes));
  return GPDLA_OK;
}

static int level_split_host(int32_t device, const double* ll, int64_t rows, int64_t S, int64_t ld,
                            const double* offset_samples, const double* log_nhi_samples,
                            const double* min_z, const double* max_z, const int32_t* base_inds,
                            int32_t levels, const double* level_posteriors,
                            const gpdla_population_spec* spec, const gpdla_sample_cuts* cuts, double* poisson_plane,
                            int32_t* large_inds, double* large_probs, int32_t* large_bins) {
  HostSampleRows h{ll, rows, S, ld, offset_samples, log_nhi_samples, nullptr, min_z, max_z, base_inds, levels};
  int rc = h.check(true);
  if (rc) return rc;
  HostSampleCuts hc{cuts, rows};
  if ((rc = hc.check())) return rc;
  if (!level_posteriors || !spec || !poisson_plane || !large_inds || !large_probs || !large_bins)
    return set_error(GPDLA_EINVAL, "null argument");
  if ((rc = validate_population_grid(spec->num_z_bins, spec->num_nhi_bins, spec->z_edges, spec->log_nhi_edges,
                                     spec->p_thresh_sample, spec->p_switch)))
    return rc;
  for (int64_t i = 0; i < (int64_t)levels * rows; ++i) {
    const double P = level_posteriors[i];
    if (P == P && !(P >= 0.0 && P <= 1.0))
      return set_error(GPDLA_EINVAL, "level_posteriors[%lld] = %g outside [0, 1]", (long long)i, P);
  }
  if ((rc = check_device(device))) return rc;
  if (rows == 0) return GPDLA_OK;
  HIP_TRY(hipSetDevice(device));
  h.nz = spec->num_z_bins; h.nn = spec->num_nhi_bins; h.z_edges = spec->z_edges; h.n_edges = spec->log_nhi_edges;
  const size_t RL = (size_t)rows * levels, nbins = (size_t)h.nz * h.nn, NL = GPDLA_POPULATION_MAX_LARGE;
  DeviceStage st;
  h.carve(st);
  hc.carve(st);
  const size_t o_P = st.carve(RL * 8), o_pl = st.carve(RL * nbins * 8), o_li = st.carve(RL * NL * 4);
  const size_t o_lp = st.carve(RL * NL * 8), o_lb = st.carve(RL * NL * kMaxDlas * 4);
  LevelSplitArgs a{};
  HIP_TRY_IN("level population", st.alloc());
  HIP_TRY_IN("level population", h.upload(st, &a.r, nullptr));
  HIP_TRY_IN("level population", hc.upload(st, &a.r));
  HIP_TRY_IN("level population", st.upload(o_P, level_posteriors, RL * 8));
  a.level_post = st.ptr<const double>(o_P); a.ld_post = rows;
  a.p_thresh_sample = spec->p_thresh_sample; a.p_switch = spec->p_switch;
  a.poisson = st.ptr<double>(o_pl); a.large_inds = st.ptr<int32_t>(o_li); a.large_probs = st.ptr<double>(o_lp);
  a.large_bins = st.ptr<int32_t>(o_lb);
  HIP_TRY_IN("level population", launch_level_split(a, nullptr));
  HIP_TRY_IN("level population", st.download(poisson_plane, o_pl, RL * nbins * 8));
  HIP_TRY_IN("level population", st.download(large_inds, o_li, RL * NL * 4));
  HIP_TRY_IN("level population", st.download(large_probs, o_lp, RL * NL * 8));
  HIP_TRY_IN("level population", st.download(large_bins, o_lb, RL * NL * kMaxDlas * 4));
  return GPDLA_OK;
}

extern "C" {

int gpdla_level_planes_f64(int32_t device, const double* ll, int64_t rows, int64_t S, int64_t ld,
                           const double* offset_samples, const double* log_nhi_samples, const double* nhi_samples,
                           const double* min_z, const double* max_z, const int32_t* base_inds, int32_t levels,
                           const gpdla_summary_spec* spec, double* bin_planes) {
  return level_planes_host(device, ll, rows, S, ld, offset_samples, log_nhi_samples, nhi_samples, min_z, max_z, base_inds,
                           levels, spec, nullptr, bin_planes);
}

int gpdla_level_planes_cut_f64(int32_t device, const double* ll, int64_t rows, int64_t S, int64_t ld,
                               const double* offset_samples, const double* log_nhi_samples, const double* nhi_samples,
                               const double* min_z, const double* max_z, const int32_t* base_inds, int32_t levels,
                               const gpdla_summary_spec* spec, const gpdla_sample_cuts* cuts, double* bin_planes) {
  return level_planes_host(device, ll, rows, S, ld, offset_samples, log_nhi_samples, nhi_samples, min_z, max_z, base_inds,
                           levels, spec, cuts, bin_planes);
}

int gpdla_population_split_levels_f64(int32_t device, const double* ll, int64_t rows, int64_t S, int64_t ld,
                                      const double* offset_samples, const double* log_nhi_samples,
                                      const double* min_z, const double* max_z, const int32_t* base_inds,
                                      int32_t levels, const double* level_posteriors,
                                      const gpdla_population_spec* spec, double* poisson_plane,
                                      int32_t* large_inds, double* large_probs, int32_t* large_bins) {
  return level_split_host(device, ll, rows, S, ld, offset_samples, log_nhi_samples, min_z, max_z, base_inds, levels,
                          level_posteriors, spec, nullptr, poisson_plane, large_inds, large_probs, large_bins);
}

int gpdla_population_split_levels_cut_f64(int32_t device, const double* ll, int64_t rows, int64_t S, int64_t ld,
                                          const double* offset_samples, const double* log_nhi_samples,
                                          const double* min_z, const double* max_z, const int32_t* base_inds,
                                          int32_t levels, const double* level_posteriors,
                                          const gpdla_population_spec* spec, const gpdla_sample_cuts* cuts,
                                          double* poisson_plane, int32_t* large_inds, double* large_probs,
                                          int32_t* large_bins) {
  return level_split_host(device, ll, rows, S, ld, offset_samples, log_nhi_samples, min_z, max_z, base_inds, levels,
                          level_posteriors, spec, cuts, poisson_plane, large_inds, large_probs, large_bins);
}

}  // extern "C"
