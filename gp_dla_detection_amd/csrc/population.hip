// Population statistics (include/gpdla.h "Population statistics"): what the
// reference's CDDF_analysis/calc_cddf.py needs from the level-1 sample rows to put intervals on f(N),
// dN/dX and Omega_DLA, reduced while the rows are on the device.
//
//   model_posterior_kernel   one thread per spectrum: p_dla = 1 - p_no (- p_lls) from row_posterior.h's
//                            model_posterior_terms, by process.py's model_posteriors* expression
//   population_split_kernel  _split_distributions_single (calc_cddf.py:724-778) on a (z, log N_HI) grid with
//                            p_j = p_dla pi_j, one 256-thread workgroup per row: row_posterior.h's
//                            split_rows<1, 512, 1>, which fixes the order of operations
//   pmf_chunk_kernel /       the Poisson-binomial pmf of each bin of a CSR list: the coefficients of
//   pmf_fold_kernel          prod_j (1 - p_j + p_j x).  A bin is cut into chunks of kPmfChunk trials in
//                            list order; one workgroup per chunk runs pmf[k] <- pmf[k] (1 - p) + pmf[k-1] p
//                            in LDS, then the chunk polynomials are folded left to right, R <- R * P_c, one
//                            launch per fold step with every coefficient an FMA chain in ascending order
//                            of P_c's index.  All terms are non-negative, so every coefficient carries a
//                            relative error bound; the order depends on the bin's own length alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/gpdla.h"
#include "internal.h"
#include "row_posterior.h"

namespace gpdla {
namespace {

static_assert(kPopulationMaxLarge == GPDLA_POPULATION_MAX_LARGE, "gpdla.h");
static_assert(kPmfChunk == GPDLA_PMF_CHUNK, "gpdla.h");

__global__ __launch_bounds__(kRowThreads) void population_split_kernel(PopulationSplitArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int row = blockIdx.x;
  split_rows<1, kRowTileOne, 1>(a, row, row, a.level_post[row], split_lds(a.r.nz, a.r.nn, kRowTileOne, 1, 1), smem);
}

__global__ __launch_bounds__(kRowThreads) void model_posterior_kernel(ModelPosteriorArgs a) {
#pragma clang fp contract(off)
  const int q = blockIdx.x * kRowThreads + threadIdx.x;
  if (q >= a.rows) return;
  double e[kMaxDlas + 2], sum;
  int n;
  if (!model_posterior_terms(a, q, e, sum, n)) { a.p_dla[q] = NAN; return; }
  const double p_no = e[0] / sum;
  double p = 1.0 - p_no;
  if (a.ll_lls) p = p - e[n - 1] / sum;
  a.p_dla[q] = p;
}

// ---- Poisson-binomial pmf ----------------------------------------------------------------------
// chunk c: trials probs[start .. start + len) of its bin -> len + 1 coefficients at out
__global__ __launch_bounds__(kRowThreads) void pmf_chunk_kernel(PmfChunkArgs a) {
  __shared__ double s_p[kPmfChunk];
  __shared__ double s_c[2][kPmfChunk + 2];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int len = a.len[c];
  const double* p = a.probs + a.start[c];
  for (int i = tid; i < len; i += kRowThreads) s_p[i] = p[i];
  for (int i = tid; i <= kPmfChunk; i += kRowThreads) { s_c[0][i] = i == 0 ? 1.0 : 0.0; s_c[1][i] = 0.0; }
  __syncthreads();
  int cur = 0;
  for (int j = 0; j < len; ++j) {
    const double pj = s_p[j], qj = 1.0 - pj;
    const double* src = s_c[cur];
    double* dst = s_c[cur ^ 1];
    for (int k = tid; k <= j + 1; k += kRowThreads) {
      const double keep = src[k] * qj;                         // src[j + 1] is still 0
      dst[k] = k > 0 ? __builtin_fma(src[k - 1], pj, keep) : keep;
    }
    __syncthreads();
    cur ^= 1;
  }
  double* out = a.dst[c];
  for (int i = tid; i <= len; i += kRowThreads) out[i] = s_c[cur][i];
}

// fold step s of every bin with more than s chunks: next[k] = sum_i P[i] cur[k - i], i ascending, where cur
// holds the product of chunks 0 .. s - 1 (lr + 1 coefficients) and P is chunk s (lp + 1 coefficients)
__global__ __launch_bounds__(kRowThreads) void pmf_fold_kernel(PmfFoldArgs a, int step) {
  __shared__ double s_P[kPmfChunk + 1];
  __shared__ double s_R[kPmfChunk + kRowThreads];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int nch = a.nch[b];
  if (nch <= step) return;
  const int64_t n = a.n[b];
  const int64_t lr = (int64_t)step * kPmfChunk;
  const int lp = (int)min((int64_t)kPmfChunk, n - lr);
  const int64_t k0 = (int64_t)blockIdx.x * kRowThreads;
  if (k0 > lr + lp) return;
  // the bin ends in buffer 0 after its last step: step s reads buffer (nch - s) & 1
  const double* cur = a.buf[(nch - step) & 1] + a.out_off[b];
  double* next = a.buf[(nch - step - 1) & 1] + a.out_off[b];
  const double* P = a.chunks + a.chunk_off[b] + lr + step;     // chunk c starts c kPmfChunk + c entries in
  for (int i = tid; i <= lp; i += kRowThreads) s_P[i] = P[i];
  const int64_t w0 = k0 - lp;                                  // the window cur[w0 .. k0 + 255]
  for (int i = tid; i < lp + kRowThreads; i += kRowThreads) {
    const int64_t r = w0 + i;
    s_R[i] = (r >= 0 && r <= lr) ? cur[r] : 0.0;
  }
  __syncthreads();
  const int64_t k = k0 + tid;
  if (k > lr + lp) return;
  const int i_lo = (int)max((int64_t)0, k - lr), i_hi = (int)min((int64_t)lp, k);
  double acc = 0.0;
  for (int i = i_lo; i <= i_hi; ++i) acc = __builtin_fma(s_P[i], s_R[tid + lp - i], acc);
  next[k] = acc;
}

}  // namespace

hipError_t launch_population_split(const PopulationSplitArgs& a, hipStream_t s) {
  if (a.r.rows < 1) return hipSuccess;
  if (!sample_rows_ok(a.r) || a.r.levels != 1) return hipErrorInvalidValue;
  const RowLds L = split_lds(a.r.nz, a.r.nn, kRowTileOne, 1, 1);
  hipLaunchKernelGGL(population_split_kernel, dim3((unsigned)a.r.rows), dim3(kRowThreads), L.total, s, a);
  return hipGetLastError();
}

hipError_t launch_model_posterior(const ModelPosteriorArgs& a, hipStream_t s) {
  if (a.rows < 1) return hipSuccess;
  if (a.levels < 1 || a.levels > kMaxDlas) return hipErrorInvalidValue;
  hipLaunchKernelGGL(model_posterior_kernel, dim3((unsigned)((a.rows + kRowThreads - 1) / kRowThreads)), dim3(kRowThreads),
                     0, s, a);
  return hipGetLastError();
}

int validate_grid_edges(const char* prefix, int64_t nz, int64_t nn, const double* z_edges, const double* n_edges) {
  for (int ax = 0; ax < 2; ++ax) {
    const double* ed = ax ? n_edges : z_edges;
    const int64_t n = ax ? nn : nz;
    for (int64_t i = 0; i <= n; ++i)
      if (!std::isfinite(ed[i]) || (i > 0 && !(ed[i] > ed[i - 1])))
        return set_error(GPDLA_EINVAL, "%s%s[%lld] = %g: edges must be finite and strictly increasing", prefix,
                         ax ? "log_nhi_edges" : "z_edges", (long long)i, ed[i]);
  }
  return GPDLA_OK;
}

// the thresholds and the grid of a population call (shared with engine.hip)
int validate_population_grid(int64_t nz, int64_t nn, const double* z_edges, const double* n_edges,
                             double p_thresh_sample, double p_switch) {
  if (nz < 1 || nn < 1) return set_error(GPDLA_EINVAL, "population grid %lld x %lld: both bin counts must be positive",
                                         (long long)nz, (long long)nn);
  if (nz * nn > GPDLA_SUMMARY_MAX_BINS)
    return set_error(GPDLA_EINVAL, "population grid %lld x %lld exceeds %d bins", (long long)nz, (long long)nn,
                     GPDLA_SUMMARY_MAX_BINS);
  if (!z_edges || !n_edges) return set_error(GPDLA_EINVAL, "null population edge array");
  if (int rc = validate_grid_edges("population ", nz, nn, z_edges, n_edges)) return rc;
  if (!(p_switch >= 1.0 / GPDLA_POPULATION_MAX_LARGE && p_switch < INFINITY))
    return set_error(GPDLA_EINVAL, "p_switch = %g: must be finite and >= 1/%d (the large list has %d slots)", p_switch,
                     GPDLA_POPULATION_MAX_LARGE, GPDLA_POPULATION_MAX_LARGE);
  if (!(p_thresh_sample >= 0.0 && p_thresh_sample < p_switch))
    return set_error(GPDLA_EINVAL, "p_thresh_sample = %g outside [0, p_switch = %g)", p_thresh_sample, p_switch);
  return GPDLA_OK;
}

int HostSampleRows::check(bool others) const {
  if (!ll || !offset || !log_nhi || !min_z || !max_z || !others) return set_error(GPDLA_EINVAL, "null argument");
  if (rows < 0 || S < 1 || ld < S || rows > INT32_MAX || S > INT32_MAX)
    return set_error(GPDLA_EINVAL, "rows=%lld S=%lld ld=%lld", (long long)rows, (long long)S, (long long)ld);
  if (levels < 1 || levels > GPDLA_MAX_DLAS) return set_error(GPDLA_EINVAL, "levels=%d outside 1..%d", levels, GPDLA_MAX_DLAS);
  if (levels > 1 && !base) return set_error(GPDLA_EINVAL, "levels=%d needs base_inds", levels);
  return GPDLA_OK;
}

void HostSampleRows::carve(DeviceStage& st) {
  const size_t R = (size_t)rows, LV = (size_t)levels;
  o_ll = st.carve(LV * R * ld * 8); o_base = st.carve((LV - 1) * R * ld * 4);
  o_off = st.carve((size_t)S * 8); o_ln = st.carve((size_t)S * 8); o_nh = st.carve(nhi ? (size_t)S * 8 : 0);
  o_zmin = st.carve(R * 8); o_zmax = st.carve(R * 8); o_ed = st.carve((size_t)(nz + nn + 2) * 8);
}

hipError_t HostSampleRows::upload(DeviceStage& st, SampleRowsArgs* r, const double** d_nhi) const {
  const size_t R = (size_t)rows, LV = (size_t)levels;
  const struct { size_t o; const void* src; size_t bytes; } copies[] = {
      {o_ll, ll, LV * R * ld * 8}, {o_base, base, (LV - 1) * R * ld * 4}, {o_off, offset, (size_t)S * 8},
      {o_ln, log_nhi, (size_t)S * 8}, {o_nh, nhi, nhi ? (size_t)S * 8 : 0}, {o_zmin, min_z, R * 8}, {o_zmax, max_z, R * 8},
      {o_ed, z_edges, nz ? (size_t)(nz + 1) * 8 : 0}, {o_ed + (size_t)(nz + 1) * 8, n_edges, nz ? (size_t)(nn + 1) * 8 : 0}};
  for (const auto& c : copies)
    if (c.bytes)
      if (hipError_t e = st.upload(c.o, c.src, c.bytes)) return e;
  *r = SampleRowsArgs{};
  r->rows = (int32_t)rows; r->levels = levels; r->ll = st.ptr<const double>(o_ll); r->ld = ld; r->S = S;
  r->base = levels > 1 ? st.ptr<const int32_t>(o_base) : nullptr; r->ld_base = ld;
  r->offset = st.ptr<const double>(o_off); r->log_nhi = st.ptr<const double>(o_ln);
  r->zmin = st.ptr<const double>(o_zmin); r->zmax = st.ptr<const double>(o_zmax);
  r->nz = nz; r->nn = nn; r->z_edges = st.ptr<const double>(o_ed); r->n_edges = st.ptr<const double>(o_ed) + nz + 1;
  if (d_nhi) *d_nhi = st.ptr<const double>(o_nh);
  return hipSuccess;
}

}  // namespace gpdla

using namespace gpdla;

extern "C" {

int gpdla_population_split_f64(int32_t device, const double* ll, int64_t rows, int64_t S, int64_t ld,
                               const double* offset_samples, const double* log_nhi_samples, const double* min_z,
                               const double* max_z, const double* p_dlas, const gpdla_population_spec* spec,
                               double* poisson_plane, int32_t* large_inds, double* large_probs, int32_t* large_bins) {
  HostSampleRows h{ll, rows, S, ld, offset_samples, log_nhi_samples, nullptr, min_z, max_z, nullptr, 1};
  int rc = h.check(p_dlas && spec && poisson_plane && large_inds && large_probs && large_bins);
  if (rc) return rc;
  if ((rc = validate_population_grid(spec->num_z_bins, spec->num_nhi_bins, spec->z_edges, spec->log_nhi_edges,
                                     spec->p_thresh_sample, spec->p_switch)))
    return rc;
  for (int64_t q = 0; q < rows; ++q)
    if (p_dlas[q] == p_dlas[q] && !(p_dlas[q] >= 0.0 && p_dlas[q] <= 1.0))
      return set_error(GPDLA_EINVAL, "p_dlas[%lld] = %g outside [0, 1]", (long long)q, p_dlas[q]);
  if ((rc = check_device(device))) return rc;
  if (rows == 0) return GPDLA_OK;
  HIP_TRY(hipSetDevice(device));
  h.nz = spec->num_z_bins; h.nn = spec->num_nhi_bins; h.z_edges = spec->z_edges; h.n_edges = spec->log_nhi_edges;
  const size_t R = (size_t)rows, nbins = (size_t)h.nz * h.nn, NL = GPDLA_POPULATION_MAX_LARGE;
  DeviceStage st;
  h.carve(st);
  const size_t o_p = st.carve(R * 8), o_pl = st.carve(R * nbins * 8), o_li = st.carve(R * NL * 4);
  const size_t o_lp = st.carve(R * NL * 8), o_lb = st.carve(R * NL * 4);
  PopulationSplitArgs pa{};
  HIP_TRY_IN("population", st.alloc());
  HIP_TRY_IN("population", h.upload(st, &pa.r, nullptr));
  HIP_TRY_IN("population", st.upload(o_p, p_dlas, R * 8));
  pa.level_post = st.ptr<const double>(o_p); pa.ld_post = rows;
  pa.p_thresh_sample = spec->p_thresh_sample; pa.p_switch = spec->p_switch;
  pa.poisson = st.ptr<double>(o_pl); pa.large_inds = st.ptr<int32_t>(o_li); pa.large_probs = st.ptr<double>(o_lp);
  pa.large_bins = st.ptr<int32_t>(o_lb);
  HIP_TRY_IN("population", launch_population_split(pa, nullptr));
  HIP_TRY_IN("population", st.download(poisson_plane, o_pl, R * nbins * 8));
  HIP_TRY_IN("population", st.download(large_inds, o_li, R * NL * 4));
  HIP_TRY_IN("population", st.download(large_probs, o_lp, R * NL * 8));
  HIP_TRY_IN("population", st.download(large_bins, o_lb, R * NL * 4));
  return GPDLA_OK;
}

int gpdla_poisson_binomial_pmf_f64(int32_t device, const double* probs, const int64_t* offsets, int64_t num_bins,
                                   double* pmf) {
  if (!offsets || !pmf || num_bins < 0) return set_error(GPDLA_EINVAL, "null argument or num_bins < 0");
  if (num_bins > INT32_MAX / 2) return set_error(GPDLA_EINVAL, "num_bins=%lld", (long long)num_bins);
  if (offsets[0] != 0) return set_error(GPDLA_EINVAL, "offsets[0] = %lld: must be 0", (long long)offsets[0]);
  for (int64_t b = 0; b < num_bins; ++b) {
    const int64_t n = offsets[b + 1] - offsets[b];
    if (n < 0 || n > GPDLA_PMF_MAX_TRIALS)
      return set_error(GPDLA_EINVAL, "bin %lld holds %lld trials (0..%d)", (long long)b, (long long)n, GPDLA_PMF_MAX_TRIALS);
  }
  const int64_t total = num_bins ? offsets[num_bins] : 0;
  if (total > 0 && !probs) return set_error(GPDLA_EINVAL, "null probs");
  for (int64_t i = 0; i < total; ++i)
    if (!(probs[i] >= 0.0 && probs[i] <= 1.0))
      return set_error(GPDLA_EINVAL, "probs[%lld] = %g outside [0, 1]", (long long)i, probs[i]);
  int rc = check_device(device);
  if (rc) return rc;
  LaunchTimes& lt = launch_times();
  lt.reset();
  if (num_bins == 0) return GPDLA_OK;
  HIP_TRY(hipSetDevice(device));
  // chunks in bin order; the multi-chunk bins get an entry in the fold tables
  const size_t NB = (size_t)num_bins, out_total = (size_t)total + NB;
  std::vector<int64_t> c_start;
  std::vector<int32_t> c_len, c_bin, c_local;
  std::vector<int64_t> f_n, f_out, f_chunk;
  std::vector<int32_t> f_nch;
  int max_nch = 1;
  int64_t max_n = 0, chunk_entries = 0;
  for (size_t b = 0; b < NB; ++b) {
    const int64_t n = offsets[b + 1] - offsets[b];
    const int nch = (int)std::max<int64_t>(1, (n + kPmfChunk - 1) / kPmfChunk);
    if (nch > 1) {
      f_n.push_back(n); f_out.push_back(offsets[b] + (int64_t)b); f_chunk.push_back(chunk_entries); f_nch.push_back(nch);
      max_nch = std::max(max_nch, nch);
      max_n = std::max(max_n, n);
    }
    for (int c = 0; c < nch; ++c) {
      c_start.push_back(offsets[b] + (int64_t)c * kPmfChunk);
      c_len.push_back((int32_t)std::min<int64_t>(kPmfChunk, n - (int64_t)c * kPmfChunk));
      c_bin.push_back((int32_t)b); c_local.push_back(c);
    }
    if (nch > 1) chunk_entries += n + nch;   // chunks 1.. are read from here (chunk 0's slot stays unused)
  }
  const size_t NC = c_len.size(), NF = f_n.size();
  if (NF > 65535) return set_error(GPDLA_EINVAL, "%lld bins beyond %d trials in one call (at most 65535)", (long long)NF, kPmfChunk);
  DeviceStage st;
  const size_t o_probs = st.carve((size_t)total * 8), o_buf0 = st.carve(out_total * 8), o_buf1 = st.carve(NF ? out_total * 8 : 0);
  const size_t o_chunks = st.carve((size_t)chunk_entries * 8), o_cs = st.carve(NC * 8), o_cl = st.carve(NC * 4);
  const size_t o_cd = st.carve(NC * 8), o_fn = st.carve(NF * 8), o_fo = st.carve(NF * 8), o_fc = st.carve(NF * 8);
  const size_t o_fh = st.carve(NF * 4);
  HIP_TRY_IN("population", st.alloc());
  double* bufs[2] = {st.ptr<double>(o_buf0), st.ptr<double>(o_buf1)};
  double* chunks = st.ptr<double>(o_chunks);
  // where each chunk's polynomial goes: a single-chunk bin's straight to the output; chunk 0 of a longer
  // bin to the buffer its fold starts from; the others to the chunk store
  std::vector<double*> c_dst(NC);
  {
    size_t f = 0;
    for (size_t c = 0; c < NC; ++c) {
      const size_t b = (size_t)c_bin[c];
      const int64_t n = offsets[b + 1] - offsets[b];
      const int nch = (int)std::max<int64_t>(1, (n + kPmfChunk - 1) / kPmfChunk);
      if (nch == 1) { c_dst[c] = bufs[0] + offsets[b] + (int64_t)b; continue; }
      if (c_local[c] == 0) c_dst[c] = bufs[(nch - 1) & 1] + f_out[f];
      else c_dst[c] = chunks + f_chunk[f] + (int64_t)c_local[c] * kPmfChunk + c_local[c];
      if (c_local[c] == nch - 1) ++f;
    }
  }
  if (total) HIP_TRY_IN("population", st.upload(o_probs, probs, (size_t)total * 8));
  HIP_TRY_IN("population", st.upload(o_cs, c_start.data(), NC * 8));
  HIP_TRY_IN("population", st.upload(o_cl, c_len.data(), NC * 4));
  HIP_TRY_IN("population", st.upload(o_cd, c_dst.data(), NC * 8));
  PmfChunkArgs ca{};
  ca.probs = st.ptr<const double>(o_probs); ca.start = st.ptr<const int64_t>(o_cs); ca.len = st.ptr<const int32_t>(o_cl);
  ca.dst = st.ptr<double* const>(o_cd);
  lt.before();
  hipLaunchKernelGGL(pmf_chunk_kernel, dim3((unsigned)NC), dim3(kRowThreads), 0, nullptr, ca);
  HIP_TRY_IN("population", hipGetLastError());
  lt.after();
  if (NF) {
    HIP_TRY_IN("population", st.upload(o_fn, f_n.data(), NF * 8));
    HIP_TRY_IN("population", st.upload(o_fo, f_out.data(), NF * 8));
    HIP_TRY_IN("population", st.upload(o_fc, f_chunk.data(), NF * 8));
    HIP_TRY_IN("population", st.upload(o_fh, f_nch.data(), NF * 4));
    PmfFoldArgs fa{};
    fa.n = st.ptr<const int64_t>(o_fn); fa.out_off = st.ptr<const int64_t>(o_fo); fa.chunk_off = st.ptr<const int64_t>(o_fc);
    fa.nch = st.ptr<const int32_t>(o_fh); fa.chunks = chunks; fa.buf[0] = bufs[0]; fa.buf[1] = bufs[1];
    lt.before();
    for (int s = 1; s < max_nch; ++s) {
      const int64_t len = std::min<int64_t>(max_n, (int64_t)(s + 1) * kPmfChunk) + 1;
      hipLaunchKernelGGL(pmf_fold_kernel, dim3((unsigned)((len + kRowThreads - 1) / kRowThreads), (unsigned)NF),
                         dim3(kRowThreads), 0, nullptr, fa, s);
      HIP_TRY_IN("population", hipGetLastError());
    }
    lt.after();
  }
  HIP_TRY_IN("population", st.download(pmf, o_buf0, out_total * 8));
  lt.finish();
  return GPDLA_OK;
}

}  // extern "C"
