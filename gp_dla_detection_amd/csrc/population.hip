// Population statistics (include/gpdla.h "Population statistics"): what the
// reference's CDDF_analysis/calc_cddf.py needs from the level-1 sample rows to put intervals on f(N),
// dN/dX and Omega_DLA, reduced while the rows are on the device.
//
//   model_posterior_kernel   one thread per spectrum: the log posteriors of the 1 + D (+ 1) models and
//                            p_dla = 1 - p_no (- p_lls), by process.py's model_posteriors* expression
//   population_split_kernel  _split_distributions_single (calc_cddf.py:724-778) on a (z, log N_HI) grid,
//                            one 256-thread workgroup per row.  pi_j is formed as posterior_summary.hip
//                            forms it (the same strided partial sums and the same trees), p_j = p_dla pi_j.
//                            The Poisson plane goes through LDS in tiles exactly like the bin planes
//                            there: bin b belongs to thread b mod 256, which adds its samples in index
//                            order.  The few samples with p_j >= p_switch are collected through an LDS
//                            integer counter and then sorted by sample index, so their order does not
//                            depend on arrival.  No floating-point atomics anywhere.
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
#include "sample_bins.h"

namespace gpdla {
namespace {

constexpr int kPopThreads = 256;
constexpr int kPopWaves = kPopThreads / 64;
constexpr int kPopTile = 512;        // samples staged per pass (12 B each)
constexpr int kPopCandidates = 16;   // LDS slots for p_j >= p_switch; the kPopulationMaxLarge lowest indices are kept

static_assert(kPopulationMaxLarge == GPDLA_POPULATION_MAX_LARGE, "gpdla.h");
static_assert(kPmfChunk == GPDLA_PMF_CHUNK, "gpdla.h");
static_assert(kPopTile % 4 == 0, "the scan reads four bin indices at a time");

__host__ __device__ inline size_t pop_up16(size_t x) { return (x + 15) & ~(size_t)15; }
struct PopLds {
  size_t red_v, red_i, edges_z, edges_n, plane, p, bin, cand_i, cand_p, cand_b, count, total;
};
__host__ __device__ inline PopLds pop_lds(int nz, int nn) {
  PopLds l{};
  size_t o = 0;
  l.red_v = o; o = pop_up16(o + kPopWaves * 8);
  l.red_i = o; o = pop_up16(o + kPopWaves * 4);
  l.edges_z = o; o = pop_up16(o + (size_t)(nz + 1) * 8);
  l.edges_n = o; o = pop_up16(o + (size_t)(nn + 1) * 8);
  l.plane = o; o = pop_up16(o + (size_t)nz * nn * 8);
  l.p = o; o = pop_up16(o + (size_t)kPopTile * 8);
  l.bin = o; o = pop_up16(o + (size_t)kPopTile * 4);
  l.cand_p = o; o = pop_up16(o + (size_t)kPopCandidates * 8);
  l.cand_i = o; o = pop_up16(o + (size_t)kPopCandidates * 4);
  l.cand_b = o; o = pop_up16(o + (size_t)kPopCandidates * 4);
  l.count = o; o = pop_up16(o + 4);
  l.total = o;
  return l;
}

__global__ __launch_bounds__(kPopThreads) void population_split_kernel(PopulationSplitArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int row = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const PopLds L = pop_lds(a.nz, a.nn);
  double* s_rv = (double*)(smem + L.red_v);
  int32_t* s_ri = (int32_t*)(smem + L.red_i);
  const int32_t S = (int32_t)a.S;
  const double* ll = a.ll + (int64_t)row * a.ld;

  // ---- the maximum over the non-NaN entries (posterior_summary.hip's MAP reduction)
  double bv = 0.0;
  int32_t bi = -1;
  for (int64_t j = tid; j < S; j += kPopThreads) {
    const double v = ll[j];
    if (v == v && (bi < 0 || v > bv)) { bv = v; bi = (int32_t)j; }
  }
  auto merge = [](double& v, int32_t& i, double ov, int32_t oi) {
    if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) { v = ov; i = oi; }
  };
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o);
    const int32_t oi = __shfl_xor(bi, o);
    merge(bv, bi, ov, oi);
  }
  if (lane == 0) { s_rv[wave] = bv; s_ri[wave] = bi; }
  __syncthreads();
  bv = s_rv[0]; bi = s_ri[0];
#pragma unroll
  for (int w = 1; w < kPopWaves; ++w) merge(bv, bi, s_rv[w], s_ri[w]);
  __syncthreads();

  // ---- W = sum_j exp(l_j - max), NaN -> 0: the same partial sums and trees as the bin planes' W
  const double m = bv;
  double loc = 0.0;
  for (int64_t j = tid; j < S; j += kPopThreads) {
    const double v = ll[j];
    loc += (v == v) ? exp(v - m) : 0.0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) loc += __shfl_xor(loc, o);
  if (lane == 0) s_rv[wave] = loc;
  __syncthreads();
  double W = s_rv[0];
#pragma unroll
  for (int w = 1; w < kPopWaves; ++w) W += s_rv[w];
  const bool usable = W > 0.0 && W < INFINITY;

  double* s_ez = (double*)(smem + L.edges_z);
  double* s_en = (double*)(smem + L.edges_n);
  double* s_pl = (double*)(smem + L.plane);
  double* s_p = (double*)(smem + L.p);
  int32_t* s_bin = (int32_t*)(smem + L.bin);
  double* s_cp = (double*)(smem + L.cand_p);
  int32_t* s_ci = (int32_t*)(smem + L.cand_i);
  int32_t* s_cb = (int32_t*)(smem + L.cand_b);
  int32_t* s_cnt = (int32_t*)(smem + L.count);
  const int nb = a.nz * a.nn;
  for (int i = tid; i <= a.nz; i += kPopThreads) s_ez[i] = a.z_edges[i];
  for (int i = tid; i <= a.nn; i += kPopThreads) s_en[i] = a.n_edges[i];
  for (int i = tid; i < nb; i += kPopThreads) s_pl[i] = 0.0;
  if (tid == 0) *s_cnt = 0;
  const double zmin = a.zmin[row], zmax = a.zmax[row], p_dla = a.p_dla[row];
  for (int64_t t0 = 0; t0 < S; t0 += kPopTile) {
    __syncthreads();   // edges, zeroed plane and counter ready; the previous tile's scan is over
    for (int i = tid; i < kPopTile; i += kPopThreads) {
      const int64_t j = t0 + i;
      int32_t b = -1;
      double p = 0.0;
      if (j < S) {
        const double v = ll[j];
        const double w = (v == v) ? exp(v - m) : 0.0;
        const double pi = usable ? w / W : 0.0;
        p = p_dla * pi;
        const int iz = find_bin(s_ez, a.nz, sample_z(zmin, zmax, a.offset[j]));
        const int in = find_bin(s_en, a.nn, a.log_nhi[j]);
        if (iz >= 0 && in >= 0) b = iz * a.nn + in;
        if (b >= 0 && p >= a.p_switch) {          // kept exactly; never enters the Poisson plane
          const int slot = atomicAdd(s_cnt, 1);   // integer, LDS: the order is fixed by the sort below
          if (slot < kPopCandidates) { s_cp[slot] = p; s_ci[slot] = (int32_t)j; s_cb[slot] = b; }
          b = -1;
        } else if (!(p > a.p_thresh_sample && p < a.p_switch)) {
          b = -1;                                 // below the sample threshold, or NaN
        }
      }
      s_p[i] = p; s_bin[i] = b;
    }
    __syncthreads();
    const int cnt = (int)min((int64_t)kPopTile, S - t0);
    for (int i0 = 0; i0 < cnt; i0 += 4) {
      const int4 b4 = *(const int4*)(s_bin + i0);   // the same address in every lane: a broadcast
      const int bs[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int b = bs[u];
        if (b >= 0 && (b & (kPopThreads - 1)) == tid) s_pl[b] += s_p[i0 + u];
      }
    }
  }
  __syncthreads();
  double* out = a.poisson + (int64_t)row * nb;
  for (int i = tid; i < nb; i += kPopThreads) out[i] = s_pl[i];
  if (tid == 0) {
    // sum pi = 1 bounds the candidates by 1 / p_switch <= kPopulationMaxLarge; were there ever more, the
    // lowest sample indices among the first kPopCandidates arrivals are kept
    const int n = min(*s_cnt, kPopCandidates);
    for (int i = 1; i < n; ++i) {      // insertion sort by sample index
      const int32_t ci = s_ci[i], cb = s_cb[i];
      const double cp = s_cp[i];
      int k = i - 1;
      while (k >= 0 && s_ci[k] > ci) { s_ci[k + 1] = s_ci[k]; s_cb[k + 1] = s_cb[k]; s_cp[k + 1] = s_cp[k]; --k; }
      s_ci[k + 1] = ci; s_cb[k + 1] = cb; s_cp[k + 1] = cp;
    }
    const int64_t o = (int64_t)row * kPopulationMaxLarge;
    for (int i = 0; i < kPopulationMaxLarge; ++i) {
      const bool use = i < n;
      a.large_inds[o + i] = use ? s_ci[i] : -1;
      a.large_probs[o + i] = use ? s_cp[i] : NAN;
      a.large_bins[o + i] = use ? s_cb[i] : -1;
    }
  }
}

// process.py model_posteriors / model_posteriors_multi / model_posteriors_sub for one spectrum: columns
// no-DLA, DLA levels 1..D, then (sub) the sub-DLA model; a NaN evidence at a level >= 2 enters as -inf,
// any other NaN makes every posterior NaN (numpy's max and sum propagate it)
__global__ __launch_bounds__(kPopThreads) void model_posterior_kernel(ModelPosteriorArgs a) {
#pragma clang fp contract(off)
  const int q = blockIdx.x * kPopThreads + threadIdx.x;
  if (q >= a.rows) return;
  double lp[kMaxDlas + 2];
  int n = 0;
  lp[n++] = a.lp_no[q] + a.ll_null[q];
  for (int d = 0; d < a.levels; ++d) {
    double v = a.lp_dla[(int64_t)d * a.ld_prior + q] + a.ll_dla[(int64_t)d * a.rows + q];
    if (d >= 1 && v != v) v = -INFINITY;
    lp[n++] = v;
  }
  if (a.ll_lls) lp[n++] = a.lp_lls[q] + a.ll_lls[q];
  double mx = lp[0];
  bool nan = mx != mx;
  for (int i = 1; i < n; ++i) {
    nan = nan || lp[i] != lp[i];
    if (lp[i] > mx) mx = lp[i];
  }
  if (nan) { a.p_dla[q] = NAN; return; }
  double e[kMaxDlas + 2], sum = 0.0;
  for (int i = 0; i < n; ++i) { e[i] = exp(lp[i] - mx); sum += e[i]; }
  const double p_no = e[0] / sum;
  double p = 1.0 - p_no;
  if (a.ll_lls) p = p - e[n - 1] / sum;
  a.p_dla[q] = p;
}

// ---- Poisson-binomial pmf ----------------------------------------------------------------------
// chunk c: trials probs[start .. start + len) of its bin -> len + 1 coefficients at out
__global__ __launch_bounds__(kPopThreads) void pmf_chunk_kernel(PmfChunkArgs a) {
  __shared__ double s_p[kPmfChunk];
  __shared__ double s_c[2][kPmfChunk + 2];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int len = a.len[c];
  const double* p = a.probs + a.start[c];
  for (int i = tid; i < len; i += kPopThreads) s_p[i] = p[i];
  for (int i = tid; i <= kPmfChunk; i += kPopThreads) { s_c[0][i] = i == 0 ? 1.0 : 0.0; s_c[1][i] = 0.0; }
  __syncthreads();
  int cur = 0;
  for (int j = 0; j < len; ++j) {
    const double pj = s_p[j], qj = 1.0 - pj;
    const double* src = s_c[cur];
    double* dst = s_c[cur ^ 1];
    for (int k = tid; k <= j + 1; k += kPopThreads) {
      const double keep = src[k] * qj;                         // src[j + 1] is still 0
      dst[k] = k > 0 ? __builtin_fma(src[k - 1], pj, keep) : keep;
    }
    __syncthreads();
    cur ^= 1;
  }
  double* out = a.dst[c];
  for (int i = tid; i <= len; i += kPopThreads) out[i] = s_c[cur][i];
}

// fold step s of every bin with more than s chunks: next[k] = sum_i P[i] cur[k - i], i ascending, where cur
// holds the product of chunks 0 .. s - 1 (lr + 1 coefficients) and P is chunk s (lp + 1 coefficients)
__global__ __launch_bounds__(kPopThreads) void pmf_fold_kernel(PmfFoldArgs a, int step) {
  __shared__ double s_P[kPmfChunk + 1];
  __shared__ double s_R[kPmfChunk + kPopThreads];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int nch = a.nch[b];
  if (nch <= step) return;
  const int64_t n = a.n[b];
  const int64_t lr = (int64_t)step * kPmfChunk;
  const int lp = (int)min((int64_t)kPmfChunk, n - lr);
  const int64_t k0 = (int64_t)blockIdx.x * kPopThreads;
  if (k0 > lr + lp) return;
  // the bin ends in buffer 0 after its last step: step s reads buffer (nch - s) & 1
  const double* cur = a.buf[(nch - step) & 1] + a.out_off[b];
  double* next = a.buf[(nch - step - 1) & 1] + a.out_off[b];
  const double* P = a.chunks + a.chunk_off[b] + lr + step;     // chunk c starts c kPmfChunk + c entries in
  for (int i = tid; i <= lp; i += kPopThreads) s_P[i] = P[i];
  const int64_t w0 = k0 - lp;                                  // the window cur[w0 .. k0 + 255]
  for (int i = tid; i < lp + kPopThreads; i += kPopThreads) {
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
  if (a.rows < 1) return hipSuccess;
  if (a.S < 1 || a.S > INT32_MAX || a.nz < 1 || a.nn < 1 || (int64_t)a.nz * a.nn > kSummaryMaxBins)
    return hipErrorInvalidValue;
  const PopLds L = pop_lds(a.nz, a.nn);
  hipLaunchKernelGGL(population_split_kernel, dim3((unsigned)a.rows), dim3(kPopThreads), L.total, s, a);
  return hipGetLastError();
}

hipError_t launch_model_posterior(const ModelPosteriorArgs& a, hipStream_t s) {
  if (a.rows < 1) return hipSuccess;
  if (a.levels < 1 || a.levels > kMaxDlas) return hipErrorInvalidValue;
  hipLaunchKernelGGL(model_posterior_kernel, dim3((unsigned)((a.rows + kPopThreads - 1) / kPopThreads)), dim3(kPopThreads),
                     0, s, a);
  return hipGetLastError();
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
  for (int ax = 0; ax < 2; ++ax) {
    const double* ed = ax ? n_edges : z_edges;
    const int64_t n = ax ? nn : nz;
    for (int64_t i = 0; i <= n; ++i)
      if (!std::isfinite(ed[i]) || (i > 0 && !(ed[i] > ed[i - 1])))
        return set_error(GPDLA_EINVAL, "population %s[%lld] = %g: edges must be finite and strictly increasing",
                         ax ? "log_nhi_edges" : "z_edges", (long long)i, ed[i]);
  }
  if (!(p_switch >= 1.0 / GPDLA_POPULATION_MAX_LARGE && p_switch < INFINITY))
    return set_error(GPDLA_EINVAL, "p_switch = %g: must be finite and >= 1/%d (the large list has %d slots)", p_switch,
                     GPDLA_POPULATION_MAX_LARGE, GPDLA_POPULATION_MAX_LARGE);
  if (!(p_thresh_sample >= 0.0 && p_thresh_sample < p_switch))
    return set_error(GPDLA_EINVAL, "p_thresh_sample = %g outside [0, p_switch = %g)", p_thresh_sample, p_switch);
  return GPDLA_OK;
}

}  // namespace gpdla

using namespace gpdla;

extern "C" {

int gpdla_population_split_f64(int32_t device, const double* ll, int64_t rows, int64_t S, int64_t ld,
                               const double* offset_samples, const double* log_nhi_samples, const double* min_z,
                               const double* max_z, const double* p_dlas, const gpdla_population_spec* spec,
                               double* poisson_plane, int32_t* large_inds, double* large_probs, int32_t* large_bins) {
  if (!ll || !offset_samples || !log_nhi_samples || !min_z || !max_z || !p_dlas || !spec || !poisson_plane ||
      !large_inds || !large_probs || !large_bins)
    return set_error(GPDLA_EINVAL, "null argument");
  if (rows < 0 || S < 1 || ld < S || rows > INT32_MAX || S > INT32_MAX)
    return set_error(GPDLA_EINVAL, "rows=%lld S=%lld ld=%lld", (long long)rows, (long long)S, (long long)ld);
  int rc = validate_population_grid(spec->num_z_bins, spec->num_nhi_bins, spec->z_edges, spec->log_nhi_edges,
                                    spec->p_thresh_sample, spec->p_switch);
  if (rc) return rc;
  for (int64_t q = 0; q < rows; ++q)
    if (p_dlas[q] == p_dlas[q] && !(p_dlas[q] >= 0.0 && p_dlas[q] <= 1.0))
      return set_error(GPDLA_EINVAL, "p_dlas[%lld] = %g outside [0, 1]", (long long)q, p_dlas[q]);
  if ((rc = check_device(device))) return rc;
  if (rows == 0) return GPDLA_OK;
  HIP_TRY(hipSetDevice(device));
  const int nz = spec->num_z_bins, nn = spec->num_nhi_bins;
  const size_t R = (size_t)rows, nbins = (size_t)nz * nn, NL = GPDLA_POPULATION_MAX_LARGE;
  size_t off = 0;
  auto carve = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
  const size_t o_ll = carve(R * ld * 8), o_off = carve((size_t)S * 8), o_ln = carve((size_t)S * 8);
  const size_t o_zmin = carve(R * 8), o_zmax = carve(R * 8), o_p = carve(R * 8), o_ed = carve((size_t)(nz + nn + 2) * 8);
  const size_t o_pl = carve(R * nbins * 8), o_li = carve(R * NL * 4), o_lp = carve(R * NL * 8), o_lb = carve(R * NL * 4);
  char* d = nullptr;
  auto done = [&](int code) {
    if (d) (void)hipFree(d);
    return code;
  };
#define TRY_P(expr)                                                                                                     \
  do {                                                                                                                  \
    hipError_t e_ = (expr);                                                                                             \
    if (e_ != hipSuccess)                                                                                               \
      return done(set_error(e_ == hipErrorOutOfMemory ? GPDLA_ENOMEM : GPDLA_EDEVICE, "population: %s failed: %s", #expr, \
                            hipGetErrorString(e_)));                                                                    \
  } while (0)
  TRY_P(hipMalloc((void**)&d, off));
  TRY_P(hipMemcpy(d + o_ll, ll, R * ld * 8, hipMemcpyHostToDevice));
  TRY_P(hipMemcpy(d + o_off, offset_samples, (size_t)S * 8, hipMemcpyHostToDevice));
  TRY_P(hipMemcpy(d + o_ln, log_nhi_samples, (size_t)S * 8, hipMemcpyHostToDevice));
  TRY_P(hipMemcpy(d + o_zmin, min_z, R * 8, hipMemcpyHostToDevice));
  TRY_P(hipMemcpy(d + o_zmax, max_z, R * 8, hipMemcpyHostToDevice));
  TRY_P(hipMemcpy(d + o_p, p_dlas, R * 8, hipMemcpyHostToDevice));
  TRY_P(hipMemcpy(d + o_ed, spec->z_edges, (size_t)(nz + 1) * 8, hipMemcpyHostToDevice));
  TRY_P(hipMemcpy(d + o_ed + (size_t)(nz + 1) * 8, spec->log_nhi_edges, (size_t)(nn + 1) * 8, hipMemcpyHostToDevice));
  PopulationSplitArgs pa{};
  pa.rows = (int32_t)rows; pa.ll = (const double*)(d + o_ll); pa.ld = ld; pa.S = S;
  pa.offset = (const double*)(d + o_off); pa.log_nhi = (const double*)(d + o_ln);
  pa.zmin = (const double*)(d + o_zmin); pa.zmax = (const double*)(d + o_zmax); pa.p_dla = (const double*)(d + o_p);
  pa.nz = nz; pa.nn = nn; pa.z_edges = (const double*)(d + o_ed); pa.n_edges = (const double*)(d + o_ed) + nz + 1;
  pa.p_thresh_sample = spec->p_thresh_sample; pa.p_switch = spec->p_switch;
  pa.poisson = (double*)(d + o_pl); pa.large_inds = (int32_t*)(d + o_li); pa.large_probs = (double*)(d + o_lp);
  pa.large_bins = (int32_t*)(d + o_lb);
  TRY_P(launch_population_split(pa, nullptr));
  TRY_P(hipMemcpy(poisson_plane, d + o_pl, R * nbins * 8, hipMemcpyDeviceToHost));
  TRY_P(hipMemcpy(large_inds, d + o_li, R * NL * 4, hipMemcpyDeviceToHost));
  TRY_P(hipMemcpy(large_probs, d + o_lp, R * NL * 8, hipMemcpyDeviceToHost));
  TRY_P(hipMemcpy(large_bins, d + o_lb, R * NL * 4, hipMemcpyDeviceToHost));
  return done(GPDLA_OK);
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
  size_t off = 0;
  auto carve = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
  const size_t o_probs = carve((size_t)total * 8), o_buf0 = carve(out_total * 8), o_buf1 = carve(NF ? out_total * 8 : 0);
  const size_t o_chunks = carve((size_t)chunk_entries * 8), o_cs = carve(NC * 8), o_cl = carve(NC * 4), o_cd = carve(NC * 8);
  const size_t o_fn = carve(NF * 8), o_fo = carve(NF * 8), o_fc = carve(NF * 8), o_fh = carve(NF * 4);
  char* d = nullptr;
  auto done = [&](int code) {
    if (d) (void)hipFree(d);
    return code;
  };
  TRY_P(hipMalloc((void**)&d, std::max<size_t>(off, 256)));
  double* bufs[2] = {(double*)(d + o_buf0), (double*)(d + o_buf1)};
  double* chunks = (double*)(d + o_chunks);
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
  if (total) TRY_P(hipMemcpy(d + o_probs, probs, (size_t)total * 8, hipMemcpyHostToDevice));
  TRY_P(hipMemcpy(d + o_cs, c_start.data(), NC * 8, hipMemcpyHostToDevice));
  TRY_P(hipMemcpy(d + o_cl, c_len.data(), NC * 4, hipMemcpyHostToDevice));
  TRY_P(hipMemcpy(d + o_cd, c_dst.data(), NC * 8, hipMemcpyHostToDevice));
  PmfChunkArgs ca{};
  ca.probs = (const double*)(d + o_probs); ca.start = (const int64_t*)(d + o_cs); ca.len = (const int32_t*)(d + o_cl);
  ca.dst = (double* const*)(d + o_cd);
  lt.before();
  hipLaunchKernelGGL(pmf_chunk_kernel, dim3((unsigned)NC), dim3(kPopThreads), 0, nullptr, ca);
  TRY_P(hipGetLastError());
  lt.after();
  if (NF) {
    TRY_P(hipMemcpy(d + o_fn, f_n.data(), NF * 8, hipMemcpyHostToDevice));
    TRY_P(hipMemcpy(d + o_fo, f_out.data(), NF * 8, hipMemcpyHostToDevice));
    TRY_P(hipMemcpy(d + o_fc, f_chunk.data(), NF * 8, hipMemcpyHostToDevice));
    TRY_P(hipMemcpy(d + o_fh, f_nch.data(), NF * 4, hipMemcpyHostToDevice));
    PmfFoldArgs fa{};
    fa.n = (const int64_t*)(d + o_fn); fa.out_off = (const int64_t*)(d + o_fo); fa.chunk_off = (const int64_t*)(d + o_fc);
    fa.nch = (const int32_t*)(d + o_fh); fa.chunks = chunks; fa.buf[0] = bufs[0]; fa.buf[1] = bufs[1];
    lt.before();
    for (int s = 1; s < max_nch; ++s) {
      const int64_t len = std::min<int64_t>(max_n, (int64_t)(s + 1) * kPmfChunk) + 1;
      hipLaunchKernelGGL(pmf_fold_kernel, dim3((unsigned)((len + kPopThreads - 1) / kPopThreads), (unsigned)NF),
                         dim3(kPopThreads), 0, nullptr, fa, s);
      TRY_P(hipGetLastError());
    }
    lt.after();
  }
  TRY_P(hipMemcpy(pmf, bufs[0], out_total * 8, hipMemcpyDeviceToHost));
  lt.finish();
#undef TRY_P
  return done(GPDLA_OK);
}

}  // extern "C"
