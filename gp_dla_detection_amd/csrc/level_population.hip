// Population statistics over every multi-DLA level (include/gpdla.h "Population statistics over every
// multi-DLA level"): what posterior_summary.hip's bin planes and population.hip's
// split reduce from the level-1 rows, for every level of a max_dlas = D run and with every absorber a
// sample carries -- its own and those of its base chain -- counted.
//
//   level_posterior_kernel  one thread per spectrum: P_d, the posterior of "exactly d DLAs", from the terms
//                           model_posterior_kernel forms for p_dla
//   level_planes_kernel     one 256-thread workgroup per (row, level).  pi_{d,j} is formed as the level-1
//                           kernels form it (the same strided partial sums, butterfly and wave tree).  The row
//                           goes through LDS in tiles of kLevelTile samples: thread t stages sample t's pi
//                           once and, after walking its chain, (bin, N) per slot; then every thread scans the
//                           tile's (sample, slot) entries in order and adds those of the bins it owns (bin b
//                           belongs to thread b mod 256) to the five plane sums in LDS.  A bin's sum is
//                           therefore the sequential sum in (sample index, slot) order, and level 1's planes
//                           are posterior_summary_kernel's bit for bit.
//   level_split_kernel      the same shape on the population grid with p = P_d pi_{d,j}: samples with
//                           p >= p_switch and a slot inside the grid go through an LDS integer counter and a
//                           final sort by sample index, the others add p to the Poisson-plane bin of each
//                           slot.  With one level and P_1 = p_dla it is population_split_kernel bit for bit.
// No floating-point atomics.  Every gather index of a chain is range-checked before it is used: a void chain
// (-1, or an index outside [0, S)) never becomes a read.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/gpdla.h"
#include "internal.h"
#include "sample_bins.h"

namespace gpdla {
namespace {

constexpr int kLevelThreads = 256;
constexpr int kLevelWaves = kLevelThreads / 64;
constexpr int kLevelTile = 256;        // samples staged per pass: one per thread, 8 + 12 (level) bytes each
constexpr int kLevelCandidates = 16;   // LDS slots for p >= p_switch; the kPopulationMaxLarge lowest indices are kept

static_assert(kLevelTile == kLevelThreads, "the staging pass gives every thread one sample");
static_assert(kMaxDlas == GPDLA_MAX_DLAS && kMaxDlas == 4, "the kernels dispatch on 1..4 slots");

__host__ __device__ inline size_t lv_up16(size_t x) { return (x + 15) & ~(size_t)15; }

// dynamic-LDS carves (bytes; every offset a multiple of 16).  At the 32 x 32 bin cap and four levels the
// planes kernel takes 48 + 544 + 40960 (planes) + 2048 (pi) + 8192 (N) + 4096 (bin) = 55,888 B, against
// posterior_summary_kernel's 51,792 B: the four (bin, N) pairs per sample are paid for with a tile of 256
// samples instead of 512.  The split kernel takes 48 + 544 + 8192 + 2048 + 4096 + 464 = 15,392 B.
struct LevelPlanesLds {
  size_t red_v, red_i, edges_z, edges_n, planes, pi, nh, bin, total;
};
__host__ __device__ inline LevelPlanesLds level_planes_lds(int nz, int nn, int levels) {
  LevelPlanesLds l{};
  size_t o = 0;
  l.red_v = o; o = lv_up16(o + kLevelWaves * 8);
  l.red_i = o; o = lv_up16(o + kLevelWaves * 4);
  l.edges_z = o; o = lv_up16(o + (size_t)(nz + 1) * 8);
  l.edges_n = o; o = lv_up16(o + (size_t)(nn + 1) * 8);
  l.planes = o; o = lv_up16(o + (size_t)kSummaryPlanes * nz * nn * 8);
  l.pi = o; o = lv_up16(o + (size_t)kLevelTile * 8);
  l.nh = o; o = lv_up16(o + (size_t)kLevelTile * levels * 8);
  l.bin = o; o = lv_up16(o + (size_t)kLevelTile * levels * 4);
  l.total = o;
  return l;
}
struct LevelSplitLds {
  size_t red_v, red_i, edges_z, edges_n, plane, p, bin, cand_p, cand_i, cand_b, count, total;
};
__host__ __device__ inline LevelSplitLds level_split_lds(int nz, int nn, int levels) {
  LevelSplitLds l{};
  size_t o = 0;
  l.red_v = o; o = lv_up16(o + kLevelWaves * 8);
  l.red_i = o; o = lv_up16(o + kLevelWaves * 4);
  l.edges_z = o; o = lv_up16(o + (size_t)(nz + 1) * 8);
  l.edges_n = o; o = lv_up16(o + (size_t)(nn + 1) * 8);
  l.plane = o; o = lv_up16(o + (size_t)nz * nn * 8);
  l.p = o; o = lv_up16(o + (size_t)kLevelTile * 8);
  l.bin = o; o = lv_up16(o + (size_t)kLevelTile * levels * 4);
  l.cand_p = o; o = lv_up16(o + (size_t)kLevelCandidates * 8);
  l.cand_i = o; o = lv_up16(o + (size_t)kLevelCandidates * 4);
  l.cand_b = o; o = lv_up16(o + (size_t)kLevelCandidates * kMaxDlas * 4);
  l.count = o; o = lv_up16(o + 4);
  l.total = o;
  return l;
}

// The maximum over the non-NaN entries of a row and W = sum_j exp(l_j - max) (NaN -> 0), by
// posterior_summary.hip's reductions: thread t takes samples t, t + 256, ... in index order, a 64-lane xor
// butterfly, then the 4 waves in wave order.  Every thread returns the same (m, W).
__device__ __forceinline__ void level_row_norm(const double* ll, int32_t S, int tid, double* s_rv, int32_t* s_ri,
                                               double& m, double& W) {
  const int lane = tid & 63, wave = tid >> 6;
  double bv = 0.0;
  int32_t bi = -1;
  for (int64_t j = tid; j < S; j += kLevelThreads) {
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
  for (int w = 1; w < kLevelWaves; ++w) merge(bv, bi, s_rv[w], s_ri[w]);
  __syncthreads();
  m = bv;   // unused when bi < 0: every weight is 0 then
  double loc = 0.0;
  for (int64_t j = tid; j < S; j += kLevelThreads) {
    const double v = ll[j];
    loc += (v == v) ? exp(v - m) : 0.0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) loc += __shfl_xor(loc, o);
  if (lane == 0) s_rv[wave] = loc;
  __syncthreads();
  W = s_rv[0];
#pragma unroll
  for (int w = 1; w < kLevelWaves; ++w) W += s_rv[w];
}

// The NS absorbers of sample j at level NS: c[0] = j, c[i] its base at each shallower level
// (posterior_summary_kernel's walk for the MAP sample).  False when the chain is void; an index is read
// from only after it passed the range check.
template <int NS>
__device__ __forceinline__ bool level_chain(const LevelRowsArgs& r, int row, int32_t j, int32_t S, int32_t (&c)[NS]) {
  bool ok = true;
  int32_t cur = j;
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    c[i] = cur;
    if (i < NS - 1 && ok) {
      cur = r.base ? r.base[((int64_t)(NS - 2 - i) * r.rows + row) * r.ld_base + cur] : -1;
      ok = cur >= 0 && cur < S;
    }
  }
  return ok;
}

// flat bin of absorber ci on the grid staged at s_ez / s_en, or -1
__device__ __forceinline__ int32_t level_bin(const LevelRowsArgs& r, const double* s_ez, const double* s_en,
                                             double zmin, double zmax, int32_t ci) {
  const int iz = find_bin(s_ez, r.nz, sample_z(zmin, zmax, r.offset[ci]));
  const int in = find_bin(s_en, r.nn, r.log_nhi[ci]);
  return (iz >= 0 && in >= 0) ? iz * r.nn + in : -1;
}

template <int NS>
__device__ __forceinline__ void level_planes_body(const LevelPlanesArgs& a, char* smem) {
  const LevelRowsArgs& r = a.r;
  const int row = blockIdx.x, tid = threadIdx.x;
  const LevelPlanesLds L = level_planes_lds(r.nz, r.nn, r.levels);
  const int32_t S = (int32_t)r.S;
  const double* ll = r.ll + ((int64_t)(NS - 1) * r.rows + row) * r.ld;
  double m, W;
  level_row_norm(ll, S, tid, (double*)(smem + L.red_v), (int32_t*)(smem + L.red_i), m, W);
  const bool usable = W > 0.0 && W < INFINITY;

  double* s_ez = (double*)(smem + L.edges_z);
  double* s_en = (double*)(smem + L.edges_n);
  double* s_pl = (double*)(smem + L.planes);
  double* s_pi = (double*)(smem + L.pi);
  double* s_nh = (double*)(smem + L.nh);
  int32_t* s_bin = (int32_t*)(smem + L.bin);
  const int nb = r.nz * r.nn;
  for (int i = tid; i <= r.nz; i += kLevelThreads) s_ez[i] = r.z_edges[i];
  for (int i = tid; i <= r.nn; i += kLevelThreads) s_en[i] = r.n_edges[i];
  for (int i = tid; i < kSummaryPlanes * nb; i += kLevelThreads) s_pl[i] = 0.0;
  const double zmin = r.zmin[row], zmax = r.zmax[row];
  for (int64_t t0 = 0; t0 < S; t0 += kLevelTile) {
    __syncthreads();   // edges and zeroed planes ready; the previous tile's scan is over
    {
      const int64_t j = t0 + tid;
      double pi = 0.0;
      int32_t b[NS];
      double nh[NS];
#pragma unroll
      for (int i = 0; i < NS; ++i) { b[i] = -1; nh[i] = 0.0; }
      if (j < S) {
        const double v = ll[j];
        const double w = (v == v) ? exp(v - m) : 0.0;
        pi = usable ? w / W : 0.0;
        int32_t c[NS];
        if ((NS == 1 || pi > 0.0) && level_chain<NS>(r, row, (int32_t)j, S, c)) {
#pragma unroll
          for (int i = 0; i < NS; ++i) {
            nh[i] = a.nhi[c[i]];
            b[i] = level_bin(r, s_ez, s_en, zmin, zmax, c[i]);
          }
        }
      }
      s_pi[tid] = pi;
#pragma unroll
      for (int i = 0; i < NS; ++i) { s_nh[tid * NS + i] = nh[i]; s_bin[tid * NS + i] = b[i]; }
    }
    __syncthreads();
    const int cnt = (int)min((int64_t)kLevelTile, S - t0) * NS;   // the entries beyond are -1
    for (int e0 = 0; e0 < cnt; e0 += 4) {
      const int4 b4 = *(const int4*)(s_bin + e0);   // the same address in every lane: a broadcast
      const int bs[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int b = bs[u];
        if (b >= 0 && (b & (kLevelThreads - 1)) == tid) {
          const double pi = s_pi[(e0 + u) / NS], N = s_nh[e0 + u];
          const double np = N * pi;
          s_pl[0 * nb + b] += pi;
          s_pl[1 * nb + b] += pi * pi;
          s_pl[2 * nb + b] += np;
          s_pl[3 * nb + b] += N * np;
          s_pl[4 * nb + b] += np * np;
        }
      }
    }
  }
  __syncthreads();
  double* out = a.planes + ((int64_t)row * r.levels + (NS - 1)) * kSummaryPlanes * nb;
  for (int i = tid; i < kSummaryPlanes * nb; i += kLevelThreads) out[i] = s_pl[i];
}

__global__ __launch_bounds__(kLevelThreads) void level_planes_kernel(LevelPlanesArgs a) {
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
  const LevelRowsArgs& r = a.r;
  const int row = blockIdx.x, tid = threadIdx.x;
  const LevelSplitLds L = level_split_lds(r.nz, r.nn, r.levels);
  const int32_t S = (int32_t)r.S;
  const double* ll = r.ll + ((int64_t)(NS - 1) * r.rows + row) * r.ld;
  double m, W;
  level_row_norm(ll, S, tid, (double*)(smem + L.red_v), (int32_t*)(smem + L.red_i), m, W);
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
  const int nb = r.nz * r.nn;
  for (int i = tid; i <= r.nz; i += kLevelThreads) s_ez[i] = r.z_edges[i];
  for (int i = tid; i <= r.nn; i += kLevelThreads) s_en[i] = r.n_edges[i];
  for (int i = tid; i < nb; i += kLevelThreads) s_pl[i] = 0.0;
  if (tid == 0) *s_cnt = 0;
  const double zmin = r.zmin[row], zmax = r.zmax[row];
  const double P = a.level_post[(int64_t)(NS - 1) * a.ld_post + row];
  for (int64_t t0 = 0; t0 < S; t0 += kLevelTile) {
    __syncthreads();   // edges, zeroed plane and counter ready; the previous tile's scan is over
    {
      const int64_t j = t0 + tid;
      double p = 0.0;
      int32_t b[NS];
#pragma unroll
      for (int i = 0; i < NS; ++i) b[i] = -1;
      if (j < S) {
        const double v = ll[j];
        const double w = (v == v) ? exp(v - m) : 0.0;
        const double pi = usable ? w / W : 0.0;
        p = P * pi;
        int32_t c[NS];
        // a sample at or below the sample threshold (or with a NaN p) contributes nothing: no walk
        if (p > a.p_thresh_sample && level_chain<NS>(r, row, (int32_t)j, S, c)) {
          bool any = false;
#pragma unroll
          for (int i = 0; i < NS; ++i) {
            b[i] = level_bin(r, s_ez, s_en, zmin, zmax, c[i]);
            any = any || b[i] >= 0;
          }
          if (any && p >= a.p_switch) {             // kept exactly; never enters the Poisson plane
            const int slot = atomicAdd(s_cnt, 1);   // integer, LDS: the order is fixed by the sort below
            if (slot < kLevelCandidates) {
              s_cp[slot] = p; s_ci[slot] = (int32_t)j;
#pragma unroll
              for (int i = 0; i < kMaxDlas; ++i) s_cb[slot * kMaxDlas + i] = i < NS ? b[i] : -1;
            }
#pragma unroll
            for (int i = 0; i < NS; ++i) b[i] = -1;
          }                                         // (p >= p_switch with no slot inside: every b is -1)
        }
      }
      s_p[tid] = p;
#pragma unroll
      for (int i = 0; i < NS; ++i) s_bin[tid * NS + i] = b[i];
    }
    __syncthreads();
    const int cnt = (int)min((int64_t)kLevelTile, S - t0) * NS;
    for (int e0 = 0; e0 < cnt; e0 += 4) {
      const int4 b4 = *(const int4*)(s_bin + e0);
      const int bs[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int b = bs[u];
        if (b >= 0 && (b & (kLevelThreads - 1)) == tid) s_pl[b] += s_p[(e0 + u) / NS];
      }
    }
  }
  __syncthreads();
  double* out = a.poisson + ((int64_t)row * r.levels + (NS - 1)) * nb;
  for (int i = tid; i < nb; i += kLevelThreads) out[i] = s_pl[i];
  if (tid == 0) {
    // sum_j P_d pi_{d,j} <= 1 bounds the candidates by 1 / p_switch <= kPopulationMaxLarge; were there ever
    // more, the lowest sample indices among the first kLevelCandidates arrivals are kept
    const int n = min(*s_cnt, kLevelCandidates);
    for (int i = 1; i < n; ++i) {      // insertion sort by sample index
      const int32_t ci = s_ci[i];
      const double cp = s_cp[i];
      int32_t cb[kMaxDlas];
#pragma unroll
      for (int u = 0; u < kMaxDlas; ++u) cb[u] = s_cb[i * kMaxDlas + u];
      int k = i - 1;
      while (k >= 0 && s_ci[k] > ci) {
        s_ci[k + 1] = s_ci[k]; s_cp[k + 1] = s_cp[k];
#pragma unroll
        for (int u = 0; u < kMaxDlas; ++u) s_cb[(k + 1) * kMaxDlas + u] = s_cb[k * kMaxDlas + u];
        --k;
      }
      s_ci[k + 1] = ci; s_cp[k + 1] = cp;
#pragma unroll
      for (int u = 0; u < kMaxDlas; ++u) s_cb[(k + 1) * kMaxDlas + u] = cb[u];
    }
    const int64_t o = ((int64_t)row * r.levels + (NS - 1)) * kPopulationMaxLarge;
    for (int i = 0; i < kPopulationMaxLarge; ++i) {
      const bool use = i < n;
      a.large_inds[o + i] = use ? s_ci[i] : -1;
      a.large_probs[o + i] = use ? s_cp[i] : NAN;
#pragma unroll
      for (int u = 0; u < kMaxDlas; ++u) a.large_bins[(o + i) * kMaxDlas + u] = use ? s_cb[i * kMaxDlas + u] : -1;
    }
  }
}

__global__ __launch_bounds__(kLevelThreads) void level_split_kernel(LevelSplitArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  switch (blockIdx.y) {   // uniform over the workgroup
    case 0: level_split_body<1>(a, smem); break;
    case 1: level_split_body<2>(a, smem); break;
    case 2: level_split_body<3>(a, smem); break;
    default: level_split_body<4>(a, smem); break;
  }
}

// model_posterior_kernel's terms (population.hip), each DLA level's posterior kept: columns no-DLA, DLA
// levels 1..D, then (sub) the sub-DLA model; a NaN evidence at a level >= 2 enters as -inf, any other NaN
// makes every posterior NaN
__global__ __launch_bounds__(kLevelThreads) void level_posterior_kernel(LevelPosteriorArgs a) {
#pragma clang fp contract(off)
  const int q = blockIdx.x * kLevelThreads + threadIdx.x;
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
  if (nan) {
    for (int d = 0; d < a.levels; ++d) a.level_post[(int64_t)d * a.rows + q] = NAN;
    return;
  }
  double e[kMaxDlas + 2], sum = 0.0;
  for (int i = 0; i < n; ++i) { e[i] = exp(lp[i] - mx); sum += e[i]; }
  for (int d = 0; d < a.levels; ++d) a.level_post[(int64_t)d * a.rows + q] = e[1 + d] / sum;
}

bool level_rows_ok(const LevelRowsArgs& r) {
  return r.S >= 1 && r.S <= INT32_MAX && r.levels >= 1 && r.levels <= kMaxDlas && r.nz >= 1 && r.nn >= 1 &&
         (int64_t)r.nz * r.nn <= kSummaryMaxBins && (r.levels == 1 || (r.base && r.ld_base >= r.S)) && r.ld >= r.S;
}

}  // namespace

hipError_t launch_level_posterior(const LevelPosteriorArgs& a, hipStream_t s) {
  if (a.rows < 1) return hipSuccess;
  if (a.levels < 1 || a.levels > kMaxDlas) return hipErrorInvalidValue;
  hipLaunchKernelGGL(level_posterior_kernel, dim3((unsigned)((a.rows + kLevelThreads - 1) / kLevelThreads)),
                     dim3(kLevelThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_level_planes(const LevelPlanesArgs& a, hipStream_t s) {
  if (a.r.rows < 1) return hipSuccess;
  if (!level_rows_ok(a.r)) return hipErrorInvalidValue;
  const LevelPlanesLds L = level_planes_lds(a.r.nz, a.r.nn, a.r.levels);
  hipLaunchKernelGGL(level_planes_kernel, dim3((unsigned)a.r.rows, (unsigned)a.r.levels), dim3(kLevelThreads), L.total,
                     s, a);
  return hipGetLastError();
}

hipError_t launch_level_split(const LevelSplitArgs& a, hipStream_t s) {
  if (a.r.rows < 1) return hipSuccess;
  if (!level_rows_ok(a.r)) return hipErrorInvalidValue;
  const LevelSplitLds L = level_split_lds(a.r.nz, a.r.nn, a.r.levels);
  hipLaunchKernelGGL(level_split_kernel, dim3((unsigned)a.r.rows, (unsigned)a.r.levels), dim3(kLevelThreads), L.total,
                     s, a);
  return hipGetLastError();
}

}  // namespace gpdla

using namespace gpdla;

namespace {

// the inputs both stand-alone calls share, on the device
struct LevelHostRows {
  char* d = nullptr;
  size_t off = 0;
  size_t carve(size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; }
};

int check_level_rows(const double* ll, int64_t rows, int64_t S, int64_t ld, const double* offset_samples,
                     const double* log_nhi_samples, const double* min_z, const double* max_z, const int32_t* base_inds,
                     int32_t levels) {
  if (!ll || !offset_samples || !log_nhi_samples || !min_z || !max_z) return set_error(GPDLA_EINVAL, "null argument");
  if (rows < 0 || S < 1 || ld < S || rows > INT32_MAX || S > INT32_MAX)
    return set_error(GPDLA_EINVAL, "rows=%lld S=%lld ld=%lld", (long long)rows, (long long)S, (long long)ld);
  if (levels < 1 || levels > GPDLA_MAX_DLAS) return set_error(GPDLA_EINVAL, "levels=%d outside 1..%d", levels, GPDLA_MAX_DLAS);
  if (levels > 1 && !base_inds) return set_error(GPDLA_EINVAL, "levels=%d needs base_inds", levels);
  return GPDLA_OK;
}

}  // namespace

#define TRY_L(expr)                                                                                                          \
  do {                                                                                                                       \
    hipError_t e_ = (expr);                                                                                                  \
    if (e_ != hipSuccess)                                                                                                    \
      return done(set_error(e_ == hipErrorOutOfMemory ? GPDLA_ENOMEM : GPDLA_EDEVICE, "level population: %s failed: %s", #expr, \
                            hipGetErrorString(e_)));                                                                         \
  } while (0)

extern "C" {

int gpdla_level_planes_f64(int32_t device, const double* ll, int64_t rows, int64_t S, int64_t ld,
                           const double* offset_samples, const double* log_nhi_samples, const double* nhi_samples,
                           const double* min_z, const double* max_z, const int32_t* base_inds, int32_t levels,
                           const gpdla_summary_spec* spec, double* bin_planes) {
  int rc = check_level_rows(ll, rows, S, ld, offset_samples, log_nhi_samples, min_z, max_z, base_inds, levels);
  if (rc) return rc;
  if (!nhi_samples || !spec || !bin_planes) return set_error(GPDLA_EINVAL, "null argument");
  // the edge rules of both grids are the same; the thresholds here are placeholders that always pass
  if ((rc = validate_population_grid(spec->num_z_bins, spec->num_nhi_bins, spec->z_edges, spec->log_nhi_edges, 0.0, 1.0)))
    return rc;
  if ((rc = check_device(device))) return rc;
  if (rows == 0) return GPDLA_OK;
  HIP_TRY(hipSetDevice(device));
  const int nz = spec->num_z_bins, nn = spec->num_nhi_bins;
  const size_t R = (size_t)rows, LV = (size_t)levels, nbins = (size_t)nz * nn;
  LevelHostRows h;
  const size_t o_ll = h.carve(LV * R * ld * 8), o_base = h.carve(levels > 1 ? (LV - 1) * R * ld * 4 : 0);
  const size_t o_off = h.carve((size_t)S * 8), o_ln = h.carve((size_t)S * 8), o_nh = h.carve((size_t)S * 8);
  const size_t o_zmin = h.carve(R * 8), o_zmax = h.carve(R * 8), o_ed = h.carve((size_t)(nz + nn + 2) * 8);
  const size_t o_pl = h.carve(R * LV * kSummaryPlanes * nbins * 8);
  char*& d = h.d;
  auto done = [&](int code) {
    if (d) (void)hipFree(d);
    return code;
  };
  TRY_L(hipMalloc((void**)&d, h.off));
  TRY_L(hipMemcpy(d + o_ll, ll, LV * R * ld * 8, hipMemcpyHostToDevice));
  if (levels > 1) TRY_L(hipMemcpy(d + o_base, base_inds, (LV - 1) * R * ld * 4, hipMemcpyHostToDevice));
  TRY_L(hipMemcpy(d + o_off, offset_samples, (size_t)S * 8, hipMemcpyHostToDevice));
  TRY_L(hipMemcpy(d + o_ln, log_nhi_samples, (size_t)S * 8, hipMemcpyHostToDevice));
  TRY_L(hipMemcpy(d + o_nh, nhi_samples, (size_t)S * 8, hipMemcpyHostToDevice));
  TRY_L(hipMemcpy(d + o_zmin, min_z, R * 8, hipMemcpyHostToDevice));
  TRY_L(hipMemcpy(d + o_zmax, max_z, R * 8, hipMemcpyHostToDevice));
  TRY_L(hipMemcpy(d + o_ed, spec->z_edges, (size_t)(nz + 1) * 8, hipMemcpyHostToDevice));
  TRY_L(hipMemcpy(d + o_ed + (size_t)(nz + 1) * 8, spec->log_nhi_edges, (size_t)(nn + 1) * 8, hipMemcpyHostToDevice));
  LevelPlanesArgs a{};
  a.r.rows = (int32_t)rows; a.r.levels = levels; a.r.ll = (const double*)(d + o_ll); a.r.ld = ld; a.r.S = S;
  a.r.base = levels > 1 ? (const int32_t*)(d + o_base) : nullptr; a.r.ld_base = ld;
  a.r.offset = (const double*)(d + o_off); a.r.log_nhi = (const double*)(d + o_ln);
  a.r.zmin = (const double*)(d + o_zmin); a.r.zmax = (const double*)(d + o_zmax);
  a.r.nz = nz; a.r.nn = nn; a.r.z_edges = (const double*)(d + o_ed); a.r.n_edges = (const double*)(d + o_ed) + nz + 1;
  a.nhi = (const double*)(d + o_nh); a.planes = (double*)(d + o_pl);
  TRY_L(launch_level_planes(a, nullptr));
  TRY_L(hipMemcpy(bin_planes, d + o_pl, R * LV * kSummaryPlanes * nbins * 8, hipMemcpyDeviceToHost));
  return done(GPDLA_OK);
}

int gpdla_population_split_levels_f64(int32_t device, const double* ll, int64_t rows, int64_t S, int64_t ld,
                                      const double* offset_samples, const double* log_nhi_samples,
                                      const double* min_z, const double* max_z, const int32_t* base_inds,
                                      int32_t levels, const double* level_posteriors,
                                      const gpdla_population_spec* spec, double* poisson_plane,
                                      int32_t* large_inds, double* large_probs, int32_t* large_bins) {
  int rc = check_level_rows(ll, rows, S, ld, offset_samples, log_nhi_samples, min_z, max_z, base_inds, levels);
  if (rc) return rc;
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
  const int nz = spec->num_z_bins, nn = spec->num_nhi_bins;
  const size_t R = (size_t)rows, LV = (size_t)levels, nbins = (size_t)nz * nn, NL = GPDLA_POPULATION_MAX_LARGE;
  LevelHostRows h;
  const size_t o_ll = h.carve(LV * R * ld * 8), o_base = h.carve(levels > 1 ? (LV - 1) * R * ld * 4 : 0);
  const size_t o_off = h.carve((size_t)S * 8), o_ln = h.carve((size_t)S * 8);
  const size_t o_zmin = h.carve(R * 8), o_zmax = h.carve(R * 8), o_P = h.carve(LV * R * 8);
  const size_t o_ed = h.carve((size_t)(nz + nn + 2) * 8);
  const size_t o_pl = h.carve(R * LV * nbins * 8), o_li = h.carve(R * LV * NL * 4), o_lp = h.carve(R * LV * NL * 8);
  const size_t o_lb = h.carve(R * LV * NL * kMaxDlas * 4);
  char*& d = h.d;
  auto done = [&](int code) {
    if (d) (void)hipFree(d);
    return code;
  };
  TRY_L(hipMalloc((void**)&d, h.off));
  TRY_L(hipMemcpy(d + o_ll, ll, LV * R * ld * 8, hipMemcpyHostToDevice));
  if (levels > 1) TRY_L(hipMemcpy(d + o_base, base_inds, (LV - 1) * R * ld * 4, hipMemcpyHostToDevice));
  TRY_L(hipMemcpy(d + o_off, offset_samples, (size_t)S * 8, hipMemcpyHostToDevice));
  TRY_L(hipMemcpy(d + o_ln, log_nhi_samples, (size_t)S * 8, hipMemcpyHostToDevice));
  TRY_L(hipMemcpy(d + o_zmin, min_z, R * 8, hipMemcpyHostToDevice));
  TRY_L(hipMemcpy(d + o_zmax, max_z, R * 8, hipMemcpyHostToDevice));
  TRY_L(hipMemcpy(d + o_P, level_posteriors, LV * R * 8, hipMemcpyHostToDevice));
  TRY_L(hipMemcpy(d + o_ed, spec->z_edges, (size_t)(nz + 1) * 8, hipMemcpyHostToDevice));
  TRY_L(hipMemcpy(d + o_ed + (size_t)(nz + 1) * 8, spec->log_nhi_edges, (size_t)(nn + 1) * 8, hipMemcpyHostToDevice));
  LevelSplitArgs a{};
  a.r.rows = (int32_t)rows; a.r.levels = levels; a.r.ll = (const double*)(d + o_ll); a.r.ld = ld; a.r.S = S;
  a.r.base = levels > 1 ? (const int32_t*)(d + o_base) : nullptr; a.r.ld_base = ld;
  a.r.offset = (const double*)(d + o_off); a.r.log_nhi = (const double*)(d + o_ln);
  a.r.zmin = (const double*)(d + o_zmin); a.r.zmax = (const double*)(d + o_zmax);
  a.r.nz = nz; a.r.nn = nn; a.r.z_edges = (const double*)(d + o_ed); a.r.n_edges = (const double*)(d + o_ed) + nz + 1;
  a.level_post = (const double*)(d + o_P); a.ld_post = rows;
  a.p_thresh_sample = spec->p_thresh_sample; a.p_switch = spec->p_switch;
  a.poisson = (double*)(d + o_pl); a.large_inds = (int32_t*)(d + o_li); a.large_probs = (double*)(d + o_lp);
  a.large_bins = (int32_t*)(d + o_lb);
  TRY_L(launch_level_split(a, nullptr));
  TRY_L(hipMemcpy(poisson_plane, d + o_pl, R * LV * nbins * 8, hipMemcpyDeviceToHost));
  TRY_L(hipMemcpy(large_inds, d + o_li, R * LV * NL * 4, hipMemcpyDeviceToHost));
  TRY_L(hipMemcpy(large_probs, d + o_lp, R * LV * NL * 8, hipMemcpyDeviceToHost));
  TRY_L(hipMemcpy(large_bins, d + o_lb, R * LV * NL * kMaxDlas * 4, hipMemcpyDeviceToHost));
  return done(GPDLA_OK);
}

}  // extern "C"
#undef TRY_L
