// Posterior summaries of the sample log-likelihood rows (include/gpdla.h "Posterior summaries";
// DESIGN.md section 13): per row and level the MAP sample and the (z_DLA, log N_HI) pairs of its base
// chain, and for level 1 the normalised sample masses binned on the caller's (z, log N_HI) grid.
//
// One 256-thread workgroup per (row, level).  Every floating-point result is formed in an order fixed
// by the sample index and the thread count alone -- no atomics -- so a row's outputs do not depend on
// which other rows share the launch (device batching) and repeat bit for bit:
//   max / argmax   thread t takes samples t, t + 256, ... in index order; the 256 candidates are merged
//                  by a 64-lane xor butterfly and then over the 4 waves in wave order.  (max, smallest
//                  index attaining it) is associative and commutative, so this is nanmax's first maximum.
//   W = sum w_j    the same strided partial sums and the same tree (a + b == b + a bitwise, so every
//                  lane of the butterfly holds the same value).
//   bin planes     the row goes through LDS in tiles of kSummaryTile samples: (pi_j, N_j, bin_j) are
//                  staged, then every thread scans the tile in index order and adds the samples of the
//                  bins it owns (bin b belongs to thread b mod 256) to the five plane sums in LDS.  A
//                  bin's sum is therefore the sequential sum over its samples in index order.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/gpdla.h"
#include "internal.h"
#include "sample_bins.h"

namespace gpdla {
namespace {

constexpr int kSummaryThreads = 256;
constexpr int kSummaryWaves = kSummaryThreads / 64;
constexpr int kSummaryTile = 512;   // samples staged per pass (20 B each)

static_assert(kSummaryPlanes == GPDLA_SUMMARY_PLANES && kSummaryMaxBins == GPDLA_SUMMARY_MAX_BINS, "gpdla.h");
static_assert(kSummaryTile % 4 == 0, "the scan reads four bin indices at a time");

// dynamic-LDS carve (bytes; every offset a multiple of 16)
struct SummaryLds {
  size_t red_v, red_i, edges_z, edges_n, planes, pi, nh, bin, total;
};
__host__ __device__ inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }
__host__ __device__ inline SummaryLds summary_lds(int nz, int nn, bool planes) {
  SummaryLds l{};
  size_t o = 0;
  l.red_v = o; o = up16(o + kSummaryWaves * 8);
  l.red_i = o; o = up16(o + kSummaryWaves * 4);
  if (planes) {
    l.edges_z = o; o = up16(o + (size_t)(nz + 1) * 8);
    l.edges_n = o; o = up16(o + (size_t)(nn + 1) * 8);
    l.planes = o; o = up16(o + (size_t)kSummaryPlanes * nz * nn * 8);
    l.pi = o; o = up16(o + (size_t)kSummaryTile * 8);
    l.nh = o; o = up16(o + (size_t)kSummaryTile * 8);
    l.bin = o; o = up16(o + (size_t)kSummaryTile * 4);
  }
  l.total = o;
  return l;
}

__global__ __launch_bounds__(kSummaryThreads) void posterior_summary_kernel(SummaryArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int row = blockIdx.x, lvl = blockIdx.y, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const bool planes = a.planes != nullptr && lvl == 0;
  const SummaryLds L = summary_lds(a.nz, a.nn, a.planes != nullptr);
  double* s_rv = (double*)(smem + L.red_v);
  int32_t* s_ri = (int32_t*)(smem + L.red_i);
  const int32_t S = (int32_t)a.S;
  const double* ll = a.ll + ((int64_t)lvl * a.rows + row) * a.ld;

  // ---- MAP: the first maximum over the non-NaN entries
  double bv = 0.0;
  int32_t bi = -1;
  for (int64_t j = tid; j < S; j += kSummaryThreads) {
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
  for (int w = 1; w < kSummaryWaves; ++w) merge(bv, bi, s_rv[w], s_ri[w]);
  __syncthreads();

  if (tid == 0) {
    const int64_t o = (int64_t)lvl * a.rows + row;
    a.map_ind[o] = bi;
    a.map_ll[o] = bi >= 0 ? bv : NAN;
    // the chain: the sample itself, then its base at each shallower level
    int32_t c[kMaxDlas];
    bool ok = bi >= 0;
    int32_t cur = bi;
#pragma unroll
    for (int i = 0; i < kMaxDlas; ++i) {
      c[i] = cur;
      if (i < lvl && ok) {
        cur = a.base ? a.base[((int64_t)(lvl - 1 - i) * a.rows + row) * a.ld_base + cur] : -1;
        ok = cur >= 0 && cur < S;
      }
    }
    const double zmin = a.zmin[row], zmax = a.zmax[row];
#pragma unroll
    for (int i = 0; i < kMaxDlas; ++i) {
      const bool use = ok && i <= lvl;
      const int32_t ci = use ? c[i] : 0;
      a.map_z[o * kMaxDlas + i] = use ? sample_z(zmin, zmax, a.offset[ci]) : NAN;
      a.map_n[o * kMaxDlas + i] = use ? a.log_nhi[ci] : NAN;
    }
  }
  if (!planes) return;

  // ---- W = sum_j exp(l_j - max), NaN -> 0 (the resampler's weights, multi_dla.hip)
  const double m = bv;   // unused when bi < 0: every weight is 0 then
  double loc = 0.0;
  for (int64_t j = tid; j < S; j += kSummaryThreads) {
    const double v = ll[j];
    loc += (v == v) ? exp(v - m) : 0.0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) loc += __shfl_xor(loc, o);
  if (lane == 0) s_rv[wave] = loc;
  __syncthreads();
  double W = s_rv[0];
#pragma unroll
  for (int w = 1; w < kSummaryWaves; ++w) W += s_rv[w];
  const bool usable = W > 0.0 && W < INFINITY;

  // ---- binned planes
  double* s_ez = (double*)(smem + L.edges_z);
  double* s_en = (double*)(smem + L.edges_n);
  double* s_pl = (double*)(smem + L.planes);
  double* s_pi = (double*)(smem + L.pi);
  double* s_nh = (double*)(smem + L.nh);
  int32_t* s_bin = (int32_t*)(smem + L.bin);
  const int nb = a.nz * a.nn;
  for (int i = tid; i <= a.nz; i += kSummaryThreads) s_ez[i] = a.z_edges[i];
  for (int i = tid; i <= a.nn; i += kSummaryThreads) s_en[i] = a.n_edges[i];
  for (int i = tid; i < kSummaryPlanes * nb; i += kSummaryThreads) s_pl[i] = 0.0;
  const double zmin = a.zmin[row], zmax = a.zmax[row];
  for (int64_t t0 = 0; t0 < S; t0 += kSummaryTile) {
    __syncthreads();   // edges and zeroed planes ready; the previous tile's scan is over
    for (int i = tid; i < kSummaryTile; i += kSummaryThreads) {
      const int64_t j = t0 + i;
      int32_t b = -1;
      double pi = 0.0, nh = 0.0;
      if (j < S) {
        const double v = ll[j];
        const double w = (v == v) ? exp(v - m) : 0.0;
        pi = usable ? w / W : 0.0;
        nh = a.nhi[j];
        const int iz = find_bin(s_ez, a.nz, sample_z(zmin, zmax, a.offset[j]));
        const int in = find_bin(s_en, a.nn, a.log_nhi[j]);
        if (iz >= 0 && in >= 0) b = iz * a.nn + in;
      }
      s_pi[i] = pi; s_nh[i] = nh; s_bin[i] = b;
    }
    __syncthreads();
    const int cnt = (int)min((int64_t)kSummaryTile, S - t0);
    for (int i0 = 0; i0 < cnt; i0 += 4) {
      const int4 b4 = *(const int4*)(s_bin + i0);   // the same address in every lane: a broadcast
      const int bs[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int b = bs[u];
        if (b >= 0 && (b & (kSummaryThreads - 1)) == tid) {
          const double pi = s_pi[i0 + u], N = s_nh[i0 + u];
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
  double* out = a.planes + (int64_t)row * kSummaryPlanes * nb;
  for (int i = tid; i < kSummaryPlanes * nb; i += kSummaryThreads) out[i] = s_pl[i];
}

}  // namespace

hipError_t launch_posterior_summary(const SummaryArgs& a, hipStream_t s) {
  if (a.rows < 1 || a.levels < 1) return hipSuccess;
  if (a.S < 1 || a.S > INT32_MAX || a.levels > kMaxDlas) return hipErrorInvalidValue;
  if (a.planes && (a.nz < 1 || a.nn < 1 || (int64_t)a.nz * a.nn > kSummaryMaxBins)) return hipErrorInvalidValue;
  const SummaryLds L = summary_lds(a.nz, a.nn, a.planes != nullptr);
  hipLaunchKernelGGL(posterior_summary_kernel, dim3((unsigned)a.rows, (unsigned)a.levels), dim3(kSummaryThreads),
                     L.total, s, a);
  return hipGetLastError();
}

}  // namespace gpdla
