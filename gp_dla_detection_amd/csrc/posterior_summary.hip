// Posterior summaries of the sample log-likelihood rows (include/gpdla.h "Posterior summaries";
// DESIGN.md section 13): per row and level the MAP sample and the (z_DLA, log N_HI) pairs of its base
// chain, and for level 1 the normalised sample masses binned on the caller's (z, log N_HI) grid.
//
// One 256-thread workgroup per (row, level).  This file adds the MAP outputs to the shared reductions of
// row_posterior.h, which fixes the order of every floating-point operation; the level-1 planes are its
// planes_rows<1, 512>.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/gpdla.h"
#include "internal.h"
#include "row_posterior.h"

namespace gpdla {
namespace {

static_assert(kSummaryPlanes == GPDLA_SUMMARY_PLANES && kSummaryMaxBins == GPDLA_SUMMARY_MAX_BINS, "gpdla.h");

__global__ __launch_bounds__(kRowThreads) void posterior_summary_kernel(SummaryArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const SampleRowsArgs& r = a.r;
  const int row = blockIdx.x, lvl = blockIdx.y, tid = threadIdx.x;
  const RowLds L = planes_lds(r.nz, r.nn, kRowTileOne, 1, a.planes != nullptr);
  const double* ll = r.ll + ((int64_t)lvl * r.rows + row) * r.ld;
  const RowMax best = row_first_max(ll, (int32_t)r.S, tid, (double*)(smem + L.red_v), (int32_t*)(smem + L.red_i));

  if (tid == 0) {
    const int64_t o = (int64_t)lvl * r.rows + row;
    a.map_ind[o] = best.i;
    a.map_ll[o] = best.i >= 0 ? best.v : NAN;
    // the chain: the sample itself, then its base at each shallower level
    int32_t c[kMaxDlas];
    const bool ok = best.i >= 0 && walk_chain<kMaxDlas>(r, row, best.i, lvl + 1, c);
    const double zmin = r.zmin[row], zmax = r.zmax[row];
#pragma unroll
    for (int i = 0; i < kMaxDlas; ++i) {
      const bool use = ok && i <= lvl;
      const int32_t ci = use ? c[i] : 0;
      a.map_z[o * kMaxDlas + i] = use ? sample_z(zmin, zmax, r.offset[ci]) : NAN;
      a.map_n[o * kMaxDlas + i] = use ? r.log_nhi[ci] : NAN;
    }
  }
  if (a.planes == nullptr || lvl != 0) return;
  // best.v is unused when best.i < 0: every weight is 0 then
  planes_rows<1, kRowTileOne>(r, a.nhi, row, ll, best.v, L, smem, a.planes + (int64_t)row * kSummaryPlanes * r.nz * r.nn);
}

}  // namespace

hipError_t launch_posterior_summary(const SummaryArgs& a, hipStream_t s) {
  if (a.r.rows < 1 || a.r.levels < 1) return hipSuccess;
  if (!sample_rows_ok(a.r, a.planes != nullptr)) return hipErrorInvalidValue;
  const RowLds L = planes_lds(a.r.nz, a.r.nn, kRowTileOne, 1, a.planes != nullptr);
  hipLaunchKernelGGL(posterior_summary_kernel, dim3((unsigned)a.r.rows, (unsigned)a.r.levels), dim3(kRowThreads),
                     L.total, s, a);
  return hipGetLastError();
}

}  // namespace gpdla
