// Where a DLA sample falls on a caller's (z, log N_HI) grid: shared by the posterior summaries
// (posterior_summary.hip) and the population split (population.hip), which must agree on membership.
#pragma once

#include <hip/hip_runtime.h>

namespace gpdla {

// z_j = min_z + (max_z - min_z) * offset_j with each operation rounded on its own, as numpy (and
// process_qsos.m:163) forms it: a fused multiply-add would move samples across bin edges
__device__ __forceinline__ double sample_z(double zmin, double zmax, double off) {
#pragma clang fp contract(off)
  const double span = zmax - zmin;
  const double t = span * off;
  return zmin + t;
}

// the i with e[i] <= x < e[i + 1], or -1 (also for NaN); e[0..n] strictly increasing
__device__ __forceinline__ int find_bin(const double* e, int n, double x) {
  if (!(x >= e[0]) || !(x < e[n])) return -1;
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (x >= e[mid]) lo = mid; else hi = mid;
  }
  return lo;
}

}  // namespace gpdla
