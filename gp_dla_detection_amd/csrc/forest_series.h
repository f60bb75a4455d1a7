// The Lyman-series sum of the null model (DESIGN.md sections 14 and 16; Ho, Bird & Garnett 2020,
// arXiv:2003.11036), shared by inference (forest.hip) and training (objective.hip): one definition of
// the line tables, of the comparison that decides which lines absorb at a pixel and of the order the
// lines are summed in.  For a pixel at observed wavelength lambda of a quasar at z_QSO and line
// i = 1..L:
//   z_i = (lambda - lambda_i) / lambda_i,   t_i = tau_0 c_i (1 + z_i)^beta [z_i <= z_QSO]
// with lambda_i = kTransitionWavelengths[i-1] 1e8 Angstrom and c_i = kLeadingConstants[i-1] /
// kLeadingConstants[0] (= f_i lambda_i / (f_1 lambda_1)).
#pragma once

#include <hip/hip_runtime.h>

#include "lyman_series.h"

namespace gpdla {

// lambda_i (Angstrom) and c_i into LDS: one multiplication / one division each, correctly rounded,
// i.e. the doubles a host restatement gets from the same two tables
__device__ inline void forest_tables(double* s_lam, double* s_c) {
  if (threadIdx.x < kMaxLines) {
    s_lam[threadIdx.x] = kTransitionWavelengths[threadIdx.x] * 1e8;
    s_c[threadIdx.x] = kLeadingConstants[threadIdx.x] / kLeadingConstants[0];
  }
  __syncthreads();
}

// sum_i t_i(tau_0, beta) at observed wavelength lam.  The comparison and 1 + z_i are evaluated as
// written (no contraction): a pixel one ulp either side of a line's edge must take the side the
// model's definition gives it.
__device__ inline double forest_tau(double lam, double z_qso, double tau_0, double beta, int L,
                                    const double* s_lam, const double* s_c) {
#pragma clang fp contract(off)
  double sum = 0.0;
  for (int i = 0; i < L; ++i) {
    const double li = s_lam[i];
    const double zi = (lam - li) / li;
    if (zi <= z_qso) {
      const double base = 1.0 + zi;
      sum += tau_0 * s_c[i] * pow(base, beta);
    }
  }
  return sum;
}

// The training matrices carry 1 + z_Lya per pixel (learn_qso_model.m:55-58): the observed wavelength
// is that times lambda_1, one rounded product (a host restatement multiplies the same two doubles)
__device__ inline double forest_lambda(double lya_1pz, const double* s_lam) {
#pragma clang fp contract(off)
  return lya_1pz * s_lam[0];
}

// How many lines absorb at lam, by forest_tau's comparison.  lambda_i decreases with i and the lines
// are at least 6e-5 apart relative, so z_i increases with i by far more than its rounding: the active
// lines are a prefix of the series, and the count stops at the first inactive one.
__device__ inline int forest_active_lines(double lam, double z_qso, int L, const double* s_lam) {
#pragma clang fp contract(off)
  int n = 0;
  while (n < L) {
    const double li = s_lam[n];
    const double zi = (lam - li) / li;
    if (!(zi <= z_qso)) break;
    ++n;
  }
  return n;
}

}  // namespace gpdla
