// Lyman-series forest of the null model (Ho, Bird & Garnett 2020,
// arXiv:2003.11036): the effective optical depth of the series at a pixel,
//   sum_{i=1..L} tau_0 c_i (1 + z_i)^beta [z_i <= z_QSO],  z_i = (lambda - lambda_i) / lambda_i,
// with lambda_i = kTransitionWavelengths[i-1] 1e8 Angstrom and c_i = kLeadingConstants[i-1] /
// kLeadingConstants[0] (= f_i lambda_i / (f_1 lambda_1)), summed in line order.  forest_kernel runs
// between prep_kernel and the likelihood sweep and rewrites the kMu / kOmega2 words of the valid
// slots of the fused layout; forest_f64_kernel is the same sum on a plain wavelength array.  The sum
// itself (forest_tables, forest_tau) is forest_series.h's, which the training objective shares.
// forest_covariance_kernel follows forest_kernel when the mean flux also
// multiplies the M rows (and omega^2): it rescales the u-words and rebuilds the Khatri-Rao entries.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "device_common.h"
#include "forest_series.h"
#include "internal.h"

namespace gpdla {

namespace {

// One thread per slot; gridDim.y blocks share a spectrum's slots.  Slot j holds segment j / Ls, step
// j % Ls, i.e. pixel-order position gg L + t (prep_kernel pass 3a); masked, padding and round-up
// slots have no pixel and keep their neutral words.
__global__ __launch_bounds__(256) void forest_kernel(ForestArgs a) {
  __shared__ double s_lam[kMaxLines], s_c[kMaxLines];
  forest_tables(s_lam, s_c);
  const int q = blockIdx.x;
  const SpecInfo inf = a.info[q];
  if (inf.J == 0) return;
  const int64_t pb = a.offsets[q];
  const double* wl = a.wavelengths + pb;
  const double z = a.z_qsos[q];
  const int64_t sb = inf.slot_base, cap = a.slot_cap[q];
  const int32_t* smap = a.slot_pixel + sb;
  const int L = inf.L, J = inf.J;
  const int Ls = L > 0 ? ((L + kChunkSteps - 1) / kChunkSteps) * kChunkSteps : kChunkSteps;
  const double fv = ldexp(1.0, inf.scale_e);
  for (int64_t j = threadIdx.x + 256 * (int64_t)blockIdx.y; j < cap; j += 256 * (int64_t)gridDim.y) {
    const int gg = (int)(j / Ls), t = (int)(j - (int64_t)gg * Ls);
    const int pos = (gg < 4 && t < L) ? gg * L + t : -1;
    const int pix = (pos >= 0 && pos < J) ? smap[pos] : -1;
    if (pix < 0) continue;
    // the pixel's own wavelength: in reference mode the slot's kLam word is the pos-th in-range
    // wavelength (the profile's), while its flux and model are the pos-th unmasked pixel's
    const double lam = wl[pix];
    double* row = a.panel + (sb + j) * a.row;
    if (a.variance_series) {
      const double rest = lam / (1 + z);
      const int gi = interp_index(a.rest, a.num_rest, rest);
      const double lom = interp_eval(a.rest, a.log_omega, a.num_rest, gi, rest);
      const double tau = forest_tau(lam, z, a.tau_0, a.beta, a.num_lines, s_lam, s_c);
      double om2 = exp(2 * lom);
      const double sf = 1 - exp(-tau) + a.c_0;
      om2 = om2 * (sf * sf);
      row[a.w_omega2] = om2 * fv;
    }
    if (a.mean_flux) {
      const double tau = forest_tau(lam, z, a.mf_tau_0, a.mf_beta, a.num_lines, s_lam, s_c);
      row[a.w_mu] = row[a.w_mu] * exp(-tau);  // (mu 2^(E/2)) e = (mu e) 2^(E/2): the scaling is exact
    }
  }
}

// Mean-flux suppression of the covariance: after forest_kernel, the u-words of
// every valid slot (M_i 2^(E/2), entries 4 kGT + i) are multiplied by the slot's mean flux F, the Gram
// entries are rebuilt as products of the scaled u-words of their pair (prep_kernel pass 3b's table), and
// under scope 2 the kOmega2 word is multiplied by F F.  F is forest_kernel's double: forest_tau at the
// pixel's own wavelength.  Blocks take 256 slots at a time: one thread per slot forms F (no lane repeats
// a pow) into LDS, then one wave per slot rewrites the row with lanes over entries.  Slots without a
// pixel, the tile padding, the columns of a padded rank (0 F = 0) and the other spare words are left as
// prep_kernel wrote them.
template <int K>
__global__ __launch_bounds__(256) void forest_covariance_kernel(ForestArgs a) {
  using Lay = Layout<K>;
  __shared__ double s_lam[kMaxLines], s_c[kMaxLines];
  __shared__ double s_F[256];            // the 256 slots' F, or -1: no pixel
  __shared__ double s_M[4][K];           // each wave's scaled u-words of its current slot
  __shared__ uint16_t s_rc[Lay::kNGram];
  forest_tables(s_lam, s_c);
  const int q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SpecInfo inf = a.info[q];
  if (inf.J == 0) return;
  for (int e = tid; e < Lay::kNGram; e += 256) {
    int r, c;
    gram_pair<K>(e, r, c);
    s_rc[e] = (uint16_t)(r | (c << 8));
  }
  const int64_t pb = a.offsets[q];
  const double* wl = a.wavelengths + pb;
  const double z = a.z_qsos[q];
  const int64_t sb = inf.slot_base, cap = a.slot_cap[q];
  const int32_t* smap = a.slot_pixel + sb;
  const int L = inf.L, J = inf.J;
  const int Ls = L > 0 ? ((L + kChunkSteps - 1) / kChunkSteps) * kChunkSteps : kChunkSteps;
  double* sM = s_M[wave];
  for (int64_t j0 = 256 * (int64_t)blockIdx.y; j0 < cap; j0 += 256 * (int64_t)gridDim.y) {
    __syncthreads();  // s_rc (first round); the previous round's reads of s_F
    {
      const int64_t j = j0 + tid;
      const int gg = (int)(j / Ls), t = (int)(j - (int64_t)gg * Ls);
      const int pos = (j < cap && gg < 4 && t < L) ? gg * L + t : -1;
      const int pix = (pos >= 0 && pos < J) ? smap[pos] : -1;
      s_F[tid] = pix >= 0 ? exp(-forest_tau(wl[pix], z, a.mf_tau_0, a.mf_beta, a.num_lines, s_lam, s_c)) : -1.0;
    }
    __syncthreads();
    for (int i = 0; i < 64; ++i) {
      const double F = s_F[64 * wave + i];  // wave-uniform
      if (F < 0.0) continue;
      double* row = a.panel + (sb + j0 + 64 * wave + i) * Lay::kRow;
      if (lane < K) {
        const int e = 4 * Lay::kGT + lane;
        double* w = row + (e & 3) * Lay::kJS + (e >> 2);
        const double v = *w * F;  // (M 2^(E/2)) F = (M F) 2^(E/2): one rounding, the definition's
        *w = v;
        sM[lane] = v;
      }
      if (lane == 63 && a.mean_flux_scope == 2) row[Lay::kOmega2] = row[Lay::kOmega2] * (F * F);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the wave's LDS row before its reads
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      for (int e = lane; e < Lay::kNGram; e += 64) {
        const int rc = s_rc[e];
        row[(e & 3) * Lay::kJS + (e >> 2)] = sM[rc & 255] * sM[rc >> 8];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // reads of this slot's row done before
      __builtin_amdgcn_wave_barrier();                         // the next slot overwrites it
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
}

__global__ __launch_bounds__(256) void forest_f64_kernel(const double* __restrict__ wl, int64_t n, double z_qso,
                                                         double tau_0, double beta, int32_t L,
                                                         double* __restrict__ out) {
  __shared__ double s_lam[kMaxLines], s_c[kMaxLines];
  forest_tables(s_lam, s_c);
  const int64_t i = threadIdx.x + 256 * (int64_t)blockIdx.x;
  if (i < n) out[i] = forest_tau(wl[i], z_qso, tau_0, beta, L, s_lam, s_c);
}

}  // namespace

#define GPDLA_FOR_EACH_RANK(X) X(4) X(8) X(10) X(12) X(16) X(20) X(24)

hipError_t launch_forest(int K, ForestArgs a, hipStream_t s) {
  a.row = 0;
#define X(k) if (K == k) { a.row = Layout<k>::kRow; a.w_mu = Layout<k>::kMu; a.w_omega2 = Layout<k>::kOmega2; }
  GPDLA_FOR_EACH_RANK(X)
#undef X
  if (a.row == 0 || a.num_lines < 1 || a.num_lines > kMaxLines) return hipErrorInvalidValue;
  if (a.q_count < 1) return hipSuccess;
  hipLaunchKernelGGL(forest_kernel, dim3((unsigned)a.q_count, 4), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_forest_covariance(int K, const ForestArgs& a, hipStream_t s) {
  if (a.num_lines < 1 || a.num_lines > kMaxLines || !a.mean_flux || a.mean_flux_scope < 1 || a.mean_flux_scope > 2)
    return hipErrorInvalidValue;
  if (a.q_count < 1) return hipSuccess;
#define X(k)                                                                                                  \
  if (K == k) {                                                                                               \
    hipLaunchKernelGGL(forest_covariance_kernel<k>, dim3((unsigned)a.q_count, 4), dim3(256), 0, s, a);        \
    return hipGetLastError();                                                                                 \
  }
  GPDLA_FOR_EACH_RANK(X)
#undef X
  return hipErrorInvalidValue;
}

hipError_t launch_forest_f64(const double* wl, int64_t n, double z_qso, double tau_0, double beta, int32_t L,
                             double* out, hipStream_t s) {
  if (L < 1 || L > kMaxLines) return hipErrorInvalidValue;
  if (n < 1) return hipSuccess;
  const int64_t nb = (n + 255) / 256;
  if (nb > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(forest_f64_kernel, dim3((unsigned)nb), dim3(256), 0, s, wl, n, z_qso, tau_0, beta, L, out);
  return hipGetLastError();
}

}  // namespace gpdla
