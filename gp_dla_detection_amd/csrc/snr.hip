// Per-spectrum SNR (include/gpdla.h "Per-spectrum SNR"): calc_cddf.py's find_snr
// (:906-924) for every spectrum at once, the number behind the population code's `keep` mask.
//
//   snr_kernel<T>   one 256-thread workgroup per spectrum.  Pass 1 keeps the pixels redward of
//                   1215.67 (1 + max_z) (compared in double), floors their flux and writes the ratio
//                   sqrt(noise_variance) / |flux| (formed in the cells' class T) to the spectrum's stretch of a
//                   workspace as long as the pixel arrays, in whatever order the lanes arrive: the median is a
//                   function of the multiset.  Pass 2 selects by counting: the value of rank r is the one with
//                   exactly r values below it, ties broken by position.  Real files leave about 45 pixels
//                   between z_max and the red trim, so the quadratic count is a few thousand compares; any
//                   count up to the spectrum's length works, there is no LDS cap.
// This file is compiled without FMA contraction; sqrt and / are the correctly rounded ones in both classes.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/gpdla.h"
#include "internal.h"

#pragma clang fp contract(off)

namespace gpdla {
namespace {

constexpr double kLyaRest = 1215.67;     // calc_cddf.py:914

__device__ __forceinline__ float root(float v) { return sqrtf(v); }
__device__ __forceinline__ double root(double v) { return sqrt(v); }
__device__ __forceinline__ float magnitude(float v) { return fabsf(v); }
__device__ __forceinline__ double magnitude(double v) { return fabs(v); }

template <class T>
struct SnrArgs {
  const int64_t* offsets;        // device [Q + 1]
  const T* wavelengths;
  const T* flux;
  const T* noise;
  const double* max_z;           // [Q]
  const double* norm;            // [Q] or nullptr
  T* work;                       // [pixels]
  T* snrs;                       // [Q]
};

template <class T>
__global__ __launch_bounds__(256) void snr_kernel(SnrArgs<T> a) {
  __shared__ int s_n, s_nan;
  __shared__ T s_mid[2];
  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t p0 = a.offsets[q];
  const int len = (int)(a.offsets[q + 1] - p0);
  if (tid == 0) { s_n = 0; s_nan = 0; }
  __syncthreads();
  const double edge = kLyaRest * (1.0 + a.max_z[q]);
  T* w = a.work + p0;
  for (int i = tid; i < len; i += 256) {
    if (!((double)a.wavelengths[p0 + i] > edge)) continue;
    T f = a.flux[p0 + i];
    if (a.norm) {
      const double nrm = a.norm[q];
      if ((double)f / nrm < 0.1) f = (T)(nrm * 0.1);
    } else if ((double)f < 0.1) {
      f = (T)0.1;
    }
    const T ratio = root(a.noise[p0 + i]) / magnitude(f);
    if (ratio != ratio) atomicOr(&s_nan, 1);
    w[atomicAdd(&s_n, 1)] = ratio;
  }
  __threadfence_block();
  __syncthreads();
  const int n = s_n;
  if (n == 0 || s_nan) {
    if (tid == 0) a.snrs[q] = (T)NAN;
    return;
  }
  const int r_lo = (n - 1) / 2, r_hi = n / 2;     // equal for an odd count
  for (int i = tid; i < n; i += 256) {
    const T v = w[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const T u = w[j];
      rank += (u < v || (u == v && j < i)) ? 1 : 0;
    }
    if (rank == r_lo) s_mid[0] = v;
    if (rank == r_hi) s_mid[1] = v;
  }
  __syncthreads();
  if (tid == 0) {
    const T med = r_lo == r_hi ? s_mid[0] : (s_mid[0] + s_mid[1]) / (T)2;
    a.snrs[q] = (T)1 / med;
  }
}

template <class T>
int spectrum_snrs(int32_t device, int64_t Q, const int64_t* offsets, const T* wavelengths, const T* flux, const T* noise,
                  const double* max_z, const double* norm, T* snrs) {
  if (!offsets || !max_z || !snrs) return set_error(GPDLA_EINVAL, "snrs: null argument");
  if (Q < 1 || Q > INT32_MAX) return set_error(GPDLA_EINVAL, "snrs: Q=%lld", (long long)Q);
  if (offsets[0] != 0) return set_error(GPDLA_EINVAL, "snrs: offsets[0] must be 0");
  for (int64_t q = 0; q < Q; ++q)
    if (offsets[q + 1] < offsets[q] || offsets[q + 1] - offsets[q] > INT32_MAX)
      return set_error(GPDLA_EINVAL, "snrs: offsets[%lld] = %lld after %lld", (long long)(q + 1), (long long)offsets[q + 1],
                       (long long)offsets[q]);
  const size_t P = (size_t)offsets[Q];
  if (P && (!wavelengths || !flux || !noise)) return set_error(GPDLA_EINVAL, "snrs: null pixel array");
  int rc = check_device(device);
  if (rc) return rc;
  LaunchTimes& lt = launch_times();
  lt.reset();
  HIP_TRY(hipSetDevice(device));
  DeviceStage st;
  const size_t o_off = st.carve((size_t)(Q + 1) * 8), o_w = st.carve(P * sizeof(T)), o_f = st.carve(P * sizeof(T));
  const size_t o_n = st.carve(P * sizeof(T)), o_ws = st.carve(P * sizeof(T)), o_z = st.carve((size_t)Q * 8);
  const size_t o_nm = st.carve(norm ? (size_t)Q * 8 : 0), o_s = st.carve((size_t)Q * sizeof(T));
  HIP_TRY_IN("snrs", st.alloc());
  HIP_TRY_IN("snrs", st.upload(o_off, offsets, (size_t)(Q + 1) * 8));
  if (P) {
    HIP_TRY_IN("snrs", st.upload(o_w, wavelengths, P * sizeof(T)));
    HIP_TRY_IN("snrs", st.upload(o_f, flux, P * sizeof(T)));
    HIP_TRY_IN("snrs", st.upload(o_n, noise, P * sizeof(T)));
  }
  HIP_TRY_IN("snrs", st.upload(o_z, max_z, (size_t)Q * 8));
  if (norm) HIP_TRY_IN("snrs", st.upload(o_nm, norm, (size_t)Q * 8));
  SnrArgs<T> sa{st.ptr<const int64_t>(o_off), st.ptr<const T>(o_w), st.ptr<const T>(o_f), st.ptr<const T>(o_n),
                st.ptr<const double>(o_z), norm ? st.ptr<const double>(o_nm) : nullptr, st.ptr<T>(o_ws), st.ptr<T>(o_s)};
  lt.before();
  hipLaunchKernelGGL(snr_kernel<T>, dim3((unsigned)Q), dim3(256), 0, nullptr, sa);
  HIP_TRY_IN("snrs", hipGetLastError());
  lt.after();
  HIP_TRY_IN("snrs", st.download(snrs, o_s, (size_t)Q * sizeof(T)));
  lt.finish();
  return GPDLA_OK;
}

}  // namespace
}  // namespace gpdla

using namespace gpdla;

extern "C" {

int gpdla_spectrum_snrs_f32(int32_t device, int64_t Q, const int64_t* offsets, const float* wavelengths, const float* flux,
                            const float* noise_variance, const double* max_z_dlas, const double* normalizers, float* snrs) {
  return spectrum_snrs<float>(device, Q, offsets, wavelengths, flux, noise_variance, max_z_dlas, normalizers, snrs);
}

int gpdla_spectrum_snrs_f64(int32_t device, int64_t Q, const int64_t* offsets, const double* wavelengths, const double* flux,
                            const double* noise_variance, const double* max_z_dlas, const double* normalizers, double* snrs) {
  return spectrum_snrs<double>(device, Q, offsets, wavelengths, flux, noise_variance, max_z_dlas, normalizers, snrs);
}

}  // extern "C"
