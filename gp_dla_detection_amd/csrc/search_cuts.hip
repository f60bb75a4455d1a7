// Search cuts (include/gpdla.h "Search cuts"): calc_cddf.py's `lowzcut` and
// `filter_noisy_pixels` for every spectrum at once -- which pixels of the search range are good, where the
// range ends under the proximity cut, and the absorption path each z bin keeps.
//
//   search_cuts_kernel   one 256-thread workgroup per spectrum.  Pass 1 walks the pixels in chunks of 256 in
//                        pixel order and compacts the selected ones in that order: a ballot per wave, a prefix
//                        over the 4 waves, the lane's rank among the set bits below it.  The good flags of a
//                        chunk are OR-ed into at most 9 LDS words (integer, order-free) and every finished word
//                        goes to the spectrum's stretch of the bitmap with one plain store; the word a chunk
//                        leaves unfinished is carried into the next.  Pass 2 forms the nz + 1 path values of each
//                        grid: thread t tests pixels t, t + 256, ... for being a start, finds the first bad pixel
//                        after a start by word-wise bit searches, and the terms are added as per-thread partial
//                        sums in pixel order, a 64-lane xor butterfly and the waves in order.
// No cap on the pixel count below the spectrum's length, no floating-point atomics.  This file is compiled
// without FMA contraction.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/gpdla.h"
#include "internal.h"

#pragma clang fp contract(off)

namespace gpdla {
namespace {

constexpr double kLyaRest = 1215.67;     // calc_cddf.py:934, the constant of snr.hip
constexpr int kCutThreads = 256;
constexpr int kCutWaves = kCutThreads / 64;
constexpr int kCutChunkWords = kCutThreads / 32 + 1;   // 256 bits from a bit offset below 32 touch 9 words

// X(z), catalog.absorption_distance with the cube as two products
__device__ __forceinline__ double absorption_x(double z, double om) {
  const double t = 1.0 + z;
  const double c = t * t * t;
  return 2.0 * sqrt(om * c + (1.0 - om)) / (3.0 * om);
}

__device__ __forceinline__ bool good_bit(const uint32_t* words, int i) { return (words[i >> 5] >> (i & 31)) & 1u; }

// the first bad pixel in [from, n), or n; from < n, and the bits from n on are 0
__device__ __forceinline__ int first_bad(const uint32_t* words, int from, int n) {
  int w = from >> 5;
  uint32_t inv = ~words[w] & (~0u << (from & 31));
  for (;;) {
    if (inv) {
      const int e = w * 32 + __ffs((int)inv) - 1;
      return e < n ? e : n;
    }
    ++w;
    if (w * 32 >= n) return n;
    inv = ~words[w];
  }
}

// sum of one value per thread: xor butterfly, waves in order; every thread returns the same value
__device__ __forceinline__ double block_sum(double loc, int tid, double* s_red) {
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) loc += __shfl_xor(loc, o);
  if (lane == 0) s_red[wave] = loc;
  __syncthreads();
  double v = s_red[0];
#pragma unroll
  for (int w = 1; w < kCutWaves; ++w) v += s_red[w];
  __syncthreads();
  return v;
}

__global__ __launch_bounds__(kCutThreads) void search_cuts_kernel(SearchCutArgs a) {
  __shared__ int32_t s_cnt[kCutWaves];
  __shared__ uint32_t s_bits[kCutChunkWords + 1];
  __shared__ double s_red[kCutWaves];
  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t p0 = a.offsets[q];
  const int len = (int)(a.offsets[q + 1] - p0);
  const double zmin = a.zmin[q], zmax = a.zmax[q];
  const double span = zmax - zmin;
  const double lo = kLyaRest * (1.0 + zmin), hi = kLyaRest * (1.0 + zmax);
  const bool pix = a.noise_thresh == a.noise_thresh, prox = a.proximity_zone == a.proximity_zone;
  const int64_t wo = a.word_off[q];
  const int nwords = (int)(a.word_off[q + 1] - wo);   // ceil(len / 32)
  uint32_t* words = a.words + wo;

  // ---- pass 1: the selected pixels in pixel order, their good flags as a bitmap
  int base = 0, ngood = 0;
  if (tid <= kCutChunkWords) s_bits[tid] = 0u;
  for (int c0 = 0; c0 < len; c0 += kCutThreads) {
    __syncthreads();   // s_bits holds the carried word and zeros; s_cnt is free
    const int i = c0 + tid;
    bool sel = false, good = false;
    if (i < len) {
      const double w = a.wavelengths[p0 + i];
      sel = lo < w && w < hi;
      good = sel && (!pix || a.noise[p0 + i] < a.noise_thresh);
    }
    const unsigned long long mask = __ballot(sel);
    if (lane == 0) s_cnt[wave] = __popcll(mask);
    __syncthreads();
    int pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kCutWaves; ++w) {
      if (w == wave) pre = tot;
      tot += s_cnt[w];
    }
    if (good) {
      const int pos = base + pre + __popcll(mask & ((1ull << lane) - 1ull));
      atomicOr(&s_bits[(pos >> 5) - (base >> 5)], 1u << (pos & 31));   // integer, LDS: order-free
      ++ngood;
    }
    __syncthreads();
    const int nb = base + tot, done = (nb >> 5) - (base >> 5);   // words finished by this chunk: at most 8
    if (tid < done) words[(base >> 5) + tid] = s_bits[tid];
    const uint32_t carry = s_bits[done];
    __syncthreads();
    if (tid <= kCutChunkWords) s_bits[tid] = tid == 0 ? carry : 0u;
    base = nb;
  }
  __syncthreads();
  const int n = base;
  if (tid == 0 && (n & 31)) words[n >> 5] = s_bits[0];
  for (int w = ((n + 31) >> 5) + tid; w < nwords; w += kCutThreads) words[w] = 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ngood += __shfl_xor(ngood, o);
  if (lane == 0) s_cnt[wave] = ngood;
  double z_upper = zmax;
  if (prox) {
    const double zu = zmax - a.proximity_zone;
    z_upper = zmin > zu ? zmin : zu;       // max(max_z - proximity_zone, min_z), calc_cddf.py:352
  }
  if (tid == 0) { a.npix[q] = n; a.z_upper[q] = z_upper; }
  __threadfence_block();
  __syncthreads();   // the bitmap and the wave counts are visible to the workgroup
  int total_good = 0;
#pragma unroll
  for (int w = 0; w < kCutWaves; ++w) total_good += s_cnt[w];
  const bool all_good = n >= 1 && total_good == n;

  // ---- pass 2: the path of every bin and of the whole extent, per grid (every branch on launch or spectrum
  // values alone: uniform over the workgroup)
  for (int g = 0; g < 2; ++g) {
    const int nz = a.nz[g];
    if (nz < 1) continue;
    const double* e = a.z_edges[g];
    double* out = a.path[g] + q * (int64_t)(nz + 1);
    for (int c = 0; c <= nz; ++c) {
      const double z_lo = c < nz ? e[c] : e[0], z_hi = c < nz ? e[c + 1] : e[nz];
      double val = 0.0;
      if (zmin < z_hi && z_upper > z_lo) {
        const double pmin = z_lo > zmin ? z_lo : zmin, pmax = z_hi < z_upper ? z_hi : z_upper;
        const double x_max = absorption_x(pmax, a.omega_m);
        if (!pix || all_good) {
          val = x_max - absorption_x(pmin, a.omega_m);
        } else if (n >= 2) {
          const double last = (double)(n - 1);
          auto zz = [&](int i) { return zmin + (span * (double)i) / last; };
          double loc = 0.0;
          for (int i = tid; i < n - 1; i += kCutThreads) {
            if (!good_bit(words, i)) continue;
            const double zi = zz(i);
            if (!(zi >= pmin && zi <= pmax)) continue;
            if (i > 0 && good_bit(words, i - 1) && zz(i - 1) >= pmin) continue;   // inside a region, not its start
            const int eb = first_bad(words, i + 1, n);
            double x_top = x_max;
            if (eb < n && zz(eb) < pmax) x_top = absorption_x(zz(eb - 1), a.omega_m);
            loc += x_top - absorption_x(zi, a.omega_m);
          }
          val = block_sum(loc, tid, s_red);
        }
      }
      if (tid == 0) out[c] = val;
    }
  }
}

}  // namespace

hipError_t launch_search_cuts(const SearchCutArgs& a, int64_t Q, hipStream_t s) {
  if (Q < 1) return hipSuccess;
  if (Q > INT32_MAX || a.nz[0] < 0 || a.nz[1] < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(search_cuts_kernel, dim3((unsigned)Q), dim3(kCutThreads), 0, s, a);
  return hipGetLastError();
}

namespace {

int check_edges(const char* what, int32_t nz, const double* e) {
  if (nz < 0 || nz > kSummaryMaxBins) return set_error(GPDLA_EINVAL, "search cuts: %s grid of %d z bins", what, nz);
  if (nz == 0) return GPDLA_OK;
  if (!e) return set_error(GPDLA_EINVAL, "search cuts: %s grid without edges", what);
  for (int i = 0; i <= nz; ++i)
    if (!(e[i] - e[i] == 0.0) || (i && !(e[i] > e[i - 1])))
      return set_error(GPDLA_EINVAL, "search cuts: %s z_edges[%d] = %g: edges must be finite and strictly increasing",
                       what, i, e[i]);
  return GPDLA_OK;
}

}  // namespace

int validate_search_cuts(const gpdla_search_cuts* cuts, const double* path_summary, const double* path_population) {
  const double pz = cuts->proximity_zone, nt = cuts->noise_thresh;
  if (pz != pz && nt != nt) return set_error(GPDLA_EINVAL, "search cuts: both cuts are off");
  if (pz == pz && !(pz >= 0.0 && pz < INFINITY)) return set_error(GPDLA_EINVAL, "search cuts: proximity_zone = %g", pz);
  const int32_t nzs[2] = {cuts->num_z_bins_summary, cuts->num_z_bins_population};
  const double* edges[2] = {cuts->z_edges_summary, cuts->z_edges_population};
  const double* paths[2] = {path_summary, path_population};
  const char* names[2] = {"summary", "population"};
  for (int g = 0; g < 2; ++g) {
    if (int rc = check_edges(names[g], nzs[g], edges[g])) return rc;
    if ((nzs[g] > 0) != (paths[g] != nullptr))
      return set_error(GPDLA_EINVAL, "search cuts: the %s grid and its path array go together", names[g]);
  }
  if ((nzs[0] || nzs[1]) && !(cuts->omega_m > 0.0 && cuts->omega_m <= 1.0))
    return set_error(GPDLA_EINVAL, "search cuts: omega_m = %g outside (0, 1]", cuts->omega_m);
  return GPDLA_OK;
}

}  // namespace gpdla

using namespace gpdla;

extern "C" {

int gpdla_search_cuts_f64(int32_t device, int64_t Q, const int64_t* offsets, const double* wavelengths,
                          const double* noise_variance, const double* min_z, const double* max_z,
                          const gpdla_search_cuts* cuts, const gpdla_search_cut_results* res) {
  if (!offsets || !min_z || !max_z || !cuts || !res) return set_error(GPDLA_EINVAL, "search cuts: null argument");
  if (res->memory != GPDLA_MEM_HOST) return set_error(GPDLA_EINVAL, "search cuts: results must be host memory");
  if (!res->z_uppers || !res->pixel_counts || !res->bitmap_offsets || !res->bitmap_words)
    return set_error(GPDLA_EINVAL, "search cuts: null result array");
  if (Q < 1 || Q > INT32_MAX) return set_error(GPDLA_EINVAL, "search cuts: Q=%lld", (long long)Q);
  if (offsets[0] != 0) return set_error(GPDLA_EINVAL, "search cuts: offsets[0] must be 0");
  for (int64_t q = 0; q < Q; ++q)
    if (offsets[q + 1] < offsets[q] || offsets[q + 1] - offsets[q] > INT32_MAX - 64)
      return set_error(GPDLA_EINVAL, "search cuts: offsets[%lld] = %lld after %lld", (long long)(q + 1),
                       (long long)offsets[q + 1], (long long)offsets[q]);
  const size_t P = (size_t)offsets[Q];
  if (P && (!wavelengths || !noise_variance)) return set_error(GPDLA_EINVAL, "search cuts: null pixel array");
  int rc = validate_search_cuts(cuts, res->path_summary, res->path_population);
  if (rc) return rc;
  const double pz = cuts->proximity_zone, nt = cuts->noise_thresh;
  const int32_t nzs[2] = {cuts->num_z_bins_summary, cuts->num_z_bins_population};
  const double* edges[2] = {cuts->z_edges_summary, cuts->z_edges_population};
  double* paths[2] = {res->path_summary, res->path_population};
  if ((rc = check_device(device))) return rc;
  LaunchTimes& lt = launch_times();
  lt.reset();
  HIP_TRY(hipSetDevice(device));
  int64_t* woff = res->bitmap_offsets;
  woff[0] = 0;
  for (int64_t q = 0; q < Q; ++q) woff[q + 1] = woff[q] + (offsets[q + 1] - offsets[q] + 31) / 32;
  const size_t NW = (size_t)woff[Q];
  DeviceStage st;
  const size_t o_off = st.carve((size_t)(Q + 1) * 8), o_w = st.carve(P * 8), o_n = st.carve(P * 8);
  const size_t o_zmin = st.carve((size_t)Q * 8), o_zmax = st.carve((size_t)Q * 8), o_wo = st.carve((size_t)(Q + 1) * 8);
  const size_t o_words = st.carve(NW * 4), o_np = st.carve((size_t)Q * 4), o_zu = st.carve((size_t)Q * 8);
  size_t o_e[2], o_p[2];
  for (int g = 0; g < 2; ++g) {
    o_e[g] = st.carve(nzs[g] ? (size_t)(nzs[g] + 1) * 8 : 0);
    o_p[g] = st.carve(nzs[g] ? (size_t)Q * (nzs[g] + 1) * 8 : 0);
  }
  HIP_TRY_IN("search cuts", st.alloc());
  HIP_TRY_IN("search cuts", st.upload(o_off, offsets, (size_t)(Q + 1) * 8));
  if (P) {
    HIP_TRY_IN("search cuts", st.upload(o_w, wavelengths, P * 8));
    HIP_TRY_IN("search cuts", st.upload(o_n, noise_variance, P * 8));
  }
  HIP_TRY_IN("search cuts", st.upload(o_zmin, min_z, (size_t)Q * 8));
  HIP_TRY_IN("search cuts", st.upload(o_zmax, max_z, (size_t)Q * 8));
  HIP_TRY_IN("search cuts", st.upload(o_wo, woff, (size_t)(Q + 1) * 8));
  SearchCutArgs a{};
  a.offsets = st.ptr<const int64_t>(o_off); a.wavelengths = st.ptr<const double>(o_w); a.noise = st.ptr<const double>(o_n);
  a.zmin = st.ptr<const double>(o_zmin); a.zmax = st.ptr<const double>(o_zmax);
  a.proximity_zone = pz; a.noise_thresh = nt; a.omega_m = cuts->omega_m;
  a.word_off = st.ptr<const int64_t>(o_wo); a.words = st.ptr<uint32_t>(o_words);
  a.npix = st.ptr<int32_t>(o_np); a.z_upper = st.ptr<double>(o_zu);
  for (int g = 0; g < 2; ++g) {
    a.nz[g] = nzs[g];
    if (!nzs[g]) continue;
    HIP_TRY_IN("search cuts", st.upload(o_e[g], edges[g], (size_t)(nzs[g] + 1) * 8));
    a.z_edges[g] = st.ptr<const double>(o_e[g]); a.path[g] = st.ptr<double>(o_p[g]);
  }
  lt.before();
  HIP_TRY_IN("search cuts", launch_search_cuts(a, Q, nullptr));
  lt.after();
  HIP_TRY_IN("search cuts", st.download(res->z_uppers, o_zu, (size_t)Q * 8));
  HIP_TRY_IN("search cuts", st.download(res->pixel_counts, o_np, (size_t)Q * 4));
  if (NW) HIP_TRY_IN("search cuts", st.download(res->bitmap_words, o_words, NW * 4));
  for (int g = 0; g < 2; ++g)
    if (nzs[g]) HIP_TRY_IN("search cuts", st.download(paths[g], o_p[g], (size_t)Q * (nzs[g] + 1) * 8));
  lt.finish();
  return GPDLA_OK;
}

}  // extern "C"
