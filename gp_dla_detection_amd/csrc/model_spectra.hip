// Model spectra on the fused fp64 layout (gfx950): for each spectrum of a resident batch and a given set of 0 to 4
// absorbers, the absorption a on the likelihood's pixels, the mean the likelihood compares the flux with (a mu),
// the GP's posterior continuum mu + M w^ with the standard deviation of its low-rank part, r'K^-1 r and the
// log-likelihood.  With d = a^2 omega^2 + sigma^2, r = y - a mu, V = diag(a) M:
//     B = I + V'D^-1 V,  u = V'D^-1 r,  w^ = B^-1 u,  chi2 = r'D^-1 r - u'B^-1 u,
//     continuum_j = mu_j + M_j w^,  var_j = M_j B^-1 M_j'.
//
// One 256-thread workgroup per spectrum, three passes over its panel rows:
//   1  per pixel: a (each absorber's raw profile over the padded grid, broadened by the 7 instrument taps on its
//      own as gpdla_voigt_f64 does, the broadened profiles multiplied as in multi_dla.hip), a^2 / d, a r / d and a
//      into LDS (GPDLA_MODEL_SPECTRA_LDS pixels; beyond that the spectrum's stretch of a global workspace), and
//      the partial sums of r'D^-1 r and sum log d
//   2  the Gram and u as one weighted sum of the panel rows: thread t owns the row's words t and t + 256 and adds
//      the pixels in index order (a row is read by consecutive lanes: coalesced; fixed order: the sums are a
//      function of the spectrum alone).  Then a Cholesky factorisation of B in LDS, its inverse, w^ and u'B^-1 u
//   3  per pixel, one wave each: the two dot products of the row with w^ (its M words) and with the packed B^-1
//      (its Khatri-Rao words, off-diagonals doubled), a 64-lane butterfly, and the four outputs
// No atomics on data; repeated calls and any batching agree bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "device_common.h"
#include "internal.h"

namespace gpdla {

namespace {

constexpr int kModelLds = GPDLA_MODEL_SPECTRA_LDS;

template <int K>
__global__ __launch_bounds__(256) void model_spectra_kernel(ModelSpectraArgs a) {
  using Lay = Layout<K>;
  constexpr int kWords = Lay::kRow;               // doubles of a panel row
  constexpr int kWPT = (kWords + 255) / 256;      // row words per thread
  __shared__ double s_w[kModelLds], s_t[kModelLds], s_a[kModelLds];
  __shared__ double s_raw[256 + 2 * kWidth];
  __shared__ double s_acc[kWPT * 256], s_cv[kWPT * 256], s_cc[kWPT * 256];
  __shared__ double s_B[K * K], s_Li[K * K], s_Bi[K * K], s_u[K], s_v[K], s_wh[K];
  __shared__ double s_d4[4];
  __shared__ int s_i4[4];
  __shared__ int s_bad;

  const int q = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const SpecInfo inf = a.info[q];
  const int J = inf.J;
  if (J == 0) {  // unusable spectrum: nothing per pixel, NaN scalars
    if (tid == 0) {
      a.chi2[q] = NAN;
      a.log_likelihood[q] = NAN;
      a.num_pixels[q] = inf.n;
    }
    return;
  }
  const int64_t o0 = a.cap_offsets[q];
  if ((int64_t)inf.n > a.cap_offsets[q + 1] - o0) {  // over its capacity: nothing is written past it
    if (tid == 0) {
      atomicOr(a.status, 2);
      a.chi2[q] = NAN;
      a.log_likelihood[q] = NAN;
      a.num_pixels[q] = inf.n;
    }
    return;
  }
  const int L = inf.L;
  const int Ls = ((L + kChunkSteps - 1) / kChunkSteps) * kChunkSteps;
  const double* panel = a.panel + inf.slot_base * Lay::kRow;
  const double* lam = a.lam_pad + inf.lam_base;
  const int32_t* smap = a.slot_pixel + inf.slot_base;
  const bool in_lds = J <= kModelLds;
  double* W = in_lds ? s_w : a.scratch + inf.slot_base;
  double* T = in_lds ? s_t : a.scratch + a.scratch_plane + inf.slot_base;
  double* A = in_lds ? s_a : a.scratch + 2 * a.scratch_plane + inf.slot_base;
  // position p (pixel order) -> panel row: segment p / L, step p % L (prep_kernel)
  auto row_of = [&](int p) { return panel + (int64_t)((p / L) * Ls + p % L) * Lay::kRow; };

  // the absorbers; one that is not a number (a level without a MAP sample) gives NaN outputs
  int count = a.counts[q];
  count = count < 0 ? 0 : (count > kMaxDlas ? kMaxDlas : count);
  double zfac[kMaxDlas], Nd[kMaxDlas];
  bool nan_abs = false;
#pragma unroll
  for (int c = 0; c < kMaxDlas; ++c) {
    const double z = c < count ? a.z_dlas[(int64_t)q * kMaxDlas + c] : 0.0;
    const double N = c >= count ? 0.0 : a.nhis ? a.nhis[(int64_t)q * kMaxDlas + c]
                                               : exp10(a.log_nhis[(int64_t)q * kMaxDlas + c]);
    nan_abs |= !(fabs(z) < INFINITY) || !(fabs(N) < INFINITY);
    zfac[c] = 1.0 / (1 + z);
    Nd[c] = N;
  }
  if (nan_abs) count = 0;
  if (tid == 0) s_bad = 0;

  // ---- pass 1
  double q1 = 0.0, ldsum = 0.0;
  for (int base = 0; base < J; base += 256) {
    const int p = base + tid;
    double ab = 1.0;
    for (int c = 0; c < count; ++c) {
      __syncthreads();
      for (int i = tid; i < 256 + 2 * kWidth; i += 256) {
        const int pp = base + i;  // padded position: the profile of pixel p reads pp = p .. p + 6
        s_raw[i] = pp < J + 2 * kWidth ? raw_profile(lam[pp], zfac[c], Nd[c], a.num_lines, a.lines) : 0.0;
      }
      __syncthreads();
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k <= 2 * kWidth; ++k) acc += s_raw[tid + k] * kInstrumentProfile[k];  // voigt.c:297-299
      ab = c == 0 ? acc : ab * acc;
    }
    if (p < J) {
      const double* row = row_of(p);
      const double y = row[Lay::kY], noise = row[Lay::kNoise], mu = row[Lay::kMu], om2 = row[Lay::kOmega2];
      // process_qsos.m:191-197; masked rows (y = mu = omega^2 = 0, noise = 1) add nothing
      const double r = fma(-mu, ab, y);
      const double a2 = ab * ab;
      const double d = fma(om2, a2, noise);
      const double rd = r / d;
      W[p] = a2 / d;
      T[p] = ab * rd;
      A[p] = ab;
      q1 = fma(r, rd, q1);
      ldsum += log(d);
    }
  }
  q1 = block_reduce_sum(q1, s_d4);
  ldsum = block_reduce_sum(ldsum, s_d4);
  __threadfence_block();
  __syncthreads();

  // ---- pass 2: the weighted row sum by row word.  Word wi holds entry e = 4 (wi % kJS) + wi / kJS when
  // wi % kJS < kTiles: a Gram pair for e < kNGram (weight a^2 / d), u_i for e = 4 kGT + i (weight a r / d)
  {
    double acc[kWPT];
    bool is_g[kWPT], is_e[kWPT];
#pragma unroll
    for (int i = 0; i < kWPT; ++i) {
      const int wi = tid + 256 * i, tp = wi % Lay::kJS;
      acc[i] = 0.0;
      is_e[i] = wi < kWords && tp < Lay::kTiles;
      is_g[i] = tp < Lay::kGT;
    }
    int gg = 0, t = 0;
#pragma unroll 4
    for (int p = 0; p < J; ++p) {
      const double* row = panel + (int64_t)(gg * Ls + t) * Lay::kRow;
      const double wg = W[p], wu = T[p];
#pragma unroll
      for (int i = 0; i < kWPT; ++i)
        if (is_e[i]) acc[i] = fma(is_g[i] ? wg : wu, row[tid + 256 * i], acc[i]);
      if (++t == L) { t = 0; ++gg; }
    }
#pragma unroll
    for (int i = 0; i < kWPT; ++i) s_acc[tid + 256 * i] = acc[i];
  }
  __syncthreads();
  for (int e = tid; e < K * K; e += 256) {
    const int r = e / K, c = e % K;
    const int g = gram_index<K>(r < c ? r : c, r < c ? c : r);
    s_B[e] = s_acc[(g & 3) * Lay::kJS + (g >> 2)] + (r == c ? 1.0 : 0.0);
  }
  if (tid < K) {
    const int ue = 4 * Lay::kGT + tid;
    s_u[tid] = s_acc[(ue & 3) * Lay::kJS + (ue >> 2)];
  }
  __syncthreads();
  // Cholesky B = L L' (lower triangle of s_B), right-looking, lane i of the first wave owns row i
  for (int j = 0; j < K; ++j) {
    if (tid == 0) {
      const double piv = s_B[j * K + j];
      if (!(piv > 0.0) || !(piv < INFINITY)) s_bad = 1;
      s_B[j * K + j] = sqrt(piv);
    }
    __syncthreads();
    if (tid > j && tid < K) s_B[tid * K + j] /= s_B[j * K + j];
    __syncthreads();
    if (tid > j && tid < K) {
      const double lij = s_B[tid * K + j];
      for (int c = j + 1; c <= tid; ++c) s_B[tid * K + c] = fma(-lij, s_B[c * K + j], s_B[tid * K + c]);
    }
    __syncthreads();
  }
  // L^-1 by columns: lane c solves L x = e_c
  if (tid < K) {
    const int c = tid;
    for (int i = 0; i < K; ++i) {
      double x = 0.0;
      if (i >= c) {
        double s = i == c ? 1.0 : 0.0;
        for (int k = c; k < i; ++k) s = fma(-s_B[i * K + k], s_Li[k * K + c], s);
        x = s / s_B[i * K + i];
      }
      s_Li[i * K + c] = x;
    }
  }
  __syncthreads();
  // B^-1 = L^-T L^-1, v = L^-1 u
  for (int e = tid; e < K * K; e += 256) {
    const int r = e / K, c = e % K;
    double s = 0.0;
    for (int i = r > c ? r : c; i < K; ++i) s = fma(s_Li[i * K + r], s_Li[i * K + c], s);
    s_Bi[e] = s;
  }
  if (tid < K) {
    double s = 0.0;
    for (int k = 0; k <= tid; ++k) s = fma(s_Li[tid * K + k], s_u[k], s);
    s_v[tid] = s;
  }
  __syncthreads();
  if (tid < K) {
    double s = 0.0;
    for (int c = 0; c < K; ++c) s = fma(s_Bi[tid * K + c], s_u[c], s);
    s_wh[tid] = s;
  }
  __syncthreads();
  const bool bad = s_bad != 0;
  const bool give_nan = bad || nan_abs;
  if (tid == 0) {
    double ubu = 0.0, ldb = 0.0;
    for (int i = 0; i < K; ++i) {
      ubu = fma(s_v[i], s_v[i], ubu);
      ldb += log(s_B[i * K + i]);
    }
    const double chi2 = q1 - ubu;
    const double logdet_d = ldsum + inf.de_shift * kLn2;
    const double ll = -0.5 * (chi2 + (logdet_d + 2.0 * ldb) + inf.n * kLog2Pi);  // log_mvnpdf_low_rank.m:30-32
    if (bad && !nan_abs) atomicOr(a.status, 1);
    a.chi2[q] = give_nan ? NAN : chi2;
    a.log_likelihood[q] = give_nan ? NAN : ll;
    a.num_pixels[q] = inf.n;
  }
  // the two coefficient vectors of pass 3, by row word
#pragma unroll
  for (int i = 0; i < kWPT; ++i) {
    const int wi = tid + 256 * i, tp = wi % Lay::kJS, e = 4 * tp + wi / Lay::kJS;
    double cv = 0.0, cc = 0.0;
    if (wi < kWords && tp < Lay::kTiles) {
      if (e < Lay::kNGram) {
        int r, c;
        gram_pair<K>(e, r, c);
        cv = r == c ? s_Bi[r * K + c] : 2.0 * s_Bi[r * K + c];
      } else if (e >= 4 * Lay::kGT && e - 4 * Lay::kGT < K) {
        cc = s_wh[e - 4 * Lay::kGT];
      }
    }
    s_cv[wi] = cv;
    s_cc[wi] = cc;
  }
  // a pixel's place among the spectrum's unmasked pixels, kept where a r / d was (-1: a masked slot)
  {
    int before = 0;
    for (int base = 0; base < J; base += 256) {
      const int p = base + tid;
      const int v = (p < J && smap[p] >= 0) ? 1 : 0;
      int total;
      const int ex = block_excl_scan(v, s_i4, &total);
      if (p < J) T[p] = v ? (double)(before + ex) : -1.0;
      before += total;
    }
  }
  __threadfence_block();
  __syncthreads();

  // ---- pass 3
  const double us = ldexp(1.0, -(inf.scale_e / 2));  // back to the caller's units (exact)
  for (int p = wave; p < J; p += 4) {
    const double rk = T[p];
    if (rk < 0.0) continue;  // (wave-uniform)
    const double* row = row_of(p);
    double sv = 0.0, sc = 0.0;
    for (int wi = lane; wi < kWords; wi += 64) {
      if (wi % Lay::kJS < Lay::kTiles) {
        const double v = row[wi];
        sv = fma(v, s_cv[wi], sv);
        sc = fma(v, s_cc[wi], sc);
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      sv += __shfl_xor(sv, off);
      sc += __shfl_xor(sc, off);
    }
    if (lane == 0) {
      const int64_t o = o0 + (int64_t)rk;
      const double mu = row[Lay::kMu], ab = A[p];
      a.pixel_inds[o] = smap[p];
      a.absorption[o] = nan_abs ? NAN : ab;
      a.model_mean[o] = give_nan ? NAN : ab * mu * us;
      a.continuum_mean[o] = give_nan ? NAN : (mu + sc) * us;
      a.continuum_sd[o] = give_nan ? NAN : sqrt(fmax(sv, 0.0)) * us;
    }
  }
}

// one thread per spectrum of the batch
__global__ __launch_bounds__(256) void model_levels_kernel(ModelLevelArgs a) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= a.rows) return;
  int level;
  if (a.given) {
    level = a.given[q];
    level = level < 0 ? 0 : (level > a.levels ? a.levels : level);
  } else {
    level = 1;
    double best = -INFINITY;
    for (int d = 1; d <= a.levels; ++d) {
      const double v = a.ll_dla[(int64_t)(d - 1) * a.rows + q] + (a.lp_dla ? a.lp_dla[(int64_t)(d - 1) * a.rows + q] : 0.0);
      if (v > best) { best = v; level = d; }   // NaN never compares greater
    }
  }
  a.counts[q] = level;
  if (a.level_out) a.level_out[q] = level;
  for (int i = 0; i < kMaxDlas; ++i) {
    const int64_t src = ((int64_t)(level - 1) * a.rows + q) * kMaxDlas + i;
    a.z_dlas[(int64_t)q * kMaxDlas + i] = i < level ? a.map_z[src] : NAN;
    a.log_nhis[(int64_t)q * kMaxDlas + i] = i < level ? a.map_n[src] : NAN;
  }
}

template <int K>
hipError_t launch_model_spectra_k(const ModelSpectraArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((model_spectra_kernel<K>), dim3((unsigned)a.q_count), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace

bool model_spectra_supported(int K) {
#define X(k) if (K == k) return true;
  GPDLA_FOR_EACH_RANK(X)
#undef X
  return false;
}

hipError_t launch_model_levels(const ModelLevelArgs& a, hipStream_t s) {
  if (a.rows < 1) return hipSuccess;
  hipLaunchKernelGGL(model_levels_kernel, dim3((unsigned)((a.rows + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_model_spectra(int K, const ModelSpectraArgs& a, hipStream_t s) {
  if (a.q_count < 1) return hipSuccess;
#define X(k) if (K == k) return launch_model_spectra_k<k>(a, s);
  GPDLA_FOR_EACH_RANK(X)
#undef X
  return hipErrorInvalidValue;
}

}  // namespace gpdla
