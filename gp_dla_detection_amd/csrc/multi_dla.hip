// Multi-DLA levels on the fused fp64 path (gfx950): the level-d likelihood sweep (d DLAs per
// sample), the per-spectrum posterior resampler that draws each sample's base sample and builds the
// next level's chain table, and the NaN-aware log-mean-exp of a level.
//
// The model is Ho, Bird & Garnett 2020 (arXiv:2003.11036) as laid out in DESIGN.md "Multi-DLA".
// The sweep is the single-DLA likelihood_kernel (kernels.hip) with the Voigt part repeated per DLA:
// same slot panel, LDS ring, f64 MFMA Gram and quad LDL^T; kernels.hip itself is left as it is, so
// its single-DLA code objects do not change.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "device_common.h"
#include "internal.h"

namespace gpdla {

namespace {

// stage_chunk of kernels.hip (see there for the hazards inside the string): chunk c's 16 panel rows
// into an LDS ring buffer by global_load_lds_dwordx4, wave w the 4 rows of segment w.
template <int K>
__device__ inline void stage_chunk_m(const double* __restrict__ panel, int Ls, int c, uint32_t buf,
                                     int wave_s, const uint32_t (&voff)[Layout<K>::kPieces]) {
  using Lay = Layout<K>;
#pragma unroll
  for (int tt = 0; tt < kChunkSteps; ++tt) {
    const double* src = panel + ((int64_t)wave_s * Ls + c * kChunkSteps + tt) * Lay::kRow;
    const uint32_t dst = buf + (uint32_t)((tt * 4 + wave_s) * Lay::kRowS * 8);
#pragma unroll
    for (int h = 0; h < Lay::kPieces; ++h) {
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
      asm volatile("s_nop 4\n\ts_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2"
                   :: "s"(dst + h * 1024), "v"(voff[h]), "s"(src) : "memory", "m0");
#pragma clang diagnostic pop
    }
  }
}

// Raw 3-line profiles exp(N tot) of one DLA at a chunk's 4 wavelengths: the chunk prologue of
// likelihood_kernel (one shared reciprocal for the 12 T_j = 1/x_j^2, branch-free outer wings, the
// rare inner-wing / core fix-up, table exp), as a function so that it can run once per DLA.
__device__ inline void raw_chunk3(const double (&lamc)[kChunkSteps], const double (&afac)[3], double N,
                                  double core_lim, bool wave_clamp, const double* __restrict__ core_lds,
                                  const double* __restrict__ wing_lds, const double* __restrict__ exp_lds,
                                  double (&rwv)[kChunkSteps]) {
  double tot[kChunkSteps];
  uint32_t cm = 0;
  double Tj[3][kChunkSteps];
  {
    double a0[kChunkSteps], a1[kChunkSteps], a2[kChunkSteps], p01[kChunkSteps], qq[kChunkSteps], iq[kChunkSteps];
#pragma unroll
    for (int tt = 0; tt < kChunkSteps; ++tt) {
      tot[tt] = 0.0;
      const double x0 = fma(lamc[tt], afac[0], -kC2), x1 = fma(lamc[tt], afac[1], -kC2),
                   x2 = fma(lamc[tt], afac[2], -kC2);
      cm |= (((fabs(x0) < kOuterX) | (fabs(x1) < kOuterX) | (fabs(x2) < kOuterX)) ? 1u : 0u) << tt;
      a0[tt] = fma(x0, x0, 0x1p-60); a1[tt] = fma(x1, x1, 0x1p-60); a2[tt] = fma(x2, x2, 0x1p-60);
      p01[tt] = a0[tt] * a1[tt];
      qq[tt] = p01[tt] * a2[tt];
    }
    batch_rcp4(qq, iq);
#pragma unroll
    for (int tt = 0; tt < kChunkSteps; ++tt) {
      const double r01 = iq[tt] * a2[tt];
      Tj[0][tt] = a1[tt] * r01;
      Tj[1][tt] = a0[tt] * r01;
      Tj[2][tt] = p01[tt] * iq[tt];
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    int zoff;
    asm volatile("s_mov_b32 %0, 0" : "=s"(zoff));
    const double* wl = wing_lds + zoff + j * kWingStride;
#pragma unroll
    for (int tt = 0; tt < kChunkSteps; ++tt) tot[tt] -= outer_poly(wl, Tj[j][tt]);
  }
  if (cm) {
#pragma unroll
    for (int tt = 0; tt < kChunkSteps; ++tt) {
      if (cm & (1u << tt)) {
        double ax, T;
        const double* wl;
        int j;
        nearest_line(lamc[tt], afac, Tj[0][tt], Tj[1][tt], Tj[2][tt], wing_lds, ax, T, wl, j);
        if (ax >= kCoreX) {
          tot[tt] += outer_poly(wl, T) - wing_poly(wl, T);
        } else {
          const double cf = core_eval(core_lds + j * kCoreTable, ax);
          double t = 0.0;
#pragma unroll
          for (int jj = 0; jj < 3; ++jj) t -= jj == j ? cf : outer_poly(wing_lds + jj * kWingStride, Tj[jj][tt]);
          tot[tt] = fmax(t, core_lim);
        }
      }
    }
  }
  if (wave_clamp) {
#pragma unroll
    for (int tt = 0; tt < kChunkSteps; ++tt) rwv[tt] = exp_tab128_nc(fmax(N * tot[tt], -1100.0), exp_lds);
  } else {
#pragma unroll
    for (int tt = 0; tt < kChunkSteps; ++tt) rwv[tt] = exp_tab128_nc(N * tot[tt], exp_lds);
  }
}

constexpr int multi_min_blocks(int K, int D) {
  return K <= (D <= 2 ? GPDLA_MULTI_2BLOCK_MAXK_D2 : D == 3 ? GPDLA_MULTI_2BLOCK_MAXK_D3 : GPDLA_MULTI_2BLOCK_MAXK_D4)
             ? 2 : 1;
}

// ---------------------------------------------------------------------------------------------
// Level-D sweep: one spectrum and 64 samples per block (4 waves x 16), lanes as in
// likelihood_kernel (sample = lane & 15, segment = lane >> 4).  DLA 0 of a lane is the sample's own,
// DLAs 1..D-1 those of its chain; each has its line factors, column density and raw-profile window,
// is broadened by the 7 taps on its own, and the D broadened profiles are multiplied (own first).
// Everything from r = y - mu a on is the single-DLA code.  There is no null-model lane here.
// ---------------------------------------------------------------------------------------------
template <int K, int D>
__global__ __launch_bounds__(256, multi_min_blocks(K, D)) void multi_level_kernel(MultiLevelArgs a) {
  using Lay = Layout<K>;
  constexpr int kTiles = Lay::kTiles;
  constexpr int kGT = Lay::kGT;
  constexpr int kRowS = Lay::kRowS;
  constexpr int kJS = Lay::kJS;
  constexpr int kBuf = 4 * kChunkSteps * kRowS;
  static_assert(kWavesPerBlock == 4, "stage_chunk_m: one wave per segment");
  static_assert(D >= 2 && D <= kMaxDlas, "levels 2..kMaxDlas");
  constexpr int kWingLds = 4 * ((3 * kWingStride + 3) / 4);
  constexpr int kExpLds = 128;
  constexpr int kCoreLds = 3 * kCoreTable + kWingLds + kExpLds;
  __shared__ __attribute__((aligned(16))) double lds[2 * kBuf + kCoreLds];
  double* core_lds = lds + 2 * kBuf;
  double* wing_lds = core_lds + 3 * kCoreTable;
  double* exp_lds = wing_lds + kWingLds;

  // XCD-aware block order, as likelihood_kernel
  const int64_t blocks_x = (a.S + kSamplesPerBlock - 1) / kSamplesPerBlock;
  const int64_t per_xcd = gridDim.x / 8;
  const int64_t v = (int64_t)(blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
  if (v >= blocks_x * a.q_count) return;
  const int q = (int)(v / blocks_x);
  const int64_t bx = v - (int64_t)q * blocks_x;
  const SpecInfo inf = a.info[q];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t s_base = bx * kSamplesPerBlock + wave * kSamplesPerWave;
  if (inf.J == 0) {  // unusable spectrum: NaN rows at every level
    const int64_t su = s_base + (lane >> 2);
    if ((lane & 3) == 0 && su < a.S) a.sample_ll[q * a.ld + a.perm[su]] = NAN;
    return;
  }
  const int L = inf.L;
  const int nchunks = (L + kChunkSteps - 1) / kChunkSteps;
  const int Ls = nchunks * kChunkSteps;
  const double* panel = a.panel + inf.slot_base * Lay::kRow;
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)lds;
  uint32_t voff[Lay::kPieces];
#pragma unroll
  for (int h = 0; h < Lay::kPieces; ++h) voff[h] = (uint32_t)(lane * 16 + h * 1024);

  stage_chunk_m<K>(panel, Ls, 0, lds_base, wave_s, voff);
  for (int i = threadIdx.x; i < 3 * kCoreTable; i += 256) core_lds[i] = a.lines.buf[i];
  if (threadIdx.x < 128) exp_lds[threadIdx.x] = a.lines.buf[kLineBufExp128 + threadIdx.x];
  if (threadIdx.x < 3 * kWingStride) wing_lds[threadIdx.x] = a.lines.buf[kLineBufWing + threadIdx.x];

  // ---- per-lane DLAs.  Idle lanes (s >= S) and samples without a chain run with N = 0 (absorption
  // exactly 1) and their output is dropped / NaN.
  const int g = lane >> 4;
  const int64_t s = s_base + (lane & 15);
  const bool live = s < a.S;
  double off[D], Nd[D];
  off[0] = live ? a.offsets[s] : 0.5;
  Nd[0] = live ? a.nhi[s] : 0.0;
  bool excl = false;  // the designated NaN: no chain, or a base DLA closer than min_z_separation
  {
    const int32_t* ch = a.chain + ((int64_t)q * a.S + (live ? a.perm[s] : 0)) * kMaxChain;
#pragma unroll
    for (int d = 1; d < D; ++d) {
      const int32_t c = live ? ch[d - 1] : -1;
      const bool ok = c >= 0 && c < a.S;
      excl |= !ok;
      off[d] = ok ? a.offsets_c[c] : 0.5;
      Nd[d] = ok ? a.nhi_c[c] : 0.0;
    }
  }
  const double zspan = inf.zmax - inf.zmin;
  double afac[D][3], core_lim[D];
  {
    // the exclusion compares z values rounded as the host computes them (no contraction)
    const double z0 = __dadd_rn(inf.zmin, __dmul_rn(zspan, off[0]));
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const double zdla = inf.zmin + zspan * off[d];  // process_qsos.m:163-165
      const double zfac = 1.0 / (1 + zdla);
#pragma unroll
      for (int j = 0; j < 3; ++j) afac[d][j] = a.lines.buf[kLineBufFac + j] * zfac;
      core_lim[d] = -1100.0 / Nd[d];
      if (d > 0) {
        const double zd = __dadd_rn(inf.zmin, __dmul_rn(zspan, off[d]));
        excl |= fabs(z0 - zd) < a.min_z_separation;
      }
    }
  }
  const double* lamp = a.lam_pad + inf.lam_base + (int64_t)g * L;
  double lw[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) lw[i] = lamp[i];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  bool wave_clamp;
  {
    double fmax9 = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) fmax9 += fabs(wing_poly(wing_lds + j * kWingStride, 1.0 / (kCoreX * kCoreX)));
    bool big = false;
#pragma unroll
    for (int d = 0; d < D; ++d) big |= !(Nd[d] * fmax9 <= 1e7);
    wave_clamp = __builtin_amdgcn_ballot_w64(big) != 0;
  }

  // one 10-register ring per DLA (see likelihood_kernel): window of phase P at win[d][(4 P + i) % 10]
  double win[D][10];
#pragma unroll
  for (int d = 0; d < D; ++d)
#pragma unroll
    for (int i = 0; i < 6; ++i) win[d][i] = raw_profile3<kExpLds>(lw[i], afac[d], Nd[d], core_lds, wing_lds, exp_lds);

  double acc[kTiles];
#pragma unroll
  for (int t = 0; t < kTiles; ++t) acc[t] = 0.0;
  double q1 = 0.0;
  double pm = 1.0;
  int pe = 0;

  auto chunk = [&](const int c, auto phase) __attribute__((always_inline)) {
    constexpr int B = (4 * decltype(phase)::value) % 10;
    double* cur = lds + (c & 1) * kBuf;
    if (c + 1 < nchunks)
      stage_chunk_m<K>(panel, Ls, c + 1, lds_base + (uint32_t)(((c + 1) & 1) * kBuf * 8), wave_s, voff);
    double lamc[kChunkSteps], abs_[kChunkSteps];
#pragma unroll
    for (int tt = 0; tt < kChunkSteps; ++tt) lamc[tt] = cur[(tt * 4 + g) * kRowS + Lay::kLam];
    // one DLA at a time: its 4 raw profiles, then its 7-tap broadening (voigt.c:297-299) into the
    // running product of the D broadened profiles
#pragma unroll
    for (int d = 0; d < D; ++d) {
      double rwv[kChunkSteps];
      raw_chunk3(lamc, afac[d], Nd[d], core_lim[d], wave_clamp, core_lds, wing_lds, exp_lds, rwv);
#pragma unroll
      for (int tt = 0; tt < kChunkSteps; ++tt) {
        double ab = win[d][(B + tt) % 10] * kInstrumentProfile[0];
#pragma unroll
        for (int i = 1; i < 6; ++i) ab = fma(win[d][(B + tt + i) % 10], kInstrumentProfile[i], ab);
        ab = fma(rwv[tt], kInstrumentProfile[6], ab);
        win[d][(B + tt + 6) % 10] = rwv[tt];
        abs_[tt] = d == 0 ? ab : abs_[tt] * ab;
      }
    }
    double wgs[kChunkSteps], wus[kChunkSteps];
    double rs[kChunkSteps], a2s[kChunkSteps], ds[kChunkSteps];
#pragma unroll
    for (int tt = 0; tt < kChunkSteps; ++tt) {
      const double* row = cur + (tt * 4 + g) * kRowS;
      const double y = row[Lay::kY], noise = row[Lay::kNoise], mu = row[Lay::kMu], om2 = row[Lay::kOmega2];
      const double ab = abs_[tt];
      // process_qsos.m:191-197 and log_mvnpdf_low_rank.m:11-15; masked / padding rows add nothing
      const double r = fma(-mu, ab, y);
      const double a2 = ab * ab;
      rs[tt] = r; a2s[tt] = a2; ds[tt] = fma(om2, a2, noise);
    }
    {
      double dinv[kChunkSteps], P;
      const bool p_ok = batch_rcp4_guarded(ds, dinv, P);
#pragma unroll
      for (int tt = 0; tt < kChunkSteps; ++tt) {
        const double rd = rs[tt] * dinv[tt];
        wgs[tt] = a2s[tt] * dinv[tt];
        wus[tt] = abs_[tt] * rd;
        q1 = fma(rs[tt], rd, q1);
      }
      if (p_ok) {
        pm *= P;
      } else {
#pragma unroll
        for (int tt = 0; tt < kChunkSteps; ++tt) {
          int ex;
          pm = frexp(pm * ds[tt], &ex);
          pe += ex;
        }
      }
    }
#pragma unroll
    for (int tt = 0; tt < kChunkSteps; ++tt) {
      const double wg = wgs[tt], wu = wus[tt];
      const double* brow = cur + (tt * 4 + g) * kRowS + (lane & 3) * kJS;
#pragma unroll
      for (int tp = 0; tp < kTiles; tp += 2) {
        if (tp + 1 < kTiles) {
          const double2 b = *reinterpret_cast<const double2*>(brow + tp);
          acc[tp] = __builtin_amdgcn_mfma_f64_4x4x4f64(tp < kGT ? wg : wu, b.x, acc[tp], 0, 0, 0);
          acc[tp + 1] = __builtin_amdgcn_mfma_f64_4x4x4f64(tp + 1 < kGT ? wg : wu, b.y, acc[tp + 1], 0, 0, 0);
        } else {
          acc[tp] = __builtin_amdgcn_mfma_f64_4x4x4f64(tp < kGT ? wg : wu, brow[tp], acc[tp], 0, 0, 0);
        }
      }
    }
    {
      int ex;
      pm = frexp(pm, &ex);
      pe += ex;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA for chunk c+1 landed
    __syncthreads();                                   // ... and everyone's; buffer c free again
  };
  using std::integral_constant;
  for (int c = 0; c < nchunks; c += 5) {
    chunk(c, integral_constant<int, 0>{});
    if (c + 1 >= nchunks) break;
    chunk(c + 1, integral_constant<int, 1>{});
    if (c + 2 >= nchunks) break;
    chunk(c + 2, integral_constant<int, 2>{});
    if (c + 3 >= nchunks) break;
    chunk(c + 3, integral_constant<int, 3>{});
    if (c + 4 >= nchunks) break;
    chunk(c + 4, integral_constant<int, 4>{});
  }

  // ---- segment combine and quad LDL^T epilogue, as likelihood_kernel
  q1 += __shfl_xor(q1, 16);
  q1 += __shfl_xor(q1, 32);
#pragma unroll
  for (int off2 = 16; off2 <= 32; off2 <<= 1) {
    const double pm2 = __shfl_xor(pm, off2);
    const int pe2 = __shfl_xor(pe, off2);
    int ex;
    pm = frexp(pm * pm2, &ex);
    pe += pe2 + ex;
  }
  const int jq = lane & 3, Q = lane >> 2;
  const int sig = 4 * (Q & 3) + (Q >> 2);
  const double qs = __shfl(q1, sig), dm = __shfl(pm, sig);
  const int de = __shfl(pe, sig);
  const int ex_s = __shfl((int)excl, sig);
  constexpr int NJJ = (K + 3) / 4;
  double A[NJJ][4 * NJJ], U[NJJ];
  fill_from_acc<K, 0>(A, U, acc, jq);
  bool bad;
  const double ll = ldl_factor<K>(A, U, qs, dm, (double)de + inf.de_shift, jq, inf.n, bad);
  const int64_t s2 = s_base + sig;
  if (jq == 0 && s2 < a.S) {
    if (bad && !ex_s) atomicOr(a.status, 1);
    a.sample_ll[q * a.ld + a.perm[s2]] = ex_s ? NAN : ll;
  }
}

// ---------------------------------------------------------------------------------------------
// Resampling: one 1,024-thread block per row (spectrum).  m = max of the non-NaN entries, w_i =
// exp(l_i - m) (NaN -> 0), C = inclusive prefix sum of w in caller order -- each thread sums a
// contiguous run, the runs' totals are scanned over the block -- kept in LDS up to GPDLA_RESAMPLE_LDS
// samples and in the global workspace beyond; then one binary search per sample for the smallest i
// with C_i > u_j C_{S-1}.  A zero-weight i can only be met through rounding at a run boundary: the
// search result then moves on to the next i with w_i > 0, and past the end back to the last one.
// The tail writes the base indices and the next level's chains [b] ++ chain_prev(b).
// ---------------------------------------------------------------------------------------------
constexpr int kResampleThreads = 1024;
constexpr int kResampleLds = GPDLA_RESAMPLE_LDS;

__global__ __launch_bounds__(kResampleThreads) void resample_kernel(ResampleArgs a) {
  __shared__ double s_c[kResampleLds];
  __shared__ double s_w[kResampleThreads / 64];
  const int row = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int64_t S = a.S;
  const double* ll = a.ll + (int64_t)row * a.ld;
  double* C = S <= kResampleLds ? s_c : a.cws + (int64_t)row * S;
  double m = -INFINITY, W = 0.0;
  if (!a.forced) {
    for (int64_t t = tid; t < S; t += kResampleThreads) m = fmax(m, ll[t]);  // fmax drops NaN
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
    if (lane == 0) s_w[wave] = m;
    __syncthreads();
    m = s_w[0];
#pragma unroll
    for (int w = 1; w < kResampleThreads / 64; ++w) m = fmax(m, s_w[w]);
    __syncthreads();
    const int64_t run = (S + kResampleThreads - 1) / kResampleThreads;
    const int64_t i0 = min((int64_t)tid * run, S), i1 = min(i0 + run, S);
    double loc = 0.0;
    for (int64_t i = i0; i < i1; ++i) {
      const double v = ll[i];
      loc += (v == v) ? exp(v - m) : 0.0;
    }
    double inc = loc;  // inclusive scan of the runs' totals over the block
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double t = __shfl_up(inc, o);
      if (lane >= o) inc += t;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    double before = 0.0;
    for (int w = 0; w < wave; ++w) before += s_w[w];
    __syncthreads();
    double runsum = before + (inc - loc);
    for (int64_t i = i0; i < i1; ++i) {
      const double v = ll[i];
      runsum += (v == v) ? exp(v - m) : 0.0;
      C[i] = runsum;
    }
    __threadfence_block();
    __syncthreads();
    W = C[S - 1];
  }
  const bool usable = a.forced || (W > 0.0 && W < INFINITY);
  auto weight = [&](int64_t i) {
    const double v = ll[i];
    return (v == v) ? exp(v - m) : 0.0;
  };
  for (int64_t j = tid; j < S; j += kResampleThreads) {
    int32_t b = -1;
    if (a.forced) {
      b = a.forced[(int64_t)row * S + j];
    } else if (usable) {
      const double t = a.u[j] * W;
      int64_t lo = 0, hi = S;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (C[mid] > t) hi = mid; else lo = mid + 1;
      }
      while (lo < S && !(weight(lo) > 0.0)) ++lo;
      if (lo >= S) {
        lo = S - 1;
        while (lo > 0 && !(weight(lo) > 0.0)) --lo;
      }
      b = (int32_t)lo;
    }
    a.base_inds[(int64_t)row * S + j] = b;
    if (a.chain_next) {
      int32_t* nx = a.chain_next + ((int64_t)row * S + j) * kMaxChain;
      const bool ok = b >= 0 && b < S;
#pragma unroll
      for (int i = 0; i < kMaxChain; ++i) {
        int32_t c = -1;
        if (ok && i == 0) c = b;
        else if (ok && i <= a.prev_len) c = a.chain_prev[((int64_t)row * S + b) * kMaxChain + i - 1];
        nx[i] = c;
      }
    }
  }
}

// log-mean-exp over the non-NaN samples of a level >= 2 (the too-close samples are NaN by design),
// minus the level's Occam penalty; NaN when no sample is finite
__global__ __launch_bounds__(kResampleThreads) void multi_reduce_kernel(MultiReduceArgs a) {
  __shared__ double s_w[kResampleThreads / 64];
  const int q = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const double* ll = a.sample_ll + (int64_t)q * a.ld;
  auto block_all = [&](double v, bool is_max) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double t = __shfl_xor(v, o);
      v = is_max ? fmax(v, t) : v + t;
    }
    if (lane == 0) s_w[wave] = v;
    __syncthreads();
    double r = s_w[0];
#pragma unroll
    for (int w = 1; w < kResampleThreads / 64; ++w) r = is_max ? fmax(r, s_w[w]) : r + s_w[w];
    __syncthreads();
    return r;
  };
  double m = -INFINITY, cnt = 0.0;
  for (int64_t t = tid; t < a.S; t += kResampleThreads) {
    const double v = ll[t];
    m = fmax(m, v);
    cnt += (v == v) ? 1.0 : 0.0;
  }
  m = block_all(m, true);
  cnt = block_all(cnt, false);
  double sum = 0.0;
  for (int64_t t = tid; t < a.S; t += kResampleThreads) {
    const double v = ll[t];
    if (v == v) sum += exp(v - m);
  }
  sum = block_all(sum, false);
  if (tid == 0) a.ll_dla[q] = cnt > 0.0 ? m + log(sum / cnt) - a.penalty : NAN;
}

template <int K, int D>
hipError_t launch_multi_level_kd(const MultiLevelArgs& a, hipStream_t s) {
  const int64_t blocks_x = (a.S + kSamplesPerBlock - 1) / kSamplesPerBlock;
  const int64_t nb = (blocks_x * a.q_count + 7) / 8 * 8;  // 1-D, padded for the XCD remap
  if (nb > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL((multi_level_kernel<K, D>), dim3((unsigned)nb), dim3(256), 0, s, a);
  return hipGetLastError();
}

template <int K>
hipError_t launch_multi_level_k(const MultiLevelArgs& a, hipStream_t s) {
  switch (a.chain_len) {
    case 1: return launch_multi_level_kd<K, 2>(a, s);
    case 2: return launch_multi_level_kd<K, 3>(a, s);
    case 3: return launch_multi_level_kd<K, 4>(a, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

#define GPDLA_FOR_EACH_RANK(X) X(4) X(8) X(10) X(12) X(16) X(20) X(24)

bool multi_level_supported(int K) {
#define X(k) if (K == k) return true;
  GPDLA_FOR_EACH_RANK(X)
#undef X
  return false;
}

hipError_t launch_multi_level(int K, const MultiLevelArgs& a, hipStream_t s) {
#define X(k) if (K == k) return launch_multi_level_k<k>(a, s);
  GPDLA_FOR_EACH_RANK(X)
#undef X
  return hipErrorInvalidValue;
}

hipError_t launch_resample(const ResampleArgs& a, hipStream_t s) {
  if (a.rows < 1 || a.S < 1) return hipSuccess;
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)a.rows), dim3(kResampleThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_multi_reduce(const MultiReduceArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(multi_reduce_kernel, dim3((unsigned)a.q_count), dim3(kResampleThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace gpdla
