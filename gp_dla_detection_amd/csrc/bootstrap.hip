// Bootstrap sample errors (include/gpdla.h "Bootstrap sample errors"): calc_cddf.py's
// resample / get_sample_errors (:126-184) written with multiplicities, so that B replicas of the sightline
// sample are one dense product sums[B x N] = counts[B x Q] rows[Q x N] instead of B gathers of Q rows.
//
//   bootstrap_counts_kernel  the draws: Philox4x64-10 keyed by the caller's seed, one counter per four draws,
//                            draw g of replica r = word g & 3 of counter (g >> 2, 0, r, 0); the drawn member
//                            of g's stratum is mulhi64(word, n_s); integer atomics into counts[r][spectrum]
//   bootstrap_rows_kernel    per spectrum the four planes catalog.cddf_moments accumulates (p A, p B - p p C,
//                            plain and moment), every product and difference rounded on its own (this file is
//                            compiled without FMA contraction), so they equal numpy's bit for bit
//   bootstrap_gemm_kernel    the product on v_mfma_f64_4x4x4_4b with gemm_f64.hip's probed operand maps
//                            (A[i][k] at lane 16 k + 4 b + i, B[k][j] at 16 k + 4 b + j, D[i][j] at 16 i + 4 b + j;
//                            the four blocks take the same A and four different B: 4 replicas x 16 columns per
//                            instruction).  M = replicas, N = columns, K = spectra.  A block of kBootWaves waves
//                            is 32 kBootWaves replicas x 128 columns, a wave 32 x 128 = 8 x 8 instructions per
//                            K step of 4 on 8 A and 8 B registers.  K runs in stages of kBootStageK spectra
//                            through LDS, double-buffered with the next stage's global loads in registers
//                            while this one's MFMAs run, one barrier per stage.  The counts are read as int32
//                            (half the A traffic) and converted on their way into LDS, in the layout a lane
//                            reads its 8 A operands of a K step from as 64 contiguous bytes: [wave][k][32]
//                            with replica 4 g + i of the wave at 8 i + (g ^ 2 (k / 4 & 3)): the XOR spreads the
//                            four ds_write_b64 of a loaded int4 (four k, one replica) over the banks, and is
//                            undone for free when the unrolled K step picks its registers.  Rows are
//                            [k][128 + 8] (the pad keeps a K step's four rows on different banks); MFMA column
//                            (eg, lane j16) is column 32 (eg / 2) + 2 j16 + (eg & 1) of the tile, so the 16
//                            lanes of one ds_read_b128 read 256 contiguous bytes.  (With 8 i + g and column
//                            8 j16 + eg, one counter pass showed 71 % of the LDS cycles in bank conflicts.)
//                            Both operands live in device buffers padded with zeros to whole tiles, stages
//                            and 16-byte rows, so the kernel has no bounds test: a padded replica, column or
//                            spectrum adds exact zeros.  Split-K: block z takes the spectra of slice z
//                            (kBootKSlice each) and writes its own partial tile.
//   bootstrap_reduce_kernel  sums = partial 0 + partial 1 + ... in ascending slice order (no atomics)
// The order of additions into one sum is therefore: within a slice the K steps ascending (four spectra per
// step, in the matrix core's own fixed order), then the slices ascending -- a function of Q, kBootStageK and
// kBootKSlice alone, the same for every replica wherever it sits in whichever call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/gpdla.h"
#include "internal.h"

#pragma clang fp contract(off)

namespace gpdla {
namespace {

constexpr int kBootWaves = GPDLA_BOOT_WAVES;
constexpr int kBM = 32 * kBootWaves;            // replicas per block
constexpr int kBN = 128;                        // columns per block
constexpr int kBK = GPDLA_BOOT_STAGE_K;         // spectra per stage
constexpr int kBootKSlice = GPDLA_BOOT_KSLICE;  // spectra per split-K slice
constexpr int kBootMaxChunk = GPDLA_BOOT_MAX_CHUNK;
constexpr int kBootThreads = 64 * kBootWaves;
constexpr int kBRowB = kBN + 8;                 // LDS row stride of the rows operand (doubles)
constexpr int kBStageB = kBK * kBRowB;
constexpr int kBStageA = kBootWaves * kBK * 32;
constexpr int kBStage = kBStageB + kBStageA;
static_assert(kBK % 4 == 0 && kBK >= 4, "a stage is whole K steps");
static_assert(kBootKSlice % kBK == 0 && kBootKSlice >= kBK, "a slice is whole stages");
static_assert(kBootMaxChunk % kBM == 0 && kBootMaxChunk >= kBM, "a chunk is whole block rows");
static_assert(kBootMaxChunk <= 65535, "replicas are a grid's y extent");
static_assert((kBM * kBK / 4) % kBootThreads == 0 && (kBK * kBN / 2) % kBootThreads == 0, "whole loads per thread");
using i32x4 = int __attribute__((ext_vector_type(4)));
using f64x2 = double __attribute__((ext_vector_type(2)));
constexpr int kALoads = kBM * kBK / 4 / kBootThreads;   // int4 loads per thread and stage
constexpr int kBLoads = kBK * kBN / 2 / kBootThreads;   // double2 loads per thread and stage

// ---- Philox4x64-10 (Salmon et al. 2011; Random123's constants) --------------------------------------------
__device__ __forceinline__ void philox4x64_10(uint64_t c0, uint64_t c1, uint64_t c2, uint64_t c3, uint64_t k0,
                                              uint64_t k1, uint64_t out[4]) {
  constexpr uint64_t kM0 = 0xD2E7470EE14C6C93ull, kM1 = 0xCA5A826395121157ull;
  constexpr uint64_t kW0 = 0x9E3779B97F4A7C15ull, kW1 = 0xBB67AE8584CAA73Bull;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t hi0 = __umul64hi(kM0, c0), lo0 = kM0 * c0;
    const uint64_t hi1 = __umul64hi(kM1, c2), lo1 = kM1 * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += kW0; k1 += kW1;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

struct BootCountsArgs {
  uint64_t k0, k1;
  int64_t replica0;              // the replica number of grid row 0
  int64_t G;                     // draws per replica = members
  int32_t ns;
  const int64_t* soff;           // device [ns + 1]
  const int32_t* members;        // device [G]
  int32_t* counts;               // device [replicas][ldq], zeroed
  int64_t ldq;
};

__global__ __launch_bounds__(256) void bootstrap_counts_kernel(BootCountsArgs a) {
  const int64_t quad = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t g0 = quad * 4;
  if (g0 >= a.G) return;
  uint64_t w[4];
  philox4x64_10((uint64_t)quad, 0, (uint64_t)(a.replica0 + blockIdx.y), 0, a.k0, a.k1, w);
  int32_t* row = a.counts + (int64_t)blockIdx.y * a.ldq;
  int lo = 0, hi = a.ns - 1;      // the stratum of g0: the last s with soff[s] <= g0
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.soff[mid] <= g0) lo = mid; else hi = mid - 1;
  }
  int s = lo;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t g = g0 + j;
    if (g >= a.G) break;
    while (g >= a.soff[s + 1]) ++s;          // strata are non-empty and g < soff[ns]
    const int64_t base = a.soff[s], n = a.soff[s + 1] - base;
    const int64_t pick = (int64_t)__umul64hi(w[j], (uint64_t)n);
    atomicAdd(&row[a.members[base + pick]], 1);
  }
}

struct BootRowsArgs {
  const double* planes;          // [rows][D][5][nbins]
  const double* p;               // [rows]
  const double* P;               // [rows][D] or nullptr
  const uint8_t* keep;           // [rows] or nullptr
  int32_t D, nbins;
  double thresh;
  double* rows;                  // [rows][ld]
  int64_t ld;
};

__global__ __launch_bounds__(256) void bootstrap_rows_kernel(BootRowsArgs a) {
  const int64_t q = blockIdx.x;
  const double p = a.p[q];
  const bool use = p > a.thresh && (!a.keep || a.keep[q]);      // a NaN p compares false
  double* out = a.rows + q * a.ld;
  const int nb = a.nbins;
  for (int bin = threadIdx.x; bin < nb; bin += 256) {
#pragma unroll
    for (int mom = 0; mom < 2; ++mom) {
      const int ia = mom ? 2 : 0, ib = mom ? 3 : 0, ic = mom ? 4 : 1;   // PLANE_PI.. of catalog.py
      double m = 0.0, v = 0.0;
      if (use && !a.P) {
        const double* pl = a.planes + q * 5 * nb;
        m = p * pl[ia * nb + bin];
        const double t1 = p * pl[ib * nb + bin], pp = p * p;
        v = t1 - pp * pl[ic * nb + bin];
      } else if (use) {
        for (int d = 0; d < a.D; ++d) {
          const double Pd = a.P[q * a.D + d];
          if (Pd != Pd) continue;
          const double* pl = a.planes + (q * a.D + d) * 5 * nb;
          m = m + Pd * pl[ia * nb + bin];
          const double t1 = Pd * pl[ib * nb + bin], pp = Pd * Pd;
          v = v + (t1 - pp * pl[ic * nb + bin]);
        }
      }
      out[(2 * mom) * nb + bin] = m;
      out[(2 * mom + 1) * nb + bin] = v;
    }
  }
}

struct BootGemmArgs {
  const int32_t* counts;         // [Mpad][ldq], zero beyond the replicas and the spectra
  const double* rows;            // [Kpad][ldn], zero beyond the spectra and the columns
  double* part;                  // [slices][Mpad][ldn]
  int64_t ldq, ldn, Mpad, Kpad;
};

__global__ __launch_bounds__(kBootThreads, 8 / kBootWaves) void bootstrap_gemm_kernel(BootGemmArgs a) {
  __shared__ __attribute__((aligned(16))) double lds[2 * kBStage];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kk = lane >> 4, i4 = lane & 3, j16 = lane & 15;
  const int64_t m0 = (int64_t)blockIdx.y * kBM, n0 = (int64_t)blockIdx.x * kBN;
  const int64_t k_begin = (int64_t)blockIdx.z * kBootKSlice;
  const int64_t k_end = k_begin + kBootKSlice < a.Kpad ? k_begin + kBootKSlice : a.Kpad;
  const int nstage = (int)((k_end - k_begin) / kBK);

  // global pieces of a stage.  Counts: int4 number e = tid + kBootThreads r covers replica e / (kBK / 4) of
  // the tile and spectra 4 (e % (kBK / 4)) ..+3.  Rows: double2 number e covers spectrum e / 64, columns 2 (e % 64) ..+1
  i32x4 ra[kALoads];
  f64x2 rb[kBLoads];
  auto fetch = [&](int c) {
    const int64_t k0 = k_begin + (int64_t)c * kBK;
#pragma unroll
    for (int r = 0; r < kALoads; ++r) {
      const int e = tid + kBootThreads * r;
      ra[r] = *reinterpret_cast<const i32x4*>(a.counts + (m0 + e / (kBK / 4)) * a.ldq + k0 + 4 * (e % (kBK / 4)));
    }
#pragma unroll
    for (int r = 0; r < kBLoads; ++r) {
      const int e = tid + kBootThreads * r;
      rb[r] = *reinterpret_cast<const f64x2*>(a.rows + (k0 + e / 64) * a.ldn + n0 + 2 * (e % 64));
    }
  };
  auto stash = [&](int buf) {
    double* Bb = lds + buf * kBStage;
    double* Ab = Bb + kBStageB;
#pragma unroll
    for (int r = 0; r < kALoads; ++r) {
      const int e = tid + kBootThreads * r;
      const int m = e / (kBK / 4), kq = e % (kBK / 4), k = 4 * kq;
      double* dst = Ab + ((m >> 5) * kBK + k) * 32 + 8 * (m & 3) + (((m & 31) >> 2) ^ (2 * (kq & 3)));
      dst[0] = (double)ra[r].x; dst[32] = (double)ra[r].y; dst[64] = (double)ra[r].z; dst[96] = (double)ra[r].w;
    }
#pragma unroll
    for (int r = 0; r < kBLoads; ++r) {
      const int e = tid + kBootThreads * r;
      *reinterpret_cast<f64x2*>(Bb + (e / 64) * kBRowB + 2 * (e % 64)) = rb[r];
    }
  };

  double acc[8][8];
#pragma unroll
  for (int g = 0; g < 8; ++g)
#pragma unroll
    for (int eg = 0; eg < 8; ++eg) acc[g][eg] = 0.0;

  fetch(0);
  stash(0);
  __syncthreads();
  for (int c = 0; c < nstage; ++c) {
    const int buf = c & 1;
    if (c + 1 < nstage) fetch(c + 1);
    const double* Bb = lds + buf * kBStage;
    const double* Ab = Bb + kBStageB + wave * kBK * 32;
#pragma unroll
    for (int ks = 0; ks < kBK / 4; ++ks) {
      const f64x2* ap = reinterpret_cast<const f64x2*>(Ab + (4 * ks + kk) * 32 + 8 * i4);
      const f64x2* bp = reinterpret_cast<const f64x2*>(Bb + (4 * ks + kk) * kBRowB + 2 * j16);
      double Al[8], Av[8], Bv[8];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f64x2 va = ap[q], vb = bp[16 * q];
        Al[2 * q] = va.x; Al[2 * q + 1] = va.y;
        Bv[2 * q] = vb.x; Bv[2 * q + 1] = vb.y;
      }
#pragma unroll
      for (int g = 0; g < 8; ++g) Av[g] = Al[g ^ (2 * (ks & 3))];     // undo the stash's swizzle
#pragma unroll
      for (int g = 0; g < 8; ++g)
#pragma unroll
        for (int eg = 0; eg < 8; ++eg) acc[g][eg] = __builtin_amdgcn_mfma_f64_4x4x4f64(Av[g], Bv[eg], acc[g][eg], 0, 0, 0);
    }
    if (c + 1 < nstage) stash(buf ^ 1);    // everyone left that buffer at the last barrier
    __syncthreads();
  }
  // D: this lane holds replica 4 g + (lane >> 4) of the wave and columns 32 q + 2 j16 + 0..1, q = 0..3 (padded
  // buffer: no bound)
  double* pt = a.part + ((int64_t)blockIdx.z * a.Mpad + m0 + wave * 32 + kk) * a.ldn + n0 + 2 * j16;
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    f64x2* dst = reinterpret_cast<f64x2*>(pt + (int64_t)(4 * g) * a.ldn);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f64x2 v;
      v.x = acc[g][2 * q]; v.y = acc[g][2 * q + 1];
      dst[16 * q] = v;
    }
  }
}

struct BootReduceArgs {
  const double* part;            // [slices][Mpad][ldn]
  double* sums;                  // [B][N]
  int64_t ldn, Mpad, N, B;
  int32_t slices;
};

__global__ __launch_bounds__(256) void bootstrap_reduce_kernel(BootReduceArgs a) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (c >= a.N) return;
  const double* p = a.part + b * a.ldn + c;
  double s = p[0];
  for (int z = 1; z < a.slices; ++z) s = s + p[(int64_t)z * a.Mpad * a.ldn];
  a.sums[b * a.N + c] = s;
}

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// the device buffers of a sums run: the padded rows, and per replica chunk the padded counts, the split-K
// partials and the compact sums
struct BootRun {
  int64_t Q = 0, N = 0, Kpad = 0, ldn = 0, ldq = 0, chunk = 0;
  int slices = 0;
  DeviceStage st;
  size_t o_rows = 0, o_counts = 0, o_part = 0, o_sums = 0;

  // carve for B replicas (at most kBootMaxChunk, fewer if memory is short); the caller carves its own after this
  int plan(int64_t B, int64_t Q_, int64_t N_) {
    Q = Q_; N = N_;
    Kpad = round_up(Q, kBK); ldq = Kpad; ldn = round_up(N, kBN);
    slices = (int)((Kpad + kBootKSlice - 1) / kBootKSlice);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return set_error(GPDLA_EDEVICE, "bootstrap: hipMemGetInfo failed");
    const double rows_b = (double)Kpad * ldn * 8;
    const double per_rep = (double)ldq * 4 + (double)slices * ldn * 8 + (double)N * 8;
    const double room = 0.8 * (double)free_b - rows_b - (double)(64u << 20) - (double)Q * 12;
    int64_t fit = room > 0 ? (int64_t)(room / per_rep) / kBM * kBM : 0;
    chunk = std::min<int64_t>({fit, (int64_t)kBootMaxChunk, round_up(B, kBM)});
    if (chunk < kBM)
      return set_error(GPDLA_ENOMEM, "bootstrap: %.1f GiB of rows and one block of replicas do not fit in %.1f GiB free",
                       rows_b / 1073741824.0, (double)free_b / 1073741824.0);
    o_rows = st.carve((size_t)Kpad * ldn * 8);
    o_counts = st.carve((size_t)chunk * ldq * 4);
    o_part = st.carve((size_t)slices * chunk * ldn * 8);
    o_sums = st.carve((size_t)chunk * N * 8);
    return GPDLA_OK;
  }
  hipError_t upload_rows(const double* rows) {
    if (hipError_t e = hipMemset(st.d + o_rows, 0, (size_t)Kpad * ldn * 8)) return e;
    return hipMemcpy2D(st.d + o_rows, (size_t)ldn * 8, rows, (size_t)N * 8, (size_t)N * 8, (size_t)Q, hipMemcpyHostToDevice);
  }
  hipError_t zero_counts() { return hipMemset(st.d + o_counts, 0, (size_t)chunk * ldq * 4); }
  // product and reduction of the chunk's first bc replicas, then their sums to the host
  hipError_t run(int64_t bc, double* sums_host, LaunchTimes& lt) {
    const int64_t Mpad = round_up(bc, kBM);
    BootGemmArgs ga{st.ptr<const int32_t>(o_counts), st.ptr<const double>(o_rows), st.ptr<double>(o_part), ldq, ldn, Mpad, Kpad};
    lt.before();
    hipLaunchKernelGGL(bootstrap_gemm_kernel, dim3((unsigned)(ldn / kBN), (unsigned)(Mpad / kBM), (unsigned)slices),
                       dim3(kBootThreads), 0, nullptr, ga);
    if (hipError_t e = hipGetLastError()) return e;
    lt.after();
    BootReduceArgs ra{st.ptr<const double>(o_part), st.ptr<double>(o_sums), ldn, Mpad, N, bc, slices};
    lt.before();
    hipLaunchKernelGGL(bootstrap_reduce_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)bc), dim3(256), 0, nullptr, ra);
    if (hipError_t e = hipGetLastError()) return e;
    lt.after();
    return st.download(sums_host, o_sums, (size_t)bc * N * 8);
  }
};

int validate_boot_spec(int64_t Q, const gpdla_bootstrap_spec* spec) {
  if (!spec) return set_error(GPDLA_EINVAL, "bootstrap: null spec");
  if (Q < 1 || Q > INT32_MAX - kBK) return set_error(GPDLA_EINVAL, "bootstrap: Q=%lld", (long long)Q);
  if (spec->num_replicas < 1) return set_error(GPDLA_EINVAL, "bootstrap: num_replicas=%lld", (long long)spec->num_replicas);
  if (spec->first_replica < 0) return set_error(GPDLA_EINVAL, "bootstrap: first_replica=%lld", (long long)spec->first_replica);
  if (spec->num_strata < 1 || !spec->stratum_offsets || !spec->members)
    return set_error(GPDLA_EINVAL, "bootstrap: num_strata=%d or a null stratum array", spec->num_strata);
  if (spec->stratum_offsets[0] != 0) return set_error(GPDLA_EINVAL, "bootstrap: stratum_offsets[0] must be 0");
  for (int s = 0; s < spec->num_strata; ++s)
    if (spec->stratum_offsets[s + 1] <= spec->stratum_offsets[s])
      return set_error(GPDLA_EINVAL, "bootstrap: stratum %d is empty", s);
  const int64_t G = spec->stratum_offsets[spec->num_strata];
  if (G > Q) return set_error(GPDLA_EINVAL, "bootstrap: %lld members of %lld spectra: one is listed twice", (long long)G, (long long)Q);
  std::vector<uint8_t> seen((size_t)Q, 0);
  for (int64_t g = 0; g < G; ++g) {
    const int64_t m = spec->members[g];
    if (m < 0 || m >= Q) return set_error(GPDLA_EINVAL, "bootstrap: members[%lld] = %lld outside 0..%lld", (long long)g, (long long)m, (long long)Q - 1);
    if (seen[(size_t)m]) return set_error(GPDLA_EINVAL, "bootstrap: spectrum %lld is listed twice", (long long)m);
    seen[(size_t)m] = 1;
  }
  return GPDLA_OK;
}

int validate_rows(const double* rows, int64_t Q, int64_t N) {
  if (!rows) return set_error(GPDLA_EINVAL, "bootstrap: null rows");
  if (N < 1 || N > (1 << 24)) return set_error(GPDLA_EINVAL, "bootstrap: N=%lld", (long long)N);
  for (int64_t i = 0; i < Q * N; ++i)
    if (!std::isfinite(rows[i]))
      return set_error(GPDLA_EINVAL, "bootstrap: rows[%lld][%lld] = %g is not finite", (long long)(i / N), (long long)(i % N), rows[i]);
  return GPDLA_OK;
}

// the strata on the device, and the draws of replicas r0 .. r0 + bc into zeroed counts
struct BootDraws {
  size_t o_soff = 0, o_mem = 0;
  int64_t G = 0;
  void carve(DeviceStage& st, const gpdla_bootstrap_spec* spec) {
    G = spec->stratum_offsets[spec->num_strata];
    o_soff = st.carve((size_t)(spec->num_strata + 1) * 8);
    o_mem = st.carve((size_t)G * 4);
  }
  hipError_t upload(DeviceStage& st, const gpdla_bootstrap_spec* spec) {
    if (hipError_t e = st.upload(o_soff, spec->stratum_offsets, (size_t)(spec->num_strata + 1) * 8)) return e;
    return st.upload(o_mem, spec->members, (size_t)G * 4);
  }
  hipError_t launch(DeviceStage& st, const gpdla_bootstrap_spec* spec, int64_t r0, int64_t bc, int32_t* counts, int64_t ldq,
                    LaunchTimes& lt) {
    BootCountsArgs ca{spec->seed[0], spec->seed[1], r0, G, spec->num_strata, st.ptr<const int64_t>(o_soff),
                      st.ptr<const int32_t>(o_mem), counts, ldq};
    const int64_t quads = (G + 3) / 4;
    lt.before();
    hipLaunchKernelGGL(bootstrap_counts_kernel, dim3((unsigned)((quads + 255) / 256), (unsigned)bc), dim3(256), 0, nullptr, ca);
    if (hipError_t e = hipGetLastError()) return e;
    lt.after();
    return hipSuccess;
  }
};

}  // namespace
}  // namespace gpdla

using namespace gpdla;

extern "C" {

int gpdla_bootstrap_tiling(int32_t* tile_m, int32_t* tile_n, int32_t* stage_k, int32_t* k_slice, int32_t* max_chunk) {
  if (!tile_m || !tile_n || !stage_k || !k_slice || !max_chunk) return set_error(GPDLA_EINVAL, "null argument");
  *tile_m = kBM; *tile_n = kBN; *stage_k = kBK; *k_slice = kBootKSlice; *max_chunk = kBootMaxChunk;
  return GPDLA_OK;
}

int gpdla_bootstrap_counts_i32(int32_t device, int64_t Q, const gpdla_bootstrap_spec* spec, int32_t* counts) {
  int rc = validate_boot_spec(Q, spec);
  if (rc) return rc;
  if (!counts) return set_error(GPDLA_EINVAL, "bootstrap: null counts");
  if ((rc = check_device(device))) return rc;
  LaunchTimes& lt = launch_times();
  lt.reset();
  HIP_TRY(hipSetDevice(device));
  const int64_t B = spec->num_replicas, chunk = std::min<int64_t>(B, kBootMaxChunk);
  DeviceStage st;
  BootDraws dr;
  dr.carve(st, spec);
  const size_t o_c = st.carve((size_t)chunk * Q * 4);
  HIP_TRY_IN("bootstrap", st.alloc());
  HIP_TRY_IN("bootstrap", dr.upload(st, spec));
  for (int64_t b0 = 0; b0 < B; b0 += chunk) {
    const int64_t bc = std::min(chunk, B - b0);
    HIP_TRY_IN("bootstrap", hipMemset(st.d + o_c, 0, (size_t)bc * Q * 4));
    HIP_TRY_IN("bootstrap", dr.launch(st, spec, spec->first_replica + b0, bc, st.ptr<int32_t>(o_c), Q, lt));
    HIP_TRY_IN("bootstrap", st.download(counts + b0 * Q, o_c, (size_t)bc * Q * 4));
  }
  lt.finish();
  return GPDLA_OK;
}

int gpdla_bootstrap_rows_f64(int32_t device, const double* planes, int32_t D, const double* p_dlas,
                             const double* level_posteriors, const uint8_t* keep, int64_t Q, int32_t nz, int32_t nn,
                             double p_thresh_spec, double* rows, int64_t ld_rows) {
  if (!planes || !p_dlas || !rows) return set_error(GPDLA_EINVAL, "bootstrap rows: null argument");
  if (Q < 1 || Q > INT32_MAX) return set_error(GPDLA_EINVAL, "bootstrap rows: Q=%lld", (long long)Q);
  if (D < 1 || D > GPDLA_MAX_DLAS || (!level_posteriors && D != 1))
    return set_error(GPDLA_EINVAL, "bootstrap rows: D=%d (1..%d; 1 without level_posteriors)", D, GPDLA_MAX_DLAS);
  if (nz < 1 || nn < 1 || (int64_t)nz * nn > GPDLA_SUMMARY_MAX_BINS)
    return set_error(GPDLA_EINVAL, "bootstrap rows: grid %d x %d (1..%d bins)", nz, nn, GPDLA_SUMMARY_MAX_BINS);
  const int64_t nb = (int64_t)nz * nn;
  if (ld_rows < 4 * nb) return set_error(GPDLA_EINVAL, "bootstrap rows: ld_rows=%lld below %lld", (long long)ld_rows, (long long)(4 * nb));
  int rc = check_device(device);
  if (rc) return rc;
  LaunchTimes& lt = launch_times();
  lt.reset();
  HIP_TRY(hipSetDevice(device));
  // spectra in chunks of at most 64 MiB of planes
  const size_t per_q = (size_t)D * 5 * nb * 8;
  const int64_t qc = std::max<int64_t>(1, std::min<int64_t>(Q, (int64_t)((64u << 20) / per_q)));
  DeviceStage st;
  const size_t o_pl = st.carve((size_t)qc * per_q), o_p = st.carve((size_t)qc * 8), o_P = st.carve((size_t)qc * D * 8);
  const size_t o_k = st.carve((size_t)qc), o_r = st.carve((size_t)qc * 4 * nb * 8);
  HIP_TRY_IN("bootstrap rows", st.alloc());
  for (int64_t q0 = 0; q0 < Q; q0 += qc) {
    const int64_t n = std::min(qc, Q - q0);
    HIP_TRY_IN("bootstrap rows", st.upload(o_pl, planes + q0 * D * 5 * nb, (size_t)n * per_q));
    HIP_TRY_IN("bootstrap rows", st.upload(o_p, p_dlas + q0, (size_t)n * 8));
    if (level_posteriors) HIP_TRY_IN("bootstrap rows", st.upload(o_P, level_posteriors + q0 * D, (size_t)n * D * 8));
    if (keep) HIP_TRY_IN("bootstrap rows", st.upload(o_k, keep + q0, (size_t)n));
    BootRowsArgs ra{st.ptr<const double>(o_pl), st.ptr<const double>(o_p), level_posteriors ? st.ptr<const double>(o_P) : nullptr,
                    keep ? st.ptr<const uint8_t>(o_k) : nullptr, D, (int32_t)nb, p_thresh_spec, st.ptr<double>(o_r), 4 * nb};
    lt.before();
    hipLaunchKernelGGL(bootstrap_rows_kernel, dim3((unsigned)n), dim3(256), 0, nullptr, ra);
    HIP_TRY_IN("bootstrap rows", hipGetLastError());
    lt.after();
    HIP_TRY_IN("bootstrap rows", hipMemcpy2D(rows + q0 * ld_rows, (size_t)ld_rows * 8, st.d + o_r, (size_t)4 * nb * 8,
                                             (size_t)4 * nb * 8, (size_t)n, hipMemcpyDeviceToHost));
  }
  lt.finish();
  return GPDLA_OK;
}

int gpdla_bootstrap_sums_f64(int32_t device, const int32_t* counts, const double* rows, int64_t B, int64_t Q, int64_t N,
                             double* sums) {
  if (!counts || !sums) return set_error(GPDLA_EINVAL, "bootstrap: null argument");
  if (B < 1 || Q < 1 || Q > INT32_MAX - kBK) return set_error(GPDLA_EINVAL, "bootstrap: B=%lld Q=%lld", (long long)B, (long long)Q);
  int rc = validate_rows(rows, Q, N);
  if (rc) return rc;
  for (int64_t i = 0; i < B * Q; ++i)
    if (counts[i] < 0)
      return set_error(GPDLA_EINVAL, "bootstrap: counts[%lld][%lld] = %d is negative", (long long)(i / Q), (long long)(i % Q), counts[i]);
  if ((rc = check_device(device))) return rc;
  LaunchTimes& lt = launch_times();
  lt.reset();
  HIP_TRY(hipSetDevice(device));
  BootRun run;
  if ((rc = run.plan(B, Q, N))) return rc;
  HIP_TRY_IN("bootstrap", run.st.alloc());
  HIP_TRY_IN("bootstrap", run.upload_rows(rows));
  for (int64_t b0 = 0; b0 < B; b0 += run.chunk) {
    const int64_t bc = std::min(run.chunk, B - b0);
    HIP_TRY_IN("bootstrap", run.zero_counts());
    HIP_TRY_IN("bootstrap", hipMemcpy2D(run.st.d + run.o_counts, (size_t)run.ldq * 4, counts + b0 * Q, (size_t)Q * 4, (size_t)Q * 4,
                                        (size_t)bc, hipMemcpyHostToDevice));
    HIP_TRY_IN("bootstrap", run.run(bc, sums + b0 * N, lt));
  }
  lt.finish();
  return GPDLA_OK;
}

int gpdla_bootstrap_f64(int32_t device, const double* rows, int64_t Q, int64_t N, const gpdla_bootstrap_spec* spec,
                        double* sums) {
  int rc = validate_boot_spec(Q, spec);
  if (rc) return rc;
  if (!sums) return set_error(GPDLA_EINVAL, "bootstrap: null sums");
  if ((rc = validate_rows(rows, Q, N))) return rc;
  if ((rc = check_device(device))) return rc;
  LaunchTimes& lt = launch_times();
  lt.reset();
  HIP_TRY(hipSetDevice(device));
  const int64_t B = spec->num_replicas;
  BootRun run;
  if ((rc = run.plan(B, Q, N))) return rc;
  BootDraws dr;
  dr.carve(run.st, spec);
  HIP_TRY_IN("bootstrap", run.st.alloc());
  HIP_TRY_IN("bootstrap", run.upload_rows(rows));
  HIP_TRY_IN("bootstrap", dr.upload(run.st, spec));
  for (int64_t b0 = 0; b0 < B; b0 += run.chunk) {
    const int64_t bc = std::min(run.chunk, B - b0);
    HIP_TRY_IN("bootstrap", run.zero_counts());
    HIP_TRY_IN("bootstrap", dr.launch(run.st, spec, spec->first_replica + b0, bc, run.st.ptr<int32_t>(run.o_counts), run.ldq, lt));
    HIP_TRY_IN("bootstrap", run.run(bc, sums + b0 * N, lt));
  }
  lt.finish();
  return GPDLA_OK;
}

}  // extern "C"
