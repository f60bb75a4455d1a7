// The distribution of a weighted sum of independent counts on a lattice (include/gpdla.h "Count mixture";
// DESIGN.md section 20): what calc_cddf.py's _get_omega_confidence_intervals (:562-636) builds as a list of
// (value, probability) atoms, here a chain of sparse convolutions on a dense fp64 lattice.
//
// A problem is a list of stages, a stage a sparse pmf of taps (shift_i, p_i) with non-decreasing shifts.  The
// state starts as delta at cell 0 and two buffers ping-pong (stage s reads buffer s & 1, writes the other).
//
//   mix_stage_kernel   next[g] = sum_i p_i cur[g - shift_i]: one FMA chain per cell in ascending i, terms with
//                      g < shift_i absent.  A workgroup takes GPDLA_MIX_TILE contiguous cells, thread t the cells
//                      tile + t, tile + 256 + t, ..., so for a fixed tap a wave reads 64 contiguous doubles; the
//                      taps come through LDS in passes of GPDLA_MIX_TAPS, the chains carried across the passes in
//                      registers, so a cell's order of operations is its stage's tap order whatever the constants.
//                      blockIdx.y is the problem; one launch per stage index, over the longest live prefix of the
//                      problems that have that stage (after stage s no cell above the summed largest shifts can be
//                      non-zero); a workgroup past its own problem's prefix, or of a problem without the stage, exits.
//   mix_scan_kernel    inclusive prefix sum of the final lattice into the buffer it did not end in, one workgroup
//                      per problem: GPDLA_MIX_TILE cells a step, each thread its own run of consecutive cells, the
//                      256 run totals summed left to right by one lane, the carry added last.  The order depends on
//                      the cell index and the tile alone, and the cdf never decreases (every cell's value and its
//                      right neighbour's differ by adding a non-negative term to the same partial sum).
//   mix_search_kernel  per level: the first cell with cdf >= level; the first occupied cell strictly above the
//                      first cell with cdf > level, clamped to the last occupied cell (calc_cddf.py's "one past"
//                      upper end, :986-1019 and :634-635).
// All terms are non-negative, so nothing cancels.  Plain fp64 VALU; this file needs no MFMA.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "../../include/gpdla.h"
#include "internal.h"

namespace gpdla {
namespace {

constexpr int kMixThreads = 256;
constexpr int kMixSearchThreads = 1024;                   // mix_search_kernel: one load in flight per thread, so the most a workgroup holds
constexpr int kMixTile = GPDLA_MIX_TILE;
constexpr int kMixTaps = GPDLA_MIX_TAPS;
constexpr int kMixPer = kMixTile / kMixThreads;          // cells per thread and tile
constexpr int kMixMaxLevels = GPDLA_MIX_MAX_LEVELS;
static_assert(kMixTile % kMixThreads == 0 && kMixPer >= 1 && kMixPer <= 16, "GPDLA_MIX_TILE: 256 .. 4096 in steps of 256");
static_assert(kMixTaps >= 1 && kMixTaps <= 2048, "GPDLA_MIX_TAPS: 12 bytes of LDS per tap");

struct MixArgs {
  const double* probs;          // [taps]
  const int32_t* shifts;        // [taps]
  const int64_t* tap_off;       // [stages + 1]
  const int64_t* stage_off;     // [problems + 1]
  const int32_t* live;          // [stages]: cells that can be non-zero after the stage (1 + summed largest shifts)
  double* buf[2];               // [problems][cells] each
  int64_t cells;
  int32_t stage;                // mix_stage_kernel: the stage index of this launch
  const double* levels;         // [nl]
  int32_t nl;
  int32_t* lower;               // [problems][nl]
  int32_t* upper;
  double* mass;                 // [problems]
};

__global__ __launch_bounds__(kMixThreads) void mix_stage_kernel(MixArgs a) {
  __shared__ double s_p[kMixTaps];
  __shared__ int32_t s_sh[kMixTaps];
  const int64_t p = blockIdx.y;
  const int64_t s0 = a.stage_off[p];
  if ((int64_t)a.stage >= a.stage_off[p + 1] - s0) return;
  const int64_t sg = s0 + a.stage;
  const int32_t live = a.live[sg];
  const int32_t g0 = (int32_t)blockIdx.x * kMixTile;
  if (g0 >= live) return;
  const int tid = threadIdx.x;
  const double* cur = a.buf[a.stage & 1] + p * a.cells;
  double* nxt = a.buf[(a.stage + 1) & 1] + p * a.cells;
  const int64_t t0 = a.tap_off[sg];
  const int64_t nt = a.tap_off[sg + 1] - t0;
  const int32_t g_top = min(g0 + kMixTile, live) - 1;      // the tile's last live cell
  double acc[kMixPer];
#pragma unroll
  for (int j = 0; j < kMixPer; ++j) acc[j] = 0.0;
  for (int64_t base = 0; base < nt; base += kMixTaps) {
    const int n = (int)min((int64_t)kMixTaps, nt - base);
    __syncthreads();
    for (int i = tid; i < n; i += kMixThreads) {
      s_p[i] = a.probs[t0 + base + i];
      s_sh[i] = a.shifts[t0 + base + i];
    }
    __syncthreads();
    for (int i = 0; i < n; ++i) {
      const int32_t sh = s_sh[i];
      if (sh > g_top) break;                               // shifts never decrease: no later tap reaches the tile
      const double pi = s_p[i];
#pragma unroll
      for (int j = 0; j < kMixPer; ++j) {
        const int32_t g = g0 + j * kMixThreads + tid;
        if (g >= sh && g <= g_top) acc[j] = fma(pi, cur[g - sh], acc[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kMixPer; ++j) {
    const int32_t g = g0 + j * kMixThreads + tid;
    if (g <= g_top) nxt[g] = acc[j];
  }
}

// the live prefix of a problem's final lattice and the buffer it is in
__device__ __forceinline__ int32_t final_lattice(const MixArgs& a, int64_t p, int* which) {
  const int64_t s0 = a.stage_off[p], ns = a.stage_off[p + 1] - s0;
  *which = (int)(ns & 1);
  return ns ? a.live[s0 + ns - 1] : 1;
}

__global__ __launch_bounds__(kMixThreads) void mix_scan_kernel(MixArgs a) {
  __shared__ double s_tot[kMixThreads];
  const int64_t p = blockIdx.x;
  const int tid = threadIdx.x;
  int which;
  const int32_t live = final_lattice(a, p, &which);
  const double* pmf = a.buf[which] + p * a.cells;
  double* cdf = a.buf[which ^ 1] + p * a.cells;
  double carry = 0.0;
  for (int32_t c0 = 0; c0 < live; c0 += kMixTile) {
    const int32_t g0 = c0 + tid * kMixPer;
    double v[kMixPer];
    double run = 0.0;
#pragma unroll
    for (int j = 0; j < kMixPer; ++j) {
      run += g0 + j < live ? pmf[g0 + j] : 0.0;
      v[j] = run;
    }
    s_tot[tid] = run;
    __syncthreads();
    if (tid == 0) {
      double t = 0.0;
      for (int i = 0; i < kMixThreads; ++i) {
        t += s_tot[i];
        s_tot[i] = t;
      }
    }
    __syncthreads();
    const double before = tid ? s_tot[tid - 1] : 0.0;
#pragma unroll
    for (int j = 0; j < kMixPer; ++j)
      if (g0 + j < live) cdf[g0 + j] = carry + (before + v[j]);
    carry += s_tot[kMixThreads - 1];
    __syncthreads();
  }
  if (tid == 0) a.mass[p] = carry;
}

__global__ __launch_bounds__(kMixSearchThreads) void mix_search_kernel(MixArgs a) {
  __shared__ int32_t s_lo[kMixMaxLevels], s_gt[kMixMaxLevels], s_up[kMixMaxLevels], s_last;
  const int64_t p = blockIdx.x;
  const int tid = threadIdx.x;
  int which;
  const int32_t live = final_lattice(a, p, &which);
  const double* pmf = a.buf[which] + p * a.cells;
  const double* cdf = a.buf[which ^ 1] + p * a.cells;
  if (tid < kMixMaxLevels) { s_lo[tid] = INT_MAX; s_gt[tid] = INT_MAX; s_up[tid] = INT_MAX; }
  if (tid == 0) s_last = -1;
  __syncthreads();
  double lam[kMixMaxLevels];
#pragma unroll
  for (int l = 0; l < kMixMaxLevels; ++l) lam[l] = l < a.nl ? a.levels[l] : 2.0;
  int32_t lo[kMixMaxLevels], gt[kMixMaxLevels], last = -1;
#pragma unroll
  for (int l = 0; l < kMixMaxLevels; ++l) { lo[l] = INT_MAX; gt[l] = INT_MAX; }
  for (int32_t g = tid; g < live; g += kMixSearchThreads) {
    const double c = cdf[g];
    if (pmf[g] > 0.0) last = g;
#pragma unroll
    for (int l = 0; l < kMixMaxLevels; ++l) {
      if (c >= lam[l]) lo[l] = min(lo[l], g);
      if (c > lam[l]) gt[l] = min(gt[l], g);
    }
  }
#pragma unroll
  for (int l = 0; l < kMixMaxLevels; ++l) {
    if (lo[l] != INT_MAX) atomicMin(&s_lo[l], lo[l]);
    if (gt[l] != INT_MAX) atomicMin(&s_gt[l], gt[l]);
  }
  if (last >= 0) atomicMax(&s_last, last);
  __syncthreads();
  int32_t above[kMixMaxLevels], up[kMixMaxLevels];
#pragma unroll
  for (int l = 0; l < kMixMaxLevels; ++l) { above[l] = s_gt[l]; up[l] = INT_MAX; }
  for (int32_t g = tid; g < live; g += kMixSearchThreads) {
    if (!(pmf[g] > 0.0)) continue;
#pragma unroll
    for (int l = 0; l < kMixMaxLevels; ++l)
      if (g > above[l]) up[l] = min(up[l], g);
  }
#pragma unroll
  for (int l = 0; l < kMixMaxLevels; ++l)
    if (up[l] != INT_MAX) atomicMin(&s_up[l], up[l]);
  __syncthreads();
  if (tid < a.nl) {
    const int32_t end = max(s_last, 0);                    // a lattice without mass answers cell 0
    a.lower[p * a.nl + tid] = s_lo[tid] == INT_MAX ? end : s_lo[tid];
    a.upper[p * a.nl + tid] = s_up[tid] == INT_MAX ? end : s_up[tid];
  }
}

}  // namespace
}  // namespace gpdla

using namespace gpdla;

extern "C" {

int gpdla_count_mixture_tiling(int32_t* tile, int32_t* taps, int32_t* max_levels) {
  if (!tile || !taps || !max_levels) return set_error(GPDLA_EINVAL, "count_mixture: null argument");
  *tile = kMixTile; *taps = kMixTaps; *max_levels = kMixMaxLevels;
  return GPDLA_OK;
}

int gpdla_count_mixture_f64(int32_t device, const double* probs, const int32_t* shifts, const int64_t* tap_offsets,
                            const int64_t* stage_offsets, int64_t num_problems, int64_t cells, const double* levels,
                            int32_t num_levels, int32_t* lower_cells, int32_t* upper_cells, double* mass, double* pmf) {
  if (!tap_offsets || !stage_offsets || !lower_cells || !upper_cells || !mass || (num_levels > 0 && !levels))
    return set_error(GPDLA_EINVAL, "count_mixture: null argument");
  if (num_problems < 0 || num_problems > 65535)
    return set_error(GPDLA_EINVAL, "count_mixture: num_problems=%lld outside 0..65535", (long long)num_problems);
  if (cells < 1 || cells > GPDLA_MIX_MAX_CELLS)
    return set_error(GPDLA_EINVAL, "count_mixture: cells=%lld outside 1..%d", (long long)cells, GPDLA_MIX_MAX_CELLS);
  if (num_levels < 0 || num_levels > kMixMaxLevels)
    return set_error(GPDLA_EINVAL, "count_mixture: num_levels=%d outside 0..%d", (int)num_levels, kMixMaxLevels);
  for (int32_t l = 0; l < num_levels; ++l)
    if (!(levels[l] > 0.0 && levels[l] < 1.0))
      return set_error(GPDLA_EINVAL, "count_mixture: levels[%d] = %g outside (0, 1)", (int)l, levels[l]);
  if (stage_offsets[0] != 0 || tap_offsets[0] != 0) return set_error(GPDLA_EINVAL, "count_mixture: offsets must start at 0");
  for (int64_t p = 0; p < num_problems; ++p)
    if (stage_offsets[p + 1] < stage_offsets[p])
      return set_error(GPDLA_EINVAL, "count_mixture: stage_offsets[%lld] decreases", (long long)(p + 1));
  const int64_t NS = stage_offsets[num_problems];
  if (NS > INT32_MAX) return set_error(GPDLA_EINVAL, "count_mixture: %lld stages", (long long)NS);
  for (int64_t s = 0; s < NS; ++s)
    if (tap_offsets[s + 1] <= tap_offsets[s])
      return set_error(GPDLA_EINVAL, "count_mixture: stage %lld is empty", (long long)s);
  const int64_t NT = tap_offsets[NS];
  if (NT > 0 && (!probs || !shifts)) return set_error(GPDLA_EINVAL, "count_mixture: null taps");
  std::vector<int32_t> live((size_t)NS);
  int64_t max_stages = 0;
  for (int64_t p = 0; p < num_problems; ++p) {
    int64_t reach = 0;                                     // summed largest shifts so far
    max_stages = std::max(max_stages, stage_offsets[p + 1] - stage_offsets[p]);
    for (int64_t s = stage_offsets[p]; s < stage_offsets[p + 1]; ++s) {
      int32_t prev = 0;
      for (int64_t i = tap_offsets[s]; i < tap_offsets[s + 1]; ++i) {
        if (shifts[i] < prev)
          return set_error(GPDLA_EINVAL, "count_mixture: shifts[%lld] = %d: shifts must be >= 0 and not decrease within a stage",
                           (long long)i, (int)shifts[i]);
        prev = shifts[i];
        if (!(probs[i] >= 0.0 && probs[i] < INFINITY))
          return set_error(GPDLA_EINVAL, "count_mixture: probs[%lld] = %g: must be finite and >= 0", (long long)i, probs[i]);
      }
      reach += prev;
      if (reach >= cells)
        return set_error(GPDLA_EINVAL, "count_mixture: problem %lld reaches cell %lld of %lld at its stage %lld", (long long)p,
                         (long long)reach, (long long)cells, (long long)(s - stage_offsets[p]));
      live[(size_t)s] = (int32_t)(reach + 1);
    }
  }
  int rc = check_device(device);
  if (rc) return rc;
  LaunchTimes& lt = launch_times();
  lt.reset();
  if (num_problems == 0) return GPDLA_OK;
  HIP_TRY(hipSetDevice(device));
  const size_t P = (size_t)num_problems, lattice = P * (size_t)cells * 8, NL = (size_t)num_levels;
  DeviceStage st;
  const size_t o_p = st.carve((size_t)NT * 8), o_sh = st.carve((size_t)NT * 4), o_to = st.carve((size_t)(NS + 1) * 8);
  const size_t o_so = st.carve((P + 1) * 8), o_lv = st.carve((size_t)NS * 4), o_b0 = st.carve(lattice), o_b1 = st.carve(lattice);
  const size_t o_lam = st.carve(NL * 8), o_lo = st.carve(P * NL * 4), o_up = st.carve(P * NL * 4), o_m = st.carve(P * 8);
  HIP_TRY_IN("count_mixture", st.alloc());
  if (NT) {
    HIP_TRY_IN("count_mixture", st.upload(o_p, probs, (size_t)NT * 8));
    HIP_TRY_IN("count_mixture", st.upload(o_sh, shifts, (size_t)NT * 4));
  }
  HIP_TRY_IN("count_mixture", st.upload(o_to, tap_offsets, (size_t)(NS + 1) * 8));
  HIP_TRY_IN("count_mixture", st.upload(o_so, stage_offsets, (P + 1) * 8));
  if (NS) HIP_TRY_IN("count_mixture", st.upload(o_lv, live.data(), (size_t)NS * 4));
  if (NL) HIP_TRY_IN("count_mixture", st.upload(o_lam, levels, NL * 8));
  // both buffers zero (a stage reads below its predecessor's live prefix only what an earlier stage or this
  // memset wrote), then delta at cell 0 of every problem's first buffer
  HIP_TRY_IN("count_mixture", hipMemset(st.ptr<char>(o_b0), 0, lattice));
  HIP_TRY_IN("count_mixture", hipMemset(st.ptr<char>(o_b1), 0, lattice));
  const std::vector<double> ones(P, 1.0);
  HIP_TRY_IN("count_mixture", hipMemcpy2D(st.ptr<char>(o_b0), (size_t)cells * 8, ones.data(), 8, 8, P, hipMemcpyHostToDevice));
  MixArgs a{};
  a.probs = st.ptr<const double>(o_p); a.shifts = st.ptr<const int32_t>(o_sh); a.tap_off = st.ptr<const int64_t>(o_to);
  a.stage_off = st.ptr<const int64_t>(o_so); a.live = st.ptr<const int32_t>(o_lv);
  a.buf[0] = st.ptr<double>(o_b0); a.buf[1] = st.ptr<double>(o_b1); a.cells = cells;
  a.levels = st.ptr<const double>(o_lam); a.nl = num_levels; a.lower = st.ptr<int32_t>(o_lo); a.upper = st.ptr<int32_t>(o_up);
  a.mass = st.ptr<double>(o_m);
  lt.before();
  for (int64_t s = 0; s < max_stages; ++s) {
    int32_t reach = 0;                                     // the longest live prefix among the problems with stage s
    for (size_t p = 0; p < P; ++p)
      if (stage_offsets[p + 1] - stage_offsets[p] > s) reach = std::max(reach, live[(size_t)(stage_offsets[p] + s)]);
    a.stage = (int32_t)s;
    hipLaunchKernelGGL(mix_stage_kernel, dim3((unsigned)((reach + kMixTile - 1) / kMixTile), (unsigned)P), dim3(kMixThreads),
                       0, nullptr, a);
    HIP_TRY_IN("count_mixture", hipGetLastError());
  }
  lt.after();
  lt.before();
  hipLaunchKernelGGL(mix_scan_kernel, dim3((unsigned)P), dim3(kMixThreads), 0, nullptr, a);
  HIP_TRY_IN("count_mixture", hipGetLastError());
  lt.after();
  lt.before();
  hipLaunchKernelGGL(mix_search_kernel, dim3((unsigned)P), dim3(kMixSearchThreads), 0, nullptr, a);
  HIP_TRY_IN("count_mixture", hipGetLastError());
  lt.after();
  if (NL) {
    HIP_TRY_IN("count_mixture", st.download(lower_cells, o_lo, P * NL * 4));
    HIP_TRY_IN("count_mixture", st.download(upper_cells, o_up, P * NL * 4));
  }
  HIP_TRY_IN("count_mixture", st.download(mass, o_m, P * 8));
  if (pmf)
    for (size_t p = 0; p < P; ++p) {
      const size_t which = (size_t)((stage_offsets[p + 1] - stage_offsets[p]) & 1);
      HIP_TRY_IN("count_mixture", st.download(pmf + p * (size_t)cells, (which ? o_b1 : o_b0) + p * (size_t)cells * 8,
                                              (size_t)cells * 8));
    }
  lt.finish();
  return GPDLA_OK;
}

}  // extern "C"
