// Posterior intervals of the sample log-likelihood rows (include/gpdla.h "Posterior intervals"; DESIGN.md
// section 21): per row, level and absorber slot of the base chain, and for z_DLA and log N_HI each, the
// likelihood-ratio range, the posterior mean and sd, and quantiles.
//
// One 256-thread workgroup per (row, level), built from row_posterior.h like its siblings.  A quantile is a
// weighted order statistic, found without a sort: every slot value is array[index] with the arrays shared by
// all rows, so the order of the values is a property of the sample set.  The host ranks the offsets and the
// log N_HI once per call (build_rank_table); the kernel sums a slot's masses per rank -- first per coarse bin
// rank >> s, then per rank of the coarse bin each quantile level selected -- with the owned-bin scan, so a
// bin's sum is the sequential sum in sample-index order, and reads the cdf off a fixed-order scan of the bins.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "../../include/gpdla.h"
#include "internal.h"
#include "row_posterior.h"

namespace gpdla {
namespace {

static_assert(kMaxDlas == GPDLA_MAX_DLAS && kMaxDlas == 4, "the kernel dispatches on 1..4 slots");
static_assert(kIntervalMaxLevels == GPDLA_INTERVAL_MAX_LEVELS && kIntervalQuantiles == kIntervalMaxLevels, "gpdla.h");
static_assert(kIntervalMaxSamples == GPDLA_INTERVAL_MAX_SAMPLES, "gpdla.h");
static_assert(kIntervalCoarseBins <= 4 * kRowThreads, "hist_select scans four bins per thread");
static_assert(kIntervalTile % 4 == 0, "the scan reads four bin indices at a time");

constexpr int kRes = kIntervalResults, kResMean = kIntervalQuantiles, kResSd = kResMean + 1, kResLo = kResMean + 2,
              kResHi = kResMean + 3;

template <int NS>
__device__ __forceinline__ void intervals_body(const IntervalArgs& a, char* smem) {
#pragma clang fp contract(off)
  const SampleRowsArgs& r = a.r;
  const int row = blockIdx.x, tid = threadIdx.x, nq = a.num_levels;
  const int32_t S = (int32_t)r.S;
  const IntervalLds L = interval_lds(r.S, nq);
  const int64_t o = (int64_t)(NS - 1) * r.rows + row;
  const double* ll = r.ll + o * r.ld;
  double* s_rv = (double*)(smem + L.red_v);
  int32_t* s_ri = (int32_t*)(smem + L.red_i);
  double* s_res = (double*)(smem + L.res);   // [parameter][slot][kRes]
  for (int i = tid; i < 2 * kMaxDlas * kRes; i += kRowThreads) s_res[i] = NAN;
  const RowMax best = row_first_max(ll, S, tid, s_rv, s_ri);
  const double m = best.v;                   // unused when every entry is NaN
  const double W = row_weight_sum(ll, S, tid, m, s_rv);
  __syncthreads();
  const bool usable = best.i >= 0 && weight_sum_usable(W);
  const double zmin = r.zmin[row], zmax = r.zmax[row];
  const bool z_ok = isfinite(zmin) && isfinite(zmax) && zmax >= zmin;
  int32_t count = 0;

  if (usable) {
    // ---- pass 1: the likelihood-ratio range, T and sum pi x
    const double thr = m - a.lr_delta;
    double T = 0.0, sx[2][NS], lo[2][NS], hi[2][NS], mean[2][NS];
#pragma unroll
    for (int u = 0; u < NS; ++u)
      for (int p = 0; p < 2; ++p) { sx[p][u] = 0.0; lo[p][u] = INFINITY; hi[p][u] = -INFINITY; }
    for (int32_t j = tid; j < S; j += kRowThreads) {
      const double v = ll[j];
      int32_t c[NS];
      if (!walk_chain<NS>(r, row, j, NS, c)) continue;
      const double pi = sample_mass(v, m, W, true);
      const bool in = v > thr;   // false for NaN
      T += pi;
      count += in;
#pragma unroll
      for (int u = 0; u < NS; ++u) {
        const double x[2] = {sample_z(zmin, zmax, r.offset[c[u]]), r.log_nhi[c[u]]};
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          sx[p][u] += pi * x[p];
          if (in) { lo[p][u] = x[p] < lo[p][u] ? x[p] : lo[p][u]; hi[p][u] = x[p] > hi[p][u] ? x[p] : hi[p][u]; }
        }
      }
    }
    T = row_sum(T, tid, s_rv);
    count = row_count(count, tid, s_ri);
#pragma unroll
    for (int u = 0; u < NS; ++u)
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const double sum = row_sum(sx[p][u], tid, s_rv);
        const double l = row_extreme<false>(lo[p][u], tid, s_rv), h = row_extreme<true>(hi[p][u], tid, s_rv);
        mean[p][u] = sum / T;
        if (tid == 0) {
          double* res = s_res + (p * kMaxDlas + u) * kRes;
          res[kResMean] = T > 0.0 ? mean[p][u] : NAN;
          res[kResLo] = count > 0 ? l : NAN;
          res[kResHi] = count > 0 ? h : NAN;
        }
      }
    // ---- pass 2: sum pi (x - mean)^2 about the mean just formed
    double ss[2][NS];
#pragma unroll
    for (int u = 0; u < NS; ++u) ss[0][u] = ss[1][u] = 0.0;
    if (T > 0.0)
      for (int32_t j = tid; j < S; j += kRowThreads) {
        int32_t c[NS];
        if (!walk_chain<NS>(r, row, j, NS, c)) continue;
        const double pi = sample_mass(ll[j], m, W, true);
#pragma unroll
        for (int u = 0; u < NS; ++u) {
          const double dz = sample_z(zmin, zmax, r.offset[c[u]]) - mean[0][u], dn = r.log_nhi[c[u]] - mean[1][u];
          ss[0][u] += pi * (dz * dz);
          ss[1][u] += pi * (dn * dn);
        }
      }
#pragma unroll
    for (int u = 0; u < NS; ++u)
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const double sum = row_sum(ss[p][u], tid, s_rv);
        if (tid == 0 && T > 0.0) s_res[(p * kMaxDlas + u) * kRes + kResSd] = sqrt(sum / T);
      }

    // ---- the quantiles of each slot: coarse histograms, then the ranks of the selected coarse bins
    const int s = interval_shift(r.S), nc = (int)((S - 1) >> s) + 1, cells = interval_cells(r.S, nq);
    const int G = interval_group(s, nq), mask = (1 << s) - 1;
    double* s_hz = (double*)(smem + L.hist);
    double* s_hn = s_hz + cells;
    double* s_pi = (double*)(smem + L.mass);
    int32_t* s_bz = (int32_t*)(smem + L.bin_z);
    int32_t* s_bn = (int32_t*)(smem + L.bin_n);
    double* s_tgt = (double*)(smem + L.target);      // [parameter][kIntervalQuantiles]
    double* s_basec = (double*)(smem + L.base_c);
    double* s_base = (double*)(smem + L.base);
    int32_t* s_pickc = (int32_t*)(smem + L.pick_c);
    int32_t* s_rank = (int32_t*)(smem + L.rank);
    int32_t* s_pick = (int32_t*)(smem + L.pick);
    int32_t* s_last = (int32_t*)(smem + L.last);
    for (int u = 0; u < NS; ++u) {
      // one walk of the row: per sample its mass and one bin per parameter, then the owned-bin scans
      auto pass = [&](auto&& bins) {
        for (int i = tid; i < 2 * cells; i += kRowThreads) s_hz[i] = 0.0;
        for (uint32_t t0 = 0; t0 < (uint32_t)S; t0 += kIntervalTile) {
          __syncthreads();   // zeroed histograms ready; the previous tile's scan is over
          for (int i = tid; i < kIntervalTile; i += kRowThreads) {
            const uint32_t j = t0 + i;
            double pi = 0.0;
            int32_t bz = -1, bn = -1;
            if (j < (uint32_t)S) {
              pi = sample_mass(ll[j], m, W, true);
              int32_t c[NS];
              if (pi > 0.0 && walk_chain<NS>(r, row, (int32_t)j, NS, c)) {
                int32_t cu = c[0];
#pragma unroll
                for (int k = 1; k < NS; ++k)
                  if (u == k) cu = c[k];
                bins(cu, bz, bn);
              }
            }
            s_pi[i] = pi; s_bz[i] = bz; s_bn[i] = bn;
          }
          __syncthreads();
          const int cnt = (int)min((uint32_t)kIntervalTile, (uint32_t)S - t0);
          if (z_ok) scan_tile(s_bz, cnt, tid, [&](int e, int b) { s_hz[b] += s_pi[e]; });
          scan_tile(s_bn, cnt, tid, [&](int e, int b) { s_hn[b] += s_pi[e]; });
        }
        __syncthreads();
      };

      if (tid < 2 * kIntervalQuantiles) { s_rank[tid] = -1; s_pickc[tid] = -1; }
      pass([&](int32_t cu, int32_t& bz, int32_t& bn) {
        if (z_ok) bz = a.rank_z[cu] >> s;
        bn = a.rank_n[cu] >> s;
      });
      for (int p = z_ok ? 0 : 1; p < 2; ++p) {
        const double total = hist_select<true>(p ? s_hn : s_hz, nc, 0.0, a.levels, s_tgt + p * kIntervalQuantiles, nq, tid,
                                               s_rv, s_pick, s_base, s_last);
        if (total > 0.0 && tid < nq) {
          s_pickc[p * kIntervalQuantiles + tid] = s_pick[nq + tid];
          s_basec[p * kIntervalQuantiles + tid] = s_base[tid];
          if (s == 0) s_rank[p * kIntervalQuantiles + tid] = s_pick[nq + tid];
        }
        __syncthreads();
      }
      if (s > 0)
        for (int g0 = 0; g0 < nq; g0 += G) {
          const int ng = min(G, nq - g0);
          pass([&](int32_t cu, int32_t& bz, int32_t& bn) {
            if (z_ok) {
              const int32_t rk = a.rank_z[cu], cb = rk >> s;
              for (int gi = 0; gi < ng; ++gi)
                if (s_pickc[g0 + gi] == cb) { bz = (gi << s) + (rk & mask); break; }
            }
            const int32_t rk = a.rank_n[cu], cb = rk >> s;
            for (int gi = 0; gi < ng; ++gi)
              if (s_pickc[kIntervalQuantiles + g0 + gi] == cb) { bn = (gi << s) + (rk & mask); break; }
          });
          for (int gi = 0; gi < ng; ++gi)
            for (int p = 0; p < 2; ++p) {
              const int k = p * kIntervalQuantiles + g0 + gi;
              const int32_t cb = s_pickc[k];
              if (cb < 0) continue;   // uniform: no z, or an empty slot
              int first = gi;         // levels that selected the same coarse bin share the first one's histogram
              for (int gj = gi - 1; gj >= 0; --gj)
                if (s_pickc[p * kIntervalQuantiles + g0 + gj] == cb) first = gj;
              hist_select<false>((p ? s_hn : s_hz) + (first << s), 1 << s, s_basec[k], nullptr, s_tgt + k, 1, tid, s_rv,
                                 s_pick, s_base, s_last);
              if (tid == 0) s_rank[k] = (cb << s) + s_pick[1];
            }
        }
      __syncthreads();
      if (tid < 2 * kIntervalQuantiles && (tid & (kIntervalQuantiles - 1)) < nq) {
        const int p = tid / kIntervalQuantiles, k = tid & (kIntervalQuantiles - 1);
        const int32_t rk = s_rank[tid];
        if (rk >= 0) s_res[(p * kMaxDlas + u) * kRes + k] = p ? a.uniq_n[rk] : sample_z(zmin, zmax, a.uniq_off[rk]);
      }
      __syncthreads();
    }
  }
  __syncthreads();

  // ---- write: slots >= NS and everything of an unusable row stayed NaN; z of a row without a z range is NaN
  if (tid == 0) a.lr_count[o] = count;
  for (int i = tid; i < 2 * kMaxDlas * kRes; i += kRowThreads) {
    const int p = i / (kMaxDlas * kRes), u = (i / kRes) % kMaxDlas, k = i % kRes;
    const double v = (p == 0 && !z_ok) ? NAN : s_res[i];
    const int64_t ou = o * kMaxDlas + u;
    if (k < kIntervalQuantiles) {
      if (k < nq) (p ? a.n_q : a.z_q)[ou * nq + k] = v;
    } else if (k == kResMean) {
      (p ? a.n_mean : a.z_mean)[ou] = v;
    } else if (k == kResSd) {
      (p ? a.n_sd : a.z_sd)[ou] = v;
    } else {
      (p ? a.n_lr : a.z_lr)[ou * 2 + (k - kResLo)] = v;
    }
  }
}

__global__ __launch_bounds__(kRowThreads) void posterior_intervals_kernel(IntervalArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  switch (blockIdx.y) {   // uniform over the workgroup
    case 0: intervals_body<1>(a, smem); break;
    case 1: intervals_body<2>(a, smem); break;
    case 2: intervals_body<3>(a, smem); break;
    default: intervals_body<4>(a, smem); break;
  }
}

}  // namespace

hipError_t launch_posterior_intervals(const IntervalArgs& a, hipStream_t s) {
  if (a.r.rows < 1 || a.r.levels < 1) return hipSuccess;
  if (!sample_rows_ok(a.r, false) || a.r.S > kIntervalMaxSamples || a.num_levels < 1 || a.num_levels > kIntervalMaxLevels)
    return hipErrorInvalidValue;
  const IntervalLds L = interval_lds(a.r.S, a.num_levels);
  hipLaunchKernelGGL(posterior_intervals_kernel, dim3((unsigned)a.r.rows, (unsigned)a.r.levels), dim3(kRowThreads),
                     L.total, s, a);
  return hipGetLastError();
}

void build_rank_table(const double* x, int64_t S, int32_t* rank, double* uniq) {
  std::vector<int32_t> idx((size_t)S);
  std::iota(idx.begin(), idx.end(), 0);
  // ascending, NaNs last; ties keep the index order (the ranks do not depend on it)
  std::stable_sort(idx.begin(), idx.end(), [x](int32_t i, int32_t j) {
    const bool ni = x[i] != x[i], nj = x[j] != x[j];
    return ni != nj ? nj : (!ni && x[i] < x[j]);
  });
  int32_t r = -1;
  for (int64_t i = 0; i < S; ++i) {
    const double v = x[idx[i]];
    const bool same = i > 0 && (v == x[idx[i - 1]] || (v != v && x[idx[i - 1]] != x[idx[i - 1]]));
    if (!same) uniq[++r] = v;
    rank[idx[i]] = r;
  }
  for (int64_t i = r + 1; i < S; ++i) uniq[i] = NAN;
}

int validate_interval_levels(double lr_delta, int32_t num_levels, const double* levels, int64_t S) {
  if (!(lr_delta > 0.0 && lr_delta < INFINITY)) return set_error(GPDLA_EINVAL, "lr_delta = %g: must be finite and > 0", lr_delta);
  if (num_levels < 1 || num_levels > GPDLA_INTERVAL_MAX_LEVELS)
    return set_error(GPDLA_EINVAL, "num_levels=%d outside 1..%d", num_levels, GPDLA_INTERVAL_MAX_LEVELS);
  for (int i = 0; i < num_levels; ++i) {
    if (!(levels[i] > 0.0 && levels[i] < 1.0))
      return set_error(GPDLA_EINVAL, "levels[%d] = %g: quantile levels must lie strictly inside (0, 1)", i, levels[i]);
    if (i > 0 && !(levels[i] > levels[i - 1]))
      return set_error(GPDLA_EINVAL, "levels[%d] = %g: quantile levels must be strictly increasing", i, levels[i]);
  }
  if (S > GPDLA_INTERVAL_MAX_SAMPLES)
    return set_error(GPDLA_EINVAL, "num_samples=%lld: the posterior intervals support at most %d samples", (long long)S,
                     GPDLA_INTERVAL_MAX_SAMPLES);
  return GPDLA_OK;
}

}  // namespace gpdla

using namespace gpdla;

extern "C" {

int gpdla_posterior_intervals_f64(int32_t device, const double* ll, int64_t rows, int64_t S, int64_t ld,
                                  const double* offset_samples, const double* log_nhi_samples, const double* min_z,
                                  const double* max_z, const int32_t* base_inds, int32_t levels,
                                  const gpdla_interval_spec* ispec, const gpdla_intervals* iv) {
  HostSampleRows h{ll, rows, S, ld, offset_samples, log_nhi_samples, nullptr, min_z, max_z, base_inds, levels};
  int rc = h.check(ispec && iv);
  if (rc) return rc;
  if (!iv->z_means || !iv->z_sds || !iv->log_nhi_means || !iv->log_nhi_sds || !iv->z_lr_ranges || !iv->log_nhi_lr_ranges ||
      !iv->z_quantiles || !iv->log_nhi_quantiles || !iv->lr_counts)
    return set_error(GPDLA_EINVAL, "null interval array");
  if (iv->memory != GPDLA_MEM_HOST) return set_error(GPDLA_EINVAL, "intervals memory=%d: host buffers here", iv->memory);
  if ((rc = validate_interval_levels(ispec->lr_delta, ispec->num_levels, ispec->levels, S))) return rc;
  if ((rc = check_device(device))) return rc;
  if (rows == 0) return GPDLA_OK;
  HIP_TRY(hipSetDevice(device));
  const size_t Ss = (size_t)S, LR = (size_t)levels * rows, slots = LR * kMaxDlas, nq = (size_t)ispec->num_levels;
  std::vector<int32_t> rank_z(Ss), rank_n(Ss);
  std::vector<double> uniq_off(Ss), uniq_n(Ss);
  build_rank_table(offset_samples, S, rank_z.data(), uniq_off.data());
  build_rank_table(log_nhi_samples, S, rank_n.data(), uniq_n.data());
  DeviceStage st;
  h.carve(st);
  const size_t o_rz = st.carve(Ss * 4), o_rn = st.carve(Ss * 4), o_uo = st.carve(Ss * 8), o_un = st.carve(Ss * 8);
  const size_t o_m = st.carve(4 * slots * 8), o_lr = st.carve(2 * slots * 2 * 8), o_q = st.carve(2 * slots * nq * 8);
  const size_t o_cnt = st.carve(LR * 4);
  IntervalArgs a{};
  HIP_TRY_IN("posterior_intervals", st.alloc());
  HIP_TRY_IN("posterior_intervals", h.upload(st, &a.r, nullptr));
  HIP_TRY_IN("posterior_intervals", st.upload(o_rz, rank_z.data(), Ss * 4));
  HIP_TRY_IN("posterior_intervals", st.upload(o_rn, rank_n.data(), Ss * 4));
  HIP_TRY_IN("posterior_intervals", st.upload(o_uo, uniq_off.data(), Ss * 8));
  HIP_TRY_IN("posterior_intervals", st.upload(o_un, uniq_n.data(), Ss * 8));
  a.rank_z = st.ptr<const int32_t>(o_rz); a.rank_n = st.ptr<const int32_t>(o_rn);
  a.uniq_off = st.ptr<const double>(o_uo); a.uniq_n = st.ptr<const double>(o_un);
  a.lr_delta = ispec->lr_delta; a.num_levels = ispec->num_levels;
  for (size_t i = 0; i < nq; ++i) a.levels[i] = ispec->levels[i];
  double* mom = st.ptr<double>(o_m);
  a.z_mean = mom; a.z_sd = mom + slots; a.n_mean = mom + 2 * slots; a.n_sd = mom + 3 * slots;
  a.z_lr = st.ptr<double>(o_lr); a.n_lr = a.z_lr + 2 * slots;
  a.z_q = st.ptr<double>(o_q); a.n_q = a.z_q + slots * nq;
  a.lr_count = st.ptr<int32_t>(o_cnt);
  HIP_TRY_IN("posterior_intervals", launch_posterior_intervals(a, nullptr));
  HIP_TRY_IN("posterior_intervals", st.download(iv->z_means, o_m, slots * 8));
  HIP_TRY_IN("posterior_intervals", st.download(iv->z_sds, o_m + slots * 8, slots * 8));
  HIP_TRY_IN("posterior_intervals", st.download(iv->log_nhi_means, o_m + 2 * slots * 8, slots * 8));
  HIP_TRY_IN("posterior_intervals", st.download(iv->log_nhi_sds, o_m + 3 * slots * 8, slots * 8));
  HIP_TRY_IN("posterior_intervals", st.download(iv->z_lr_ranges, o_lr, 2 * slots * 8));
  HIP_TRY_IN("posterior_intervals", st.download(iv->log_nhi_lr_ranges, o_lr + 2 * slots * 8, 2 * slots * 8));
  HIP_TRY_IN("posterior_intervals", st.download(iv->z_quantiles, o_q, slots * nq * 8));
  HIP_TRY_IN("posterior_intervals", st.download(iv->log_nhi_quantiles, o_q + slots * nq * 8, slots * nq * 8));
  HIP_TRY_IN("posterior_intervals", st.download(iv->lr_counts, o_cnt, LR * 4));
  return GPDLA_OK;
}

}  // extern "C"
