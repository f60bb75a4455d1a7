// The per-row posterior reductions every summary and population kernel is built from (posterior_summary.hip,
// population.hip, level_population.hip), each written once: DESIGN.md section 13 states the order of operations.
//
// One 256-thread workgroup reduces one row of sample log likelihoods.  Every floating-point result is formed
// in an order fixed by the sample index and the thread count alone -- no floating-point atomics -- so a row's
// outputs do not depend on which other rows share the launch and repeat bit for bit:
//   max / argmax   thread t takes samples t, t + 256, ... in index order; the 256 candidates are merged by a
//                  64-lane xor butterfly and then over the 4 waves in wave order.  (max, smallest index
//                  attaining it) is associative and commutative, so this is nanmax's first maximum.
//   W = sum w_j    the same strided partial sums and the same tree (a + b == b + a bitwise, so every lane of
//                  the butterfly holds the same value).
//   binned sums    the row goes through LDS in tiles: per sample the mass and, per absorber slot of its base
//                  chain, the flat bin are staged; then every thread scans the tile's (sample, slot) entries in
//                  order and adds those of the bins it owns (bin b belongs to thread b mod 256).  A bin's sum
//                  is therefore the sequential sum in (sample index, slot) order, whatever the tile size.
//   large list     the few samples kept exactly arrive through an LDS integer counter (the only atomic) and
//                  are sorted by sample index, so their order does not depend on arrival.
// Every gather index of a chain is range-checked before it is used: a void chain (-1, or an index outside
// [0, S)) never becomes a read.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "internal.h"

namespace gpdla {

constexpr int kRowThreads = 256;
constexpr int kRowWaves = kRowThreads / 64;
constexpr int kRowTileOne = 512;      // samples staged per pass by the level-1 launches (one absorber each)
constexpr int kRowTileLevels = 256;   // ... by the level launches: up to kMaxDlas (bin, N) pairs per sample
constexpr int kRowCandidates = 16;    // LDS slots of the large list; the kPopulationMaxLarge lowest indices are kept

static_assert(kRowTileOne % 4 == 0 && kRowTileLevels % 4 == 0, "the scan reads four bin indices at a time");

// ---- dynamic LDS: every offset a multiple of 16
__host__ __device__ inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }
struct RowLds {
  size_t red_v, red_i, edges_z, edges_n, planes, mass, nh, bin, cand_p, cand_i, cand_b, count, total;
  __host__ __device__ size_t take(size_t bytes) { const size_t o = total; total = up16(total + bytes); return o; }
};
// the two reduction arrays, the staged edges, `nplanes` planes of the grid and a tile's masses
__host__ __device__ inline RowLds row_lds(int nz, int nn, int nplanes, int tile, bool grid = true) {
  RowLds l{};
  l.red_v = l.take(kRowWaves * 8);
  l.red_i = l.take(kRowWaves * 4);
  if (grid) {
    l.edges_z = l.take((size_t)(nz + 1) * 8);
    l.edges_n = l.take((size_t)(nn + 1) * 8);
    l.planes = l.take((size_t)nplanes * nz * nn * 8);
    l.mass = l.take((size_t)tile * 8);
  }
  return l;
}
// bin planes: per sample `slots` (N, bin) pairs.  32 x 32 bins: 51,792 B at (512, 1), 55,888 B at (256, 4)
__host__ __device__ inline RowLds planes_lds(int nz, int nn, int tile, int slots, bool grid = true) {
  RowLds l = row_lds(nz, nn, kSummaryPlanes, tile, grid);
  if (grid) {
    l.nh = l.take((size_t)tile * slots * 8);
    l.bin = l.take((size_t)tile * slots * 4);
  }
  return l;
}
// split: per sample `slots` bins, and the candidates with `bin_slots` bins each.  32 x 32 bins: 15,392 B at
// (256, 4, kMaxDlas)
__host__ __device__ inline RowLds split_lds(int nz, int nn, int tile, int slots, int bin_slots) {
  RowLds l = row_lds(nz, nn, 1, tile);
  l.bin = l.take((size_t)tile * slots * 4);
  l.cand_p = l.take((size_t)kRowCandidates * 8);
  l.cand_i = l.take((size_t)kRowCandidates * 4);
  l.cand_b = l.take((size_t)kRowCandidates * bin_slots * 4);
  l.count = l.take(4);
  return l;
}

// ---- the first maximum over the non-NaN entries of a row: i = -1 (and v unused) when there is none.  Every
// thread returns the same pair; s_rv / s_ri are free again on return
struct RowMax {
  double v;
  int32_t i;
};
__device__ __forceinline__ RowMax row_first_max(const double* ll, int32_t S, int tid, double* s_rv, int32_t* s_ri) {
  const int lane = tid & 63, wave = tid >> 6;
  double bv = 0.0;
  int32_t bi = -1;
  for (int64_t j = tid; j < S; j += kRowThreads) {
    const double v = ll[j];
    if (v == v && (bi < 0 || v > bv)) { bv = v; bi = (int32_t)j; }
  }
  auto merge = [](double& v, int32_t& i, double ov, int32_t oi) {
    if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) { v = ov; i = oi; }
  };
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o);
    const int32_t oi = __shfl_xor(bi, o);
    merge(bv, bi, ov, oi);
  }
  if (lane == 0) { s_rv[wave] = bv; s_ri[wave] = bi; }
  __syncthreads();
  bv = s_rv[0]; bi = s_ri[0];
#pragma unroll
  for (int w = 1; w < kRowWaves; ++w) merge(bv, bi, s_rv[w], s_ri[w]);
  __syncthreads();
  return {bv, bi};
}

// w_j = exp(l_j - m), NaN -> 0 (the resampler's weights, multi_dla.hip), and pi_j = w_j / W
__device__ __forceinline__ double sample_weight(double v, double m) { return (v == v) ? exp(v - m) : 0.0; }
__device__ __forceinline__ bool weight_sum_usable(double W) { return W > 0.0 && W < INFINITY; }
__device__ __forceinline__ double sample_mass(double v, double m, double W, bool usable) {
  const double w = sample_weight(v, m);
  return usable ? w / W : 0.0;
}

// W = sum_j w_j; every thread returns the same value
__device__ __forceinline__ double row_weight_sum(const double* ll, int32_t S, int tid, double m, double* s_rv) {
  const int lane = tid & 63, wave = tid >> 6;
  double loc = 0.0;
  for (int64_t j = tid; j < S; j += kRowThreads) loc += sample_weight(ll[j], m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) loc += __shfl_xor(loc, o);
  if (lane == 0) s_rv[wave] = loc;
  __syncthreads();
  double W = s_rv[0];
#pragma unroll
  for (int w = 1; w < kRowWaves; ++w) W += s_rv[w];
  return W;
}

// ---- what both kinds of kernel read of the rows (internal.h)
// The `len` absorbers of sample j at level `len`: c[0] = j, c[i] its base at each shallower level.  False when
// the chain is void (then the entries from the break on are not to be used); an index is read from only
// after it passed the range check.
template <int kBound>
__device__ __forceinline__ bool walk_chain(const SampleRowsArgs& r, int row, int32_t j, int len, int32_t (&c)[kBound]) {
  const int32_t S = (int32_t)r.S;
  bool ok = (uint32_t)j < (uint32_t)S;   // 0 <= j < S in one compare: -1 (no MAP sample) is void like any other
  int32_t cur = j;
#pragma unroll
  for (int i = 0; i < kBound; ++i) {
    c[i] = cur;
    if (i < len - 1 && ok) {
      cur = r.base ? r.base[((int64_t)(len - 2 - i) * r.rows + row) * r.ld_base + cur] : -1;
      ok = cur >= 0 && cur < S;
    }
  }
  return ok;
}

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

// ---- the search cuts of one row: uniform over the launch, and over the workgroup.  The
// bitmap is read from global memory (a row's stretch is a few hundred bytes; the launches are no slower
// with the cuts on than off, profiles/search_cuts/bench_c2.json and DESIGN.md section 22): the LDS
// carves above are those of a launch without cuts
struct RowCut {
  bool prox, pix;
  double z_upper;
  int32_t n;
  const uint32_t* words;
};
__device__ __forceinline__ RowCut row_cut(const SampleRowsArgs& r, int row) {
  RowCut c{r.cut_z_upper != nullptr, r.cut_npix != nullptr, 0.0, 0, nullptr};
  if (c.prox) c.z_upper = r.cut_z_upper[row];
  if (c.pix) { c.n = r.cut_npix[row]; c.words = r.cut_words + r.cut_word_off[row]; }
  return c;
}
// whether a slot at redshift z passes the cuts: z < z_upper, and pixel (int)(((z - min_z) / span) n) good, the
// index formed in this operation order and truncated; an index outside [0, n), a NaN, n = 0 or span = 0 excludes
__device__ __forceinline__ bool slot_kept(const RowCut& c, double zmin, double zmax, double z) {
#pragma clang fp contract(off)
  if (c.prox && !(z < c.z_upper)) return false;
  if (c.pix) {
    const double span = zmax - zmin;
    const double t = (z - zmin) / span;
    const double f = t * (double)c.n;
    if (span == 0.0 || !(f > -1.0 && f < (double)c.n)) return false;
    const int32_t i = (int32_t)f;
    if (!((c.words[i >> 5] >> (i & 31)) & 1u)) return false;
  }
  return true;
}

// flat bin iz nn + in of sample ci on the grid staged at s_ez / s_en, or -1
__device__ __forceinline__ int32_t sample_bin(const SampleRowsArgs& r, const RowCut& cut, const double* s_ez,
                                              const double* s_en, double zmin, double zmax, int32_t ci) {
  const double z = sample_z(zmin, zmax, r.offset[ci]);
  if ((cut.prox || cut.pix) && !slot_kept(cut, zmin, zmax, z)) return -1;
  const int iz = find_bin(s_ez, r.nz, z);
  const int in = find_bin(s_en, r.nn, r.log_nhi[ci]);
  return (iz >= 0 && in >= 0) ? iz * r.nn + in : -1;
}

// edges into LDS and `n` zeroed plane entries; a __syncthreads() makes them visible
__device__ __forceinline__ void stage_grid(const SampleRowsArgs& r, int tid, double* s_ez, double* s_en, double* s_pl, int n) {
  for (int i = tid; i <= r.nz; i += kRowThreads) s_ez[i] = r.z_edges[i];
  for (int i = tid; i <= r.nn; i += kRowThreads) s_en[i] = r.n_edges[i];
  for (int i = tid; i < n; i += kRowThreads) s_pl[i] = 0.0;
}

// The scan of a staged tile: entries 0 .. cnt - 1 of s_bin in order (the entries up to the next multiple of
// four are -1), add(e, b) for every entry e whose bin b this thread owns
template <class Add>
__device__ __forceinline__ void scan_tile(const int32_t* s_bin, int cnt, int tid, Add add) {
  for (int e0 = 0; e0 < cnt; e0 += 4) {
    const int4 b4 = *(const int4*)(s_bin + e0);   // the same address in every lane: a broadcast
    const int bs[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int b = bs[u];
      if (b >= 0 && (b & (kRowThreads - 1)) == tid) add(e0 + u, b);
    }
  }
}

// ---- the bin planes of level NS of one row: sum pi, pi^2, N pi, N^2 pi, N^2 pi^2 per bin over every absorber
// of every sample's chain, kTile samples per pass.  m is the row's maximum (row_first_max), ll the row, L
// planes_lds() of the launch, out the row's kSummaryPlanes x nz nn result.
template <int NS, int kTile>
__device__ __forceinline__ void planes_rows(const SampleRowsArgs& r, const double* nhi, int row, const double* ll,
                                            double m, const RowLds& L, char* smem, double* out) {
  const int tid = threadIdx.x;
  const uint32_t S = (uint32_t)r.S;
  const double W = row_weight_sum(ll, (int32_t)S, tid, m, (double*)(smem + L.red_v));
  const bool usable = weight_sum_usable(W);
  double* s_ez = (double*)(smem + L.edges_z);
  double* s_en = (double*)(smem + L.edges_n);
  double* s_pl = (double*)(smem + L.planes);
  double* s_pi = (double*)(smem + L.mass);
  double* s_nh = (double*)(smem + L.nh);
  int32_t* s_bin = (int32_t*)(smem + L.bin);
  const int nb = r.nz * r.nn;
  stage_grid(r, tid, s_ez, s_en, s_pl, kSummaryPlanes * nb);
  const double zmin = r.zmin[row], zmax = r.zmax[row];
  const RowCut cut = row_cut(r, row);
  for (uint32_t t0 = 0; t0 < S; t0 += kTile) {   // S <= INT32_MAX: 32 bits hold t0 + kTile
    __syncthreads();   // edges and zeroed planes ready; the previous tile's scan is over
    for (int i = tid; i < kTile; i += kRowThreads) {
      const uint32_t j = t0 + i;
      double pi = 0.0;
      int32_t b[NS];
      double nh[NS];
#pragma unroll
      for (int u = 0; u < NS; ++u) { b[u] = -1; nh[u] = 0.0; }
      if (j < S) {
        pi = sample_mass(ll[j], m, W, usable);
        int32_t c[NS];
        if ((NS == 1 || pi > 0.0) && walk_chain<NS>(r, row, (int32_t)j, NS, c)) {
#pragma unroll
          for (int u = 0; u < NS; ++u) {
            nh[u] = nhi[c[u]];
            b[u] = sample_bin(r, cut, s_ez, s_en, zmin, zmax, c[u]);
          }
        }
      }
      s_pi[i] = pi;
#pragma unroll
      for (int u = 0; u < NS; ++u) { s_nh[i * NS + u] = nh[u]; s_bin[i * NS + u] = b[u]; }
    }
    __syncthreads();
    scan_tile(s_bin, (int)min((uint32_t)kTile, S - t0) * NS, tid, [&](int e, int b) {
      const double pi = s_pi[e / NS], N = s_nh[e];
      const double np = N * pi;
      s_pl[0 * nb + b] += pi;
      s_pl[1 * nb + b] += pi * pi;
      s_pl[2 * nb + b] += np;
      s_pl[3 * nb + b] += N * np;
      s_pl[4 * nb + b] += np * np;
    });
  }
  __syncthreads();
  for (int i = tid; i < kSummaryPlanes * nb; i += kRowThreads) out[i] = s_pl[i];
}

// ---- the large list: candidates with kBinSlots bins each
template <int kBinSlots>
struct Candidates {
  double* p;
  int32_t *i, *b, *count;
};
template <int kBinSlots, int NS>
__device__ __forceinline__ void push_candidate(const Candidates<kBinSlots>& c, double p, int32_t j, const int32_t (&b)[NS]) {
  const int slot = atomicAdd(c.count, 1);   // integer, LDS: the order is fixed by the sort below
  if (slot < kRowCandidates) {
    c.p[slot] = p; c.i[slot] = j;
#pragma unroll
    for (int u = 0; u < kBinSlots; ++u) c.b[slot * kBinSlots + u] = u < NS ? b[u] : -1;
  }
}
// One thread, after the last tile: sorts by sample index and writes the kPopulationMaxLarge entries of the row
// (-1 / NaN / -1 where unused).  sum_j P pi_j <= 1 bounds the candidates by 1 / p_switch <= kPopulationMaxLarge;
// were there ever more, the lowest sample indices among the first kRowCandidates arrivals are kept
template <int kBinSlots>
__device__ __forceinline__ void write_candidates(const Candidates<kBinSlots>& c, int32_t* inds, double* probs, int32_t* bins) {
  const int n = min(*c.count, kRowCandidates);
  for (int i = 1; i < n; ++i) {      // insertion sort by sample index
    const int32_t ci = c.i[i];
    const double cp = c.p[i];
    int32_t cb[kBinSlots];
#pragma unroll
    for (int u = 0; u < kBinSlots; ++u) cb[u] = c.b[i * kBinSlots + u];
    int k = i - 1;
    while (k >= 0 && c.i[k] > ci) {
      c.i[k + 1] = c.i[k]; c.p[k + 1] = c.p[k];
#pragma unroll
      for (int u = 0; u < kBinSlots; ++u) c.b[(k + 1) * kBinSlots + u] = c.b[k * kBinSlots + u];
      --k;
    }
    c.i[k + 1] = ci; c.p[k + 1] = cp;
#pragma unroll
    for (int u = 0; u < kBinSlots; ++u) c.b[(k + 1) * kBinSlots + u] = cb[u];
  }
  for (int i = 0; i < kPopulationMaxLarge; ++i) {
    const bool use = i < n;
    inds[i] = use ? c.i[i] : -1;
    probs[i] = use ? c.p[i] : NAN;
#pragma unroll
    for (int u = 0; u < kBinSlots; ++u) bins[i * kBinSlots + u] = use ? c.b[i * kBinSlots + u] : -1;
  }
}

// ---- the split of level NS of one row with p_j = P pi_j: samples with p_j >= p_switch and a slot inside the
// grid go to the large list (kBinSlots bins per entry), the others add p_j to the Poisson-plane bin of each
// slot.  L is split_lds() of the launch.
template <int NS, int kTile, int kBinSlots>
__device__ __forceinline__ void split_rows(const SplitArgs& a, int row, int64_t o, double P, const RowLds& L, char* smem) {
  static_assert(NS <= kBinSlots, "a candidate keeps every slot's bin");
  const SampleRowsArgs& r = a.r;
  const int tid = threadIdx.x;
  const uint32_t S = (uint32_t)r.S;
  const double* ll = r.ll + ((int64_t)(NS - 1) * r.rows + row) * r.ld;
  double* s_rv = (double*)(smem + L.red_v);
  const double m = row_first_max(ll, (int32_t)S, tid, s_rv, (int32_t*)(smem + L.red_i)).v;   // unused when every entry is NaN
  const double W = row_weight_sum(ll, (int32_t)S, tid, m, s_rv);
  const bool usable = weight_sum_usable(W);
  double* s_ez = (double*)(smem + L.edges_z);
  double* s_en = (double*)(smem + L.edges_n);
  double* s_pl = (double*)(smem + L.planes);
  double* s_p = (double*)(smem + L.mass);
  int32_t* s_bin = (int32_t*)(smem + L.bin);
  const Candidates<kBinSlots> cand{(double*)(smem + L.cand_p), (int32_t*)(smem + L.cand_i), (int32_t*)(smem + L.cand_b),
                                   (int32_t*)(smem + L.count)};
  const int nb = r.nz * r.nn;
  stage_grid(r, tid, s_ez, s_en, s_pl, nb);
  if (tid == 0) *cand.count = 0;
  const double zmin = r.zmin[row], zmax = r.zmax[row];
  const RowCut cut = row_cut(r, row);
  for (uint32_t t0 = 0; t0 < S; t0 += kTile) {   // S <= INT32_MAX: 32 bits hold t0 + kTile
    __syncthreads();   // edges, zeroed plane and counter ready; the previous tile's scan is over
    for (int i = tid; i < kTile; i += kRowThreads) {
      const uint32_t j = t0 + i;
      double p = 0.0;
      int32_t b[NS];
#pragma unroll
      for (int u = 0; u < NS; ++u) b[u] = -1;
      if (j < S) {
        p = P * sample_mass(ll[j], m, W, usable);
        int32_t c[NS];
        // A sample at or below the sample threshold (or with a NaN p) contributes nothing: no walk, no bin
        // lookup.  The threshold is tested before the switch: p_thresh_sample < p_switch (validate_population_
        // grid), so a sample that reaches the large list has passed it.
        bool any = false;
        if (p > a.p_thresh_sample && walk_chain<NS>(r, row, (int32_t)j, NS, c)) {
#pragma unroll
          for (int u = 0; u < NS; ++u) {
            b[u] = sample_bin(r, cut, s_ez, s_en, zmin, zmax, c[u]);
            any = any || b[u] >= 0;
          }
        }
        if (any && p >= a.p_switch) {               // kept exactly; never enters the Poisson plane
          push_candidate<kBinSlots, NS>(cand, p, (int32_t)j, b);
#pragma unroll
          for (int u = 0; u < NS; ++u) b[u] = -1;
        }                                           // (p >= p_switch with no slot inside: every b is -1)
      }
      s_p[i] = p;
#pragma unroll
      for (int u = 0; u < NS; ++u) s_bin[i * NS + u] = b[u];
    }
    __syncthreads();
    scan_tile(s_bin, (int)min((uint32_t)kTile, S - t0) * NS, tid, [&](int e, int b) { s_pl[b] += s_p[e / NS]; });
  }
  __syncthreads();
  double* out = a.poisson + o * nb;
  for (int i = tid; i < nb; i += kRowThreads) out[i] = s_pl[i];
  if (tid == 0)
    write_candidates<kBinSlots>(cand, a.large_inds + o * kPopulationMaxLarge, a.large_probs + o * kPopulationMaxLarge,
                                a.large_bins + o * kPopulationMaxLarge * kBinSlots);
}

// ---- posterior intervals (posterior_intervals.hip): the mass of one absorber slot goes
// into histograms over the dense ranks of its values, filled with scan_tile's owned-bin pattern: first coarse
// bins rank >> s, then the 2^s ranks of the coarse bin each quantile level selected
constexpr int kIntervalTile = 512;          // samples staged per pass: a mass and one bin per parameter
constexpr int kIntervalCoarseBins = 1024;
constexpr int kIntervalFineCells = 2048;    // (level, rank) cells of one parameter's fine histograms per pass
constexpr int kIntervalQuantiles = 8;       // kIntervalMaxLevels
// the smallest shift that leaves at most kIntervalCoarseBins bins of S ranks: 0 up to S = 1024, 10 at 2^20
__host__ __device__ inline int interval_shift(int64_t S) {
  int s = 0;
  while (((S - 1) >> s) >= kIntervalCoarseBins) ++s;
  return s;
}
// quantile levels whose fine histograms share a pass: all of them up to s = 8, 4 at s = 9, 2 at s = 10
__host__ __device__ inline int interval_group(int s, int nq) {
  const int g = kIntervalFineCells >> s;
  return g < nq ? (g < 1 ? 1 : g) : nq;
}
// cells of one parameter's histogram region: the coarse bins, or the fine cells of a group if there are more
__host__ __device__ inline int interval_cells(int64_t S, int nq) {
  const int s = interval_shift(S);
  const int coarse = (int)((S - 1) >> s) + 1, fine = s ? interval_group(s, nq) << s : 0;
  return coarse > fine ? coarse : fine;
}
struct IntervalLds {
  size_t red_v, red_i, res, target, base_c, base, pick_c, rank, pick, last, hist, mass, bin_z, bin_n, total;
  __host__ __device__ size_t take(size_t bytes) { const size_t o = total; total = up16(total + bytes); return o; }
};
constexpr int kIntervalResults = kIntervalQuantiles + 4;   // per (parameter, slot): quantiles, mean, sd, lo, hi
// 9,536 B + 16 B per cell: 19,536 B at S = 10^4 (625 coarse bins), 25,920 B at 1,024 bins, and at most 42,304 B
// (2,048 fine cells: eight levels at s = 8, or any group from s = 9 on, S = 2^20 included)
__host__ __device__ inline IntervalLds interval_lds(int64_t S, int nq) {
  IntervalLds l{};
  l.red_v = l.take(kRowWaves * 8);
  l.red_i = l.take(kRowWaves * 4);
  l.res = l.take((size_t)2 * 4 * kIntervalResults * 8);
  l.target = l.take(2 * kIntervalQuantiles * 8);   // per parameter and level: level * T
  l.base_c = l.take(2 * kIntervalQuantiles * 8);   // the coarse cdf before the selected bin
  l.base = l.take(kIntervalQuantiles * 8);         // a selection's result: the cdf before the bin taken
  l.pick_c = l.take(2 * kIntervalQuantiles * 4);   // the selected coarse bin
  l.rank = l.take(2 * kIntervalQuantiles * 4);     // the selected rank
  l.pick = l.take(2 * kIntervalQuantiles * 4);     // a selection: first candidate bins, then the bins taken
  l.last = l.take(4);
  l.hist = l.take((size_t)2 * interval_cells(S, nq) * 8);
  l.mass = l.take((size_t)kIntervalTile * 8);
  l.bin_z = l.take((size_t)kIntervalTile * 4);
  l.bin_n = l.take((size_t)kIntervalTile * 4);
  return l;
}

// sum of one value per thread in row_weight_sum's order (xor butterfly, waves in order); every thread returns
// the same value and s_rv is free again on return
__device__ __forceinline__ double row_sum(double loc, int tid, double* s_rv) {
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) loc += __shfl_xor(loc, o);
  if (lane == 0) s_rv[wave] = loc;
  __syncthreads();
  double W = s_rv[0];
#pragma unroll
  for (int w = 1; w < kRowWaves; ++w) W += s_rv[w];
  __syncthreads();
  return W;
}
// min (kMax false) or max over one value per thread: exact, so any order serves
template <bool kMax>
__device__ __forceinline__ double row_extreme(double loc, int tid, double* s_rv) {
  const int lane = tid & 63, wave = tid >> 6;
  auto pick = [](double a, double b) { return kMax ? (b > a ? b : a) : (b < a ? b : a); };
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) loc = pick(loc, __shfl_xor(loc, o));
  if (lane == 0) s_rv[wave] = loc;
  __syncthreads();
  double v = s_rv[0];
#pragma unroll
  for (int w = 1; w < kRowWaves; ++w) v = pick(v, s_rv[w]);
  __syncthreads();
  return v;
}
__device__ __forceinline__ int32_t row_count(int32_t loc, int tid, int32_t* s_ri) {
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) loc += __shfl_xor(loc, o);
  if (lane == 0) s_ri[wave] = loc;
  __syncthreads();
  int32_t v = 0;
#pragma unroll
  for (int w = 0; w < kRowWaves; ++w) v += s_ri[w];
  __syncthreads();
  return v;
}

// The cdf of a histogram of nb <= 4 kRowThreads bins as a fixed-order scan, and the bins nt targets select.
// Thread t sums its bins 4t .. 4t + 3 in order; the 256 thread sums go through a 64-lane shift scan and the
// waves in order; cdf(b) = base + (sum of the threads before) + (the thread's own partial up to b).  Target k
// is s_tgt[k], or with kScale s_tgt[k] = level[k] * total is formed here first.  The bin taken for it is the
// smallest non-empty b with cdf(b) >= target, or the last non-empty bin when rounding leaves none; s_pick[k]
// receives it and s_base[k] the cdf before it.  s_pick needs 2 nt entries.  Returns the total (every thread the
// same value); when it is not > 0 nothing is selected and s_pick / s_base are not to be read.
template <bool kScale>
__device__ __forceinline__ double hist_select(const double* h, int nb, double base, const double* level, double* s_tgt,
                                              int nt, int tid, double* s_rv, int32_t* s_pick, double* s_base,
                                              int32_t* s_last) {
  const int lane = tid & 63, wave = tid >> 6, b0 = 4 * tid;
  double a[4], p[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = b0 + i < nb ? h[b0 + i] : 0.0;
  p[0] = a[0];
#pragma unroll
  for (int i = 1; i < 4; ++i) p[i] = p[i - 1] + a[i];
  double v = p[3];
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double n = __shfl_up(v, o);
    if (lane >= o) v += n;
  }
  double ex = __shfl_up(v, 1);
  if (lane == 0) ex = 0.0;
  if (lane == 63) s_rv[wave] = v;
  if (tid < nt) s_pick[tid] = INT32_MAX;
  if (tid == 0) *s_last = -1;
  __syncthreads();
  double pre = 0.0, total = 0.0;
#pragma unroll
  for (int w = 0; w < kRowWaves; ++w) {
    if (w == wave) pre = total;
    total += s_rv[w];
  }
  if (kScale && tid < nt) s_tgt[tid] = level[tid] * total;
  if (!(total > 0.0)) {
    __syncthreads();
    return total;
  }
  if (kScale) __syncthreads();
  const double off = base + (pre + ex);
  for (int k = 0; k < nt; ++k) {
    const double t = s_tgt[k];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (a[i] > 0.0 && off + p[i] >= t) { atomicMin(&s_pick[k], b0 + i); break; }   // integer, LDS
  }
#pragma unroll
  for (int i = 3; i >= 0; --i)
    if (a[i] > 0.0) { atomicMax(s_last, b0 + i); break; }
  __syncthreads();
  for (int k = 0; k < nt; ++k) {
    int32_t b = s_pick[k];
    if (b == INT32_MAX) b = *s_last;
    if ((b >> 2) == tid) {            // total > 0: some bin is non-empty, b >= 0
      s_pick[nt + k] = b;
      const int i = b & 3;
      s_base[k] = i == 0 ? off : off + (i == 1 ? p[0] : i == 2 ? p[1] : p[2]);
    }
  }
  __syncthreads();
  return total;
}

// ---- the model posteriors of spectrum q (process.py model_posteriors / model_posteriors_multi /
// model_posteriors_sub): e[i] = exp(lp_i - max) over the columns no-DLA, DLA levels 1..D, then (sub) the sub-DLA
// model (n columns), and their sum.  A NaN evidence at a level >= 2 enters as -inf; any other NaN makes every
// posterior NaN, as numpy's max and sum propagate it: false then, with e and sum unset.
__device__ __forceinline__ bool model_posterior_terms(const ModelPosteriorArgs& a, int q, double (&e)[kMaxDlas + 2],
                                                      double& sum, int& n) {
#pragma clang fp contract(off)
  double lp[kMaxDlas + 2];
  n = 0;
  lp[n++] = a.lp_no[q] + a.ll_null[q];
  for (int d = 0; d < a.levels; ++d) {
    double v = a.lp_dla[(int64_t)d * a.ld_prior + q] + a.ll_dla[(int64_t)d * a.rows + q];
    if (d >= 1 && v != v) v = -INFINITY;
    lp[n++] = v;
  }
  if (a.ll_lls) lp[n++] = a.lp_lls[q] + a.ll_lls[q];
  double mx = lp[0];
  bool nan = mx != mx;
  for (int i = 1; i < n; ++i) {
    nan = nan || lp[i] != lp[i];
    if (lp[i] > mx) mx = lp[i];
  }
  if (nan) return false;
  sum = 0.0;
  for (int i = 0; i < n; ++i) { e[i] = exp(lp[i] - mx); sum += e[i]; }
  return true;
}

}  // namespace gpdla
