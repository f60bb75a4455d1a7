// Internal declarations shared by the kernels and the C-ABI layer.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "line_profile.h"
#include "lyman_series.h"
#include "tuning.h"

// HIP call -> C-ABI status (GPDLA_ENOMEM / GPDLA_EDEVICE with a message), in functions returning int
#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return ::gpdla::set_error(e_ == hipErrorOutOfMemory ? GPDLA_ENOMEM : GPDLA_EDEVICE,   \
                                "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),      \
                                __FILE__, __LINE__);                                        \
  } while (0)

// The same for the stand-alone calls, whose messages begin with the call's name: "<ctx>: <expr> failed: ..."
#define HIP_TRY_IN(ctx, expr)                                                                       \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess)                                                                           \
      return ::gpdla::set_error(e_ == hipErrorOutOfMemory ? GPDLA_ENOMEM : GPDLA_EDEVICE,           \
                                ctx ": %s failed: %s", #expr, hipGetErrorString(e_));               \
  } while (0)

namespace gpdla {

// C-ABI error reporting shared by the translation units (engine.hip): sets gpdla_last_error()
int set_error(int code, const char* fmt, ...);
// GPDLA_OK if `device` is a usable HIP device, else GPDLA_EDEVICE / GPDLA_EINVAL (no CPU fallback)
int check_device(int32_t device);

// Launch times of the calling thread's last one-shot call (ingest, sampler): HIP events around each
// kernel on the null stream, read back by gpdla_last_call_kernel_ms (engine.hip).  Usage: reset()
// at the call's start, before() / after() around each launch, then finish() once the call's last
// synchronous copy has returned.
struct LaunchTimes {
  static constexpr int kMax = 8;
  hipEvent_t ev[2 * kMax] = {};
  double ms[kMax] = {};
  int n = 0, done = 0;
  void reset() { n = done = 0; }
  void before() {
    if (n < kMax && (ev[2 * n] || hipEventCreate(&ev[2 * n]) == hipSuccess)) (void)hipEventRecord(ev[2 * n], 0);
  }
  void after() {
    if (n < kMax && (ev[2 * n + 1] || hipEventCreate(&ev[2 * n + 1]) == hipSuccess)) {
      (void)hipEventRecord(ev[2 * n + 1], 0);
      ++n;
    }
  }
  void finish() {
    for (int i = 0; i < n; ++i) {
      float t = 0.0f;
      ms[i] = hipEventSynchronize(ev[2 * i + 1]) == hipSuccess && hipEventElapsedTime(&t, ev[2 * i], ev[2 * i + 1]) ==
                  hipSuccess ? (double)t : -1.0;
    }
    done = n;
  }
};
LaunchTimes& launch_times();

// ---------------------------------------------------------------------------------------------
// Device data layout (HBM)
//
// A spectrum is turned into J "slots" (pixels the likelihood sweeps).  In reference mode slot j is
// the j-th unmasked in-range pixel and its absorption is the j-th value of the m-point profile
// (process_qsos.m:180,189); in unmasked mode J = m and masked slots carry weight 0.
//
// The sweep is split into 4 contiguous segments of L = ceil(J/4) slots (segment g = slots
// [gL, gL+L)); lanes g = 0..3 of a wave walk their segment in step, so the 7-tap instrument
// convolution is a register sliding window and the 4 segments form the K=4 dimension of a
// v_mfma_f64_4x4x4_4b.
//
// Panel row (one per slot, kRow doubles, 16-byte aligned): the Khatri-Rao row
//     e < NGRAM      : M_r * M_c  for Gram pair e = (r, c), r <= c (row-major upper triangle)
//     NGRAM..4GT-1   : 0 (tile padding)
//     4GT + i, i < K : M_i                       (the u = M' D^-1 diag(a) r contraction)
// stored permuted as row[(e & 3) * JS + (e >> 2)], so a lane with j = e & 3 reads consecutive
// tiles with one ds_read_b128.  Spare words per j hold the slot scalars.
// ---------------------------------------------------------------------------------------------
template <int K>
struct Layout {
  static constexpr int kNGram = K * (K + 1) / 2;
  static constexpr int kGT = (kNGram + 3) / 4;  // Gram tiles (4 entries each)
  static constexpr int kUT = (K + 3) / 4;       // u tiles
  static constexpr int kTiles = kGT + kUT;
  static constexpr int kJS = ((kTiles + 2) + 1) & ~1;  // per-j stride (doubles), even
  static constexpr int kRow = 4 * kJS;                 // doubles per slot row (HBM panel stride)
  static constexpr int kRowL = (kRow + 127) & ~127;    // DMA span per row: whole 1 KiB pieces
  static constexpr int kPieces = kRowL / 128;          // global_load_lds_dwordx4 per staged row
  // LDS row stride: the span plus 16 B, so the 4 segment rows a ds_read_b128 lane group touches
  // start in different bank quads (with the bare span, rows g and g+1 hit the same banks: every
  // B-operand read was a 2-way conflict, SQ_LDS_BANK_CONFLICT = 36% of LDS cycles, profiles/r1f)
  static constexpr int kRowS = kRowL + 2;
  static constexpr int kES = 4 * kTiles + 8;           // epilogue doubles per sample (Gram, u, scalars)
  // slot scalars in the spare words
  static constexpr int kLam = 0 * kJS + kTiles;        // padded wavelength at slot + 6
  static constexpr int kY = 0 * kJS + kTiles + 1;
  static constexpr int kNoise = 1 * kJS + kTiles;
  static constexpr int kMu = 1 * kJS + kTiles + 1;
  static constexpr int kOmega2 = 2 * kJS + kTiles;
  static constexpr int kValid = 2 * kJS + kTiles + 1;
};

struct SpecInfo {
  int32_t J;          // slots (0 => unusable spectrum)
  int32_t L;          // segment length ceil(J/4)
  int32_t n;          // unmasked in-range pixels (the n in n*log(2 pi))
  int32_t m;          // in-range pixels including masked
  double zmin, zmax;  // process_qsos.m:160-161
  int64_t slot_base;  // first panel row of this spectrum
  int64_t lam_base;   // first element of this spectrum's padded-wavelength array
  int32_t flags;
  int32_t scale_e;    // prep's unit scaling: noise, omega^2 x 2^scale_e; flux, mu, M x 2^(scale_e / 2)
  double de_shift;    // -n scale_e: log det D = log det D' + de_shift ln 2 (exact power-of-two scaling)
};

constexpr int kChunkSteps = 4;       // pixel steps staged per LDS chunk
constexpr int kSamplesPerWave = 16;
constexpr int kWavesPerBlock = 4;
constexpr int kSamplesPerBlock = kSamplesPerWave * kWavesPerBlock;

struct PrepArgs {
  int32_t q_count;
  const int64_t* offsets;        // device, [q_count + 1], relative to the pixel arrays below
  const double* wavelengths;
  const double* flux;
  const double* noise;
  const uint8_t* mask;
  const double* z_qsos;          // device, [q_count]
  const int64_t* slot_base;      // device, [q_count]
  const int64_t* lam_base;       // device, [q_count]
  const int64_t* slot_cap;       // device, [q_count]
  // model (device, rest grid row-major [G][K])
  int32_t num_rest;
  const double* rest;
  const double* mu;
  const double* M_rowmajor;
  const double* log_omega;
  double c_0, tau_0, beta;
  // params
  double min_lambda, max_lambda, lya, lyman_limit, min_z_cut, max_z_cut, pixel_spacing;
  int32_t absorption_mode;
  int32_t k;                     // rank (read by the panel-GEMM layout, prep_kernel<0>)
  int32_t om2_hi_e;              // binary exponent of the model's largest omega^2 (1 + c_0)^2 (units)
  // outputs
  SpecInfo* info;
  double* panel;                 // fused layout: [slots][kRow]; GEMM layout: [slots][k(k+1)/2] (nullptr:
                                 // the int8 panel paths form the Khatri-Rao entries from panel_m themselves)
  double* panel_m;               // GEMM layout only: [slots][k] M rows
  double* srow;                  // GEMM layout only: [slots][8] lam, y, noise, mu, om2, valid
  double* lam_pad;
  int32_t* slot_pixel;           // scratch map slot -> pixel (size = total slot capacity)
};

// Line-profile data.  Device buffer layout (doubles):
//   [kMaxLines][kCoreTable] core tables | [kMaxLines][kWingStride] wing polynomials |
//   fac[kMaxLines] | 2^(j/64)[64]
// fac_j = c / (lambda_j 1e8) / (sigma sqrt 2), so x_j = lambda * fac_j / (1 + z) - c / (sigma sqrt 2)
// (voigt.c:278-279,287 divided by sigma sqrt 2).
constexpr size_t kLineBufWing = (size_t)kMaxLines * kCoreTable;
constexpr size_t kLineBufFac = kLineBufWing + (size_t)kMaxLines * kWingStride;
constexpr size_t kLineBufExp2 = kLineBufFac + kMaxLines;  // 2^(j/64), j = 0..63 (exp_tab64)
constexpr size_t kLineBufExp128 = kLineBufExp2 + 64;      // 2^(j/128), j = 0..127 (exp_tab128_nc)
constexpr size_t kLineBufDoubles = kLineBufExp128 + 128;

struct LineArgs {
  const double* buf;   // device line buffer (layout above)
};

// ---- panel-GEMM path (any rank 1..kGemmMaxK; gemm_path.hip + gemm_f64.hip or gemm_i8.hip)
constexpr int kGemmMaxK = 64;
constexpr int kWeightQuarters = 4;                 // weights_kernel: waves per segment
// weights kernels: raw profiles per fix-up branch (raw_profile3_batch).  configs[4] A/B: 2 beats 1 and
// 4 (4 needs more registers than 4 waves per SIMD allow; profiles/r4k)
constexpr int kWB = 2;
constexpr int kWeightParts = 4 * kWeightQuarters;  // per-sample partial sums (segment x quarter)

struct WeightsArgs {
  const SpecInfo* info;
  int32_t q;                     // spectrum within the batch
  const double* srow;            // this spectrum's slot scalars [cap][8]
  const double* lam_pad;         // this spectrum's padded wavelengths
  int64_t cap;                   // this spectrum's slot capacity (GEMM inner dimension)
  const double* offsets;         // [S] ascending offsets
  const double* nhi;             // [S]
  int64_t S, s0;                 // chunk = sorted samples s0 .. s0 + sc - 1 (index S = null model)
  int32_t sc;
  int32_t num_lines;
  LineArgs lines;
  double* wg;                    // a^2 / d, weight tiles of gemm_f64 (GemmF64Args)
  double* wu;                    // a r / d, likewise
  double* q1p;                   // [sc][kWeightParts] partial sum r^2 / d
  double* ldp;                   // [sc][kWeightParts] partial sum log d
};

struct LdlArgs {
  const SpecInfo* info;
  int32_t q;
  int32_t k;
  const double* G;               // Gram, quad_index(s, e, k(k+1)/2), entries in gram_tile_index order
  const float* G32;              // the same in fp32 (panel_gemm_i8_24), or nullptr: then G is read
  const double* U;               // u, quad_index(s, i, k)
  const double* q1p;
  const double* ldp;
  int64_t S, s0;
  int32_t sc;
  const int32_t* perm;
  double* sample_ll;             // this spectrum's row, or nullptr
  double* ll_null;               // this spectrum's entry
  int32_t* status;
};

hipError_t launch_weights(const WeightsArgs& a, hipStream_t s);
hipError_t launch_ldl_batch(const LdlArgs& a, hipStream_t s);

// Gram / u hand-off between the panel GEMMs (gemm_f64.hip, gemm_i8.hip) and ldl_mfma_kernel:
// samples in groups of 4, entry e of sample s at (s >> 2) 4 n + 4 e + (s & 3) (n = entries per
// sample).  A GEMM lane's 4 consecutive samples of one entry are one 16-B (fp32) or 32-B store, and
// the LDL^T wave (4 samples x the 16 positions of a tile) reads 64 consecutive values.  Buffers
// cover whole GEMM sample tiles (gemm_f64_rows), so the GEMMs store without a sample bound.
__host__ __device__ inline int64_t quad_index(int64_t s, int64_t e, int64_t n) {
  return (s >> 2) * 4 * n + 4 * e + (s & 3);
}

// fp64 Gram / u GEMM of the panel path (gemm_f64.hip).  The weights are stored per 32-sample tile
// as [tile][slot (cap16)][32], sample 4 g + i of the tile at position 8 i + g (weights_kernel), for
// whole 128-sample blocks (sc rounded up to kGemmF64TileS)
constexpr int kGemmF64Waves = GPDLA_F64_WAVES;     // waves per block, 32 samples each
constexpr int kGemmF64TileS = 32 * kGemmF64Waves;
__host__ __device__ inline int64_t gemm_f64_cap16(int64_t cap) { return (cap + 15) / 16 * 16; }
// row strides (doubles) of the panel-GEMM layout's Khatri-Rao rows (k(k+1)/2 entries) and M rows
// (k): rounded up to even so every row starts 16-B aligned for gemm_f64's LDS-DMA pieces
__host__ __device__ inline int64_t gemm_ldp(int k) { return ((int64_t)k * (k + 1) / 2 + 1) / 2 * 2; }
__host__ __device__ inline int64_t gemm_ldm(int k) { return ((int64_t)k + 1) / 2 * 2; }
// doubles read past the last panel / M row by gemm_f64 (the pad rows up to cap16 and a 128-entry
// piece starting in the last row); the engine keeps them zeroed
__host__ __device__ inline int64_t gemm_panel_slack(int64_t ld) { return 16 * ld + 128; }
__host__ __device__ inline int64_t gemm_f64_rows(int64_t sc) { return (sc + kGemmF64TileS - 1) / kGemmF64TileS * kGemmF64TileS; }
struct GemmF64Seg {              // one product C = W' P of a launch
  const double* W;               // weight tiles (layout above)
  const double* P;               // [slot][ldp] this spectrum's panel rows
  int64_t ldp;                   // doubles per panel row
  int32_t nent;                  // output entries per sample (k(k+1)/2 Gram, or k u)
  double* C;                     // quad_index(s, e, nent), for every sample of the padded tiles
};
struct GemmF64Args {
  GemmF64Seg seg[2];             // Gram and u, one launch (the u entry tiles after the Gram ones)
  int32_t nseg;
  int64_t cap, cap16;            // slots, and slots padded to 16 (the weights' tile rows)
  int32_t sc;                    // samples of the chunk
};
hipError_t launch_gemm_f64(const GemmF64Args& a, hipStream_t s);

struct LikelihoodArgs {
  int32_t q_count;
  const SpecInfo* info;
  const double* panel;
  const double* lam_pad;
  const double* offsets;         // [S] offset samples (ascending; see engine.hip)
  const double* nhi;             // [S]
  const int32_t* perm;           // [S] sorted sample index -> output sample index
  int64_t S;
  int32_t num_lines;
  LineArgs lines;
  double* sample_ll;             // [q_count][ld] or nullptr
  int64_t ld;
  double* ll_null;               // [q_count]
  int32_t* status;
};

// ---- int8 Ozaki-sliced fused path (kernels_i8.hip; ranks with i8_supported(K))
//
// The Gram/u contraction sum_slot w(sample, slot) P(slot, entry) runs on v_mfma_i32_16x16x64_i8
// exactly in integers: per slot the weights are w~ = a^2/d (omega^2+sigma^2) in [0, 1] (Gram) and
// a r/d / beta in [-1, 1] (u, beta a static per-slot bound), quantised as X_A = rint(w~ 2^30); the
// panel entries P~ = M_r M_c / (omega^2+sigma^2) and M_i beta as X_B = rint(P~ / s_e 2^30) with a
// per-entry power-of-two scale s_e.  X_A + 2^31 is split into 4 bytes (XOR 0x80 -> signed digits,
// offset 0x808080 per slot), X_B into 4 balanced signed base-256 digits; the 13 digit pairs of
// level i + j <= 4 accumulate exactly in int32 per level, and the epilogue forms
//   sum_slot X_A X_B = sum_l 2^(8(6-l)) C_l + 0x808080 * colsum_e
// in fp64.  See DESIGN.md section 4 for the error budget.
template <int K>
struct I8Layout {
  static constexpr int kNGram = K * (K + 1) / 2;
  static constexpr int kGT = (kNGram + 15) / 16;     // Gram tiles (16 entries each)
  static constexpr int kUT = (K + 15) / 16;          // u tiles
  static constexpr int kTiles = kGT + kUT;
  static constexpr int kEnt = 16 * kTiles;           // entries incl. padding (<= 256)
  static constexpr int kUBase = 16 * kGT;            // entry of u_0
  static constexpr int kChunkSlots = 64;             // 4 segments x 16 steps (MFMA K = 64)
  static constexpr int kPlaneBytes = kEnt * 64;      // one digit plane of a chunk
  static constexpr int kChunkBytes = 4 * kPlaneBytes;
  static constexpr int kScal = 8;                    // doubles per slot record
  static constexpr int kScalBytes = kChunkSlots * kScal * 8;
};
constexpr int kI8MaxSlots = 30000;  // int32 level sums stay exact up to 4 * 32767 * 2^14 < 2^31

struct ConvertI8Args {
  int32_t q_count;
  const SpecInfo* info;
  const double* panel;           // fused f64 layout (prep_kernel<K>)
  const double* lam_pad;
  const int64_t* chunk_base;     // device, [q_count]: first i8 chunk of each spectrum
  uint8_t* panel_i8;             // [chunks][4 planes][kEnt][64 B] (16 B granules swizzled)
  double* scal;                  // [chunks][64][8]: lam(+6), y, noise, mu, om2, gscale, uscale, 0
  double* ent;                   // [q_count][2][kEnt]: s_e, colsum_e
};

struct LikelihoodI8Args {
  int32_t q_count;
  const SpecInfo* info;
  const uint8_t* panel_i8;
  const double* scal;
  const double* ent;
  const int64_t* chunk_base;
  const double* lam_pad;
  const double* offsets;
  const double* nhi;
  const int32_t* perm;
  int64_t S;
  LineArgs lines;
  double* scratch;               // [grid blocks][64][Layout<K>::kES]
  double* sample_ll;
  int64_t ld;
  double* ll_null;
  int32_t* status;
};

// ---- int8 Ozaki contraction on the panel-GEMM path (gemm_i8.hip; any rank 1..kGemmMaxK)
// K index of slot (segment g, step t): g Ls16 + t with Ls16 = 16 ceil(L / 16); a spectrum's K
// extent 4 Ls16 is a multiple of 64 and at most kstride = i8_gemm_kstride(slot_cap).
// Entries: Gram 0..E-1 padded to Ep = 64 ceil(E / 64), then u 0..k-1 padded to 64 ceil(k / 64).
__host__ __device__ inline int64_t i8_gemm_kstride(int64_t slot_cap) {
  return 64 * ((slot_cap - 16 + 63 + 63) / 64);  // >= lpix + 63 >= 4 Ls16 (slot_cap = 4 ceil(lpix/4) + 16)
}
// Order of the k(k+1)/2 Gram entries (r <= c < k) in the panel-GEMM path's Khatri-Rao rows and
// Gram arrays: tile-major over the 4 x 4 tiles the LDL^T factors (gemm_path.hip ldl_mfma_kernel), so
// the 16 lanes reading one tile of a sample read 128 contiguous bytes.  With NT = ceil((k+1)/4) tiles
// per side, the first 4 (NT - 1) columns form whole tile columns: tiles (L, I), L <= I <= NT - 2,
// row-block major, 10 entries (upper triangle, i <= j) on the diagonal and 16 (i-major) off it.  The
// w = k - 4 (NT - 1) <= 3 Gram columns of the last tile column follow: 4 w entries per tile (L, NT-1),
// L < NT - 1, then the w (w + 1) / 2 of the corner tile.
__host__ __device__ inline int gram_tile_index(int r, int c, int k) {
  const int NT = (k + 4) / 4, Kf = 4 * (NT - 1), w = k - Kf;
  const int L = r >> 2, I = c >> 2, i = r & 3, j = c & 3;
  if (c < Kf) {
    const int row = 10 * L + 16 * (L * (NT - 2) - L * (L - 1) / 2);
    return row + (I == L ? i * 4 - i * (i - 1) / 2 + (j - i) : 10 + 16 * (I - L - 1) + 4 * i + j);
  }
  const int base2 = 10 * (NT - 1) + 8 * (NT - 1) * (NT - 2);
  return base2 + L * 4 * w + (L == NT - 1 ? i * w - i * (i - 1) / 2 + (j - i) : i * w + j);
}

// The 24-bit path's error is absolute, ~2^-24 of the Gram's scale: relative to max(|ll|, 1) it grows
// where |ll| is small, which short spectra make likely (n = 3: 5.05e-7 against the fp64 panel,
// profiles/round5/r10b).  Spectra of at most kI8NarrowKs 64-slot K steps (<= 128 pixels) therefore
// take the 32-bit digits (4 planes, ~1e-9) on that path; they cost next to nothing.  Decided on the
// slot capacity (host and device agree without a sync): ks_bound = ceil(ceil(lpix / 4) / 16).
constexpr int kI8NarrowKs = 2;
__host__ __device__ inline int i8_ks_bound(int64_t slot_cap) { return (int)(((slot_cap - 16) / 4 + 15) / 16); }
__host__ __device__ inline int i8_spectrum_nd(int nd, int64_t slot_cap) {
  return (nd == 3 && i8_ks_bound(slot_cap) <= kI8NarrowKs) ? 4 : nd;
}

__host__ __device__ inline int i8_gemm_entries(int k) {
  return 64 * ((k * (k + 1) / 2 + 63) / 64) + 64 * ((k + 63) / 64);
}

struct ConvertGemmI8Args {
  int32_t k;
  const SpecInfo* info;
  const double* panel_m;         // [slots][k] M rows (the Khatri-Rao entries are formed from them)
  const double* srow;            // [slots][8]
  const int64_t* slot_base;      // device [q]
  const int64_t* slot_cap;       // device [q]
  const int64_t* bbase;          // device [q]: byte offset of the spectrum's B digit planes
  int32_t nd;                    // Gram digit planes written: 4 (levels <= 3) or 3 (levels <= 2); u: 4
  uint8_t* bdig;                 // [planes 4][entries][kstride] per spectrum
  double* ent;                   // [q][2][entries]: s_e / scaleA, c * colsum_e
};

struct WeightsI8Args {
  const SpecInfo* info;
  int32_t q;
  const double* srow;            // this spectrum's slot scalars
  const double* lam_pad;         // this spectrum's padded wavelengths
  int64_t kstride;
  const double* offsets;
  const double* nhi;
  int64_t S, s0;
  int32_t sc;
  int64_t rows;                  // sample rows allocated per digit plane (>= sc, multiple of 128)
  LineArgs lines;
  int32_t nd;                    // Gram digit planes written (4 or 3); u: 4
  uint8_t* adig;                 // [type 2 (Gram, u)][plane 4][rows][kstride]
  double* q1p;
  double* ldp;
};

struct GemmI8Args {
  const SpecInfo* info;
  int32_t q;
  int32_t k;
  int64_t kstride;
  int64_t rows;
  int32_t sc;
  int32_t nd;                    // Gram digit planes per operand: 4 (10 pairs, levels <= 3) or 3 (6 pairs); u: 4
  int32_t e_tile0, ny;           // set by launch_gemm_i8: first 64-entry tile and tile count of a launch
  int32_t ks_bound;              // bound on the spectrum's 64-slot K steps, ceil(ceil(lpix / 4) / 16)
  int32_t u_tile;                // set by launch_gemm_i8: the u entry tile fused into the Gram launch, or -1
  const uint8_t* adig;
  const uint8_t* bdig;           // this spectrum's B planes
  const double* ent;             // this spectrum's [2][entries]
  double* G;                     // quad_index(s, e, E), every sample of the rows
  float* G32;                    // if set, the Gram goes here in fp32 instead (24-bit path)
  double* U;                     // quad_index(s, i, k)
};

hipError_t launch_convert_gemm_i8(const ConvertGemmI8Args& a, int32_t q_count, hipStream_t s);
hipError_t launch_weights_i8(const WeightsI8Args& a, hipStream_t s);
hipError_t launch_diag_raw_profile(const double* lam, int64_t n, double z, double N, int32_t f32,
                                   const LineArgs& lines, double* out, hipStream_t s);
hipError_t launch_gemm_i8(const GemmI8Args& a, hipStream_t s);

bool i8_supported(int K);
int i8_fused_rank(int k);
int i8_chunk_bytes(int K);
int i8_entries(int K);
hipError_t launch_convert_i8(int K, const ConvertI8Args& a, hipStream_t s);
hipError_t launch_likelihood_i8(int K, const LikelihoodI8Args& a, hipStream_t s);

struct ReduceArgs {
  int32_t q_count;
  const SpecInfo* info;
  const double* sample_ll;
  int64_t ld;
  int64_t S;
  double* ll_dla;
  double* zmin;
  double* zmax;
  int32_t* num_pixels;
};

hipError_t launch_prep(int K, const PrepArgs& a, hipStream_t s);
hipError_t launch_likelihood(int K, const LikelihoodArgs& a, hipStream_t s);
hipError_t launch_reduce(const ReduceArgs& a, hipStream_t s);
hipError_t launch_voigt_batch(const double* lambdas, int64_t n_padded, const double* z,
                              const double* N, int64_t count, int32_t num_lines,
                              const LineArgs& lines, double* out, hipStream_t s);
hipError_t launch_mvn_single(const double* y, const double* mu, const double* M_colmajor,
                             const double* d, int64_t n, int32_t k, double* out,
                             int32_t* status, hipStream_t s);
bool rank_supported(int K);
int fused_rank(int k);
int panel_row_doubles(int K);
int panel_lds_row_doubles(int K);
int scratch_doubles(int K);

// ---- multi-DLA levels (multi_dla.hip; fused fp64 layout, num_lines = 3)
constexpr int kMaxDlas = 4;
constexpr int kMaxChain = kMaxDlas - 1;   // base DLAs a sample can carry

// Level d = 1 + chain_len: sample j (caller order) carries its own DLA and those of the samples
// chain[(q S + j) kMaxChain + i], i < chain_len (caller-order indices; -1 = no chain: NaN output).
struct MultiLevelArgs {
  int32_t q_count;
  const SpecInfo* info;
  const double* panel;
  const double* lam_pad;
  const double* offsets;         // [S] ascending (the sweep order)
  const double* nhi;             // [S] in sweep order
  const int32_t* perm;           // [S] sweep index -> caller's sample index
  const double* offsets_c;       // [S] caller order
  const double* nhi_c;           // [S] caller order
  const int32_t* chain;          // [q_count][S][kMaxChain]
  int32_t chain_len;             // d - 1
  int64_t S;
  LineArgs lines;
  double min_z_separation;
  double* sample_ll;             // [q_count][ld]
  int64_t ld;
  int32_t* status;
};

// Steps 1-3 of a level (weights, prefix sum, S searches, next chain table), one block per row.
struct ResampleArgs {
  int32_t rows;
  const double* ll;              // [rows][ld] previous level, caller order
  int64_t ld;
  int64_t S;
  const double* u;               // [S] uniforms of this level; unused with forced
  const int32_t* forced;         // [rows][S] base indices to use instead of resampling, or nullptr
  double* cws;                   // [rows][S] prefix-sum workspace, read only when S > kResampleLds
  const int32_t* chain_prev;     // [rows][S][kMaxChain] or nullptr (no chain output)
  int32_t prev_len;              // entries of chain_prev in use (d - 2)
  int32_t* chain_next;           // [rows][S][kMaxChain] or nullptr
  int32_t* base_inds;            // [rows][S] out
};

// NaN-aware log-mean-exp of a level >= 2, minus the Occam penalty
struct MultiReduceArgs {
  int32_t q_count;
  const double* sample_ll;
  int64_t ld;
  int64_t S;
  double penalty;                // (d - 1) occam_log_penalty
  double* ll_dla;                // [q_count]
};

bool multi_level_supported(int K);
hipError_t launch_multi_level(int K, const MultiLevelArgs& a, hipStream_t s);
hipError_t launch_resample(const ResampleArgs& a, hipStream_t s);
hipError_t launch_multi_reduce(const MultiReduceArgs& a, hipStream_t s);

// ---- the sample rows the summary and population kernels reduce (row_posterior.h), and the grid they bin on
constexpr int kSummaryPlanes = 5;        // sum pi, pi^2, N pi, N^2 pi, N^2 pi^2 per bin
constexpr int kSummaryMaxBins = 1024;
constexpr int kPopulationMaxLarge = 8;
constexpr int kPmfChunk = 512;           // trials per chunk polynomial
struct SampleRowsArgs {
  int32_t rows, levels;
  const double* ll;              // [levels][rows][ld], caller's sample order
  int64_t ld, S;
  const int32_t* base;           // [levels - 1][rows][ld_base] base indices, or nullptr (levels = 1)
  int64_t ld_base;
  const double* offset;          // [S] caller order
  const double* log_nhi;         // [S]
  const double* zmin;            // [rows]
  const double* zmax;            // [rows]
  int32_t nz, nn;                // grid (ignored by a summary without planes)
  const double* z_edges;         // device [nz + 1]
  const double* n_edges;         // device [nn + 1]
  // search cuts (search_cuts.hip), all device arrays; both tests off when the pointers
  // are null, and the launch then gives the outputs of a launch without these fields bit for bit
  const double* cut_z_upper;     // [rows], or nullptr: no proximity test (a slot needs z < cut_z_upper[row])
  const int32_t* cut_npix;       // [rows], or nullptr: no pixel test
  const int64_t* cut_word_off;   // [rows + 1] with cut_npix: the row's first word of cut_words
  const uint32_t* cut_words;     // bit i of a row's stretch set: pixel i is good
};
// the launch functions' check of the rows, and with `grid` of the bin counts
inline bool sample_rows_ok(const SampleRowsArgs& r, bool grid = true) {
  return r.S >= 1 && r.S <= INT32_MAX && r.levels >= 1 && r.levels <= kMaxDlas && r.ld >= r.S &&
         (r.levels == 1 || (r.base && r.ld_base >= r.S)) &&
         (!grid || (r.nz >= 1 && r.nn >= 1 && (int64_t)r.nz * r.nn <= kSummaryMaxBins));
}

// ---- posterior summaries (posterior_summary.hip): MAP sample and chain parameters per (row, level),
// binned normalised masses of level 1
struct SummaryArgs {
  SampleRowsArgs r;
  const double* nhi;             // [S]
  int32_t* map_ind;              // [levels][rows]
  double* map_ll;                // [levels][rows]
  double* map_z;                 // [levels][rows][kMaxDlas]
  double* map_n;                 // [levels][rows][kMaxDlas]
  double* planes;                // [rows][kSummaryPlanes][nz nn], or nullptr: MAP only
};
hipError_t launch_posterior_summary(const SummaryArgs& a, hipStream_t s);

// ---- posterior intervals (posterior_intervals.hip): per (row, level, slot) and parameter the likelihood-ratio
// range, mean and sd, and the quantiles as weighted order statistics over the samples' dense ranks
constexpr int kIntervalMaxLevels = 8;
constexpr int64_t kIntervalMaxSamples = 1 << 20;
struct IntervalArgs {
  SampleRowsArgs r;              // no grid
  const int32_t* rank_z;         // [S] dense rank of offset[i] among the offsets (equal values share one)
  const int32_t* rank_n;         // [S] ... of log_nhi[i]
  const double* uniq_off;        // [S] the offset of each rank
  const double* uniq_n;          // [S] the log N_HI of each rank
  double lr_delta;
  int32_t num_levels;
  double levels[kIntervalMaxLevels];
  double *z_mean, *z_sd, *n_mean, *n_sd;   // [levels][rows][kMaxDlas]
  double *z_lr, *n_lr;           // [levels][rows][kMaxDlas][2]
  double *z_q, *n_q;             // [levels][rows][kMaxDlas][num_levels]
  int32_t* lr_count;             // [levels][rows]
};
hipError_t launch_posterior_intervals(const IntervalArgs& a, hipStream_t s);
// rank[i] = the dense rank of x[i] (ascending, equal values share a rank, NaNs last and together) and
// uniq[r] = the value of rank r (NaN past the last rank); both [S]
void build_rank_table(const double* x, int64_t S, int32_t* rank, double* uniq);
// GPDLA_EINVAL with a message unless lr_delta, the quantile levels and S are usable
int validate_interval_levels(double lr_delta, int32_t num_levels, const double* levels, int64_t S);

// ---- population statistics (population.hip, level_population.hip): the model posteriors per spectrum
// (p_dla, and the posterior P_d of each DLA level), per (row, level) the binned masses and the split of
// P_d pi_{d,j} into a Poisson plane and a short list of large probabilities with every absorber of a sample's
// base chain counted (include/gpdla.h "Population statistics" and "... over every multi-DLA level"), and the
// Poisson-binomial pmf of CSR trial lists
struct ModelPosteriorArgs {
  int32_t rows, levels;
  const double* ll_null;         // [rows]
  const double* ll_dla;          // [levels][rows]
  const double* ll_lls;          // [rows], or nullptr: no sub-DLA model
  const double* lp_no;           // [rows] log priors
  const double* lp_dla;          // [levels][ld_prior]
  const double* lp_lls;          // [rows] with ll_lls
  int64_t ld_prior;
  double* p_dla;                 // [rows]: launch_model_posterior
  double* level_post;            // [levels][rows]: launch_level_posterior
};
struct LevelPlanesArgs {
  SampleRowsArgs r;
  const double* nhi;             // [S]
  double* planes;                // [rows][levels][kSummaryPlanes][nz nn]
};
// launch_level_split, and with levels = 1 launch_population_split: level_post = p_dla, ld_post = rows, and one
// bin per entry of large_bins
struct SplitArgs {
  SampleRowsArgs r;
  const double* level_post;      // [levels][ld_post]
  int64_t ld_post;
  double p_thresh_sample, p_switch;
  double* poisson;               // [rows][levels][nz nn]
  int32_t* large_inds;           // [rows][levels][kPopulationMaxLarge], -1 = unused
  double* large_probs;           // NaN = unused
  int32_t* large_bins;           // [rows][levels][kPopulationMaxLarge][kMaxDlas] (iz nn + in), -1 = unused
};
using LevelSplitArgs = SplitArgs;
using PopulationSplitArgs = SplitArgs;
struct PmfChunkArgs {
  const double* probs;
  const int64_t* start;          // [chunks] first trial
  const int32_t* len;            // [chunks] 0..kPmfChunk trials
  double* const* dst;            // [chunks] where the len + 1 coefficients go
};
struct PmfFoldArgs {             // the bins of more than one chunk
  const int64_t* n;              // trials
  const int64_t* out_off;        // the bin's offset in either fold buffer (and in the output)
  const int64_t* chunk_off;      // the bin's offset in the chunk store
  const int32_t* nch;            // chunks
  const double* chunks;
  double* buf[2];
};
hipError_t launch_model_posterior(const ModelPosteriorArgs& a, hipStream_t s);
hipError_t launch_level_posterior(const ModelPosteriorArgs& a, hipStream_t s);
hipError_t launch_population_split(const PopulationSplitArgs& a, hipStream_t s);
hipError_t launch_level_planes(const LevelPlanesArgs& a, hipStream_t s);
hipError_t launch_level_split(const LevelSplitArgs& a, hipStream_t s);
// "<prefix><axis>_edges[i] = ...: edges must be finite and strictly increasing" for either grid kind
int validate_grid_edges(const char* prefix, int64_t nz, int64_t nn, const double* z_edges, const double* n_edges);
int validate_population_grid(int64_t nz, int64_t nn, const double* z_edges, const double* n_edges,
                             double p_thresh_sample, double p_switch);

// ---- search cuts (search_cuts.hip): one workgroup per spectrum
struct SearchCutArgs {
  const int64_t* offsets;        // device [Q + 1]
  const double* wavelengths;
  const double* noise;
  const double* zmin;            // [Q]
  const double* zmax;            // [Q]
  double proximity_zone, noise_thresh;   // NaN: off
  double omega_m;
  int32_t nz[2];                 // summary, population; 0: no grid
  const double* z_edges[2];      // device [nz + 1]
  const int64_t* word_off;       // device [Q + 1]
  uint32_t* words;
  int32_t* npix;                 // [Q]
  double* z_upper;               // [Q]
  double* path[2];               // [Q][nz + 1]
};
hipError_t launch_search_cuts(const SearchCutArgs& a, int64_t Q, hipStream_t s);
// GPDLA_EINVAL with a message unless the thresholds, the grids (each with its path array) and omega_m are usable
int validate_search_cuts(const struct gpdla_search_cuts* cuts, const double* path_summary, const double* path_population);

// ---- host staging of the stand-alone entry points: one device allocation carved in 256-byte steps, freed
// when the call returns
struct DeviceStage {
  char* d = nullptr;
  size_t off = 0;
  DeviceStage() = default;
  DeviceStage(const DeviceStage&) = delete;
  DeviceStage& operator=(const DeviceStage&) = delete;
  ~DeviceStage() { if (d) (void)hipFree(d); }
  size_t carve(size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; }
  hipError_t alloc() { return hipMalloc((void**)&d, off ? off : 256); }
  hipError_t upload(size_t o, const void* src, size_t bytes) { return hipMemcpy(d + o, src, bytes, hipMemcpyHostToDevice); }
  hipError_t download(void* dst, size_t o, size_t bytes) { return hipMemcpy(dst, d + o, bytes, hipMemcpyDeviceToHost); }
  template <class T> T* ptr(size_t o) const { return (T*)(d + o); }
};
// The inputs the stand-alone summary and population calls share: the rows, their base indices, the sample
// arrays (nhi may be null), the redshift ranges and the grid's edges (nz = 0: no grid).  check() is the calls'
// common argument check (GPDLA_EINVAL with their messages; `others` = the call's further pointers are set),
// carve() before alloc(), upload() after it: fills r, and the device nhi.
struct HostSampleRows {
  const double* ll;
  int64_t rows, S, ld;
  const double *offset, *log_nhi, *nhi, *min_z, *max_z;
  const int32_t* base;
  int32_t levels;
  int nz, nn;
  const double *z_edges, *n_edges;
  size_t o_ll, o_base, o_off, o_ln, o_nh, o_zmin, o_zmax, o_ed;
  int check(bool others) const;
  void carve(DeviceStage& st);
  hipError_t upload(DeviceStage& st, SampleRowsArgs* r, const double** d_nhi) const;
};

// ---- Lyman-series forest (forest.hip): rewrites the kMu / kOmega2 words of a batch's valid slots
// between prep_kernel and the sweeps (fused fp64 layout only)
struct ForestArgs {
  int32_t q_count;
  const SpecInfo* info;          // written by prep_kernel
  const int64_t* offsets;        // device [q_count + 1], relative to wavelengths (PrepArgs::offsets)
  const double* wavelengths;
  const double* z_qsos;          // device [q_count]
  const int64_t* slot_cap;       // device [q_count]
  const int32_t* slot_pixel;     // prep_kernel's slot -> pixel map
  int32_t num_rest;
  const double* rest;
  const double* log_omega;
  double c_0, tau_0, beta;       // the model's (variance series)
  double mf_tau_0, mf_beta;      // mean flux
  int32_t num_lines;             // L, 1..kMaxLines
  int32_t variance_series, mean_flux;
  int32_t mean_flux_scope;       // what the mean flux multiplies: 0 mu, 1 mu and M, 2 mu, M and omega^2
  int32_t row, w_mu, w_omega2;   // set by launch_forest: Layout<K>::kRow, kMu, kOmega2
  double* panel;
};
hipError_t launch_forest(int K, ForestArgs a, hipStream_t s);
// the M rows (u-words and Khatri-Rao entries) and, under scope 2, the kOmega2 words of the valid slots
// times the mean flux; after launch_forest, only with mean_flux and scope 1 or 2
hipError_t launch_forest_covariance(int K, const ForestArgs& a, hipStream_t s);
// sum_i t_i(tau_0, beta) at n wavelengths (device buffers), the device function forest_kernel calls
hipError_t launch_forest_f64(const double* wl, int64_t n, double z_qso, double tau_0, double beta, int32_t L,
                             double* out, hipStream_t s);

// ---- model spectra (model_spectra.hip): one workgroup per spectrum of a batch whose
// slot panel, padded wavelengths and SpecInfo are resident (after prep_kernel and the forest launches)
struct ModelSpectraArgs {
  int32_t q_count;
  const SpecInfo* info;
  const double* panel;           // fused fp64 layout
  const double* lam_pad;
  const int32_t* slot_pixel;     // prep_kernel's position -> pixel map
  int32_t num_lines;
  LineArgs lines;
  const int32_t* counts;         // [q_count] absorbers 0..kMaxDlas
  const double* z_dlas;          // [q_count][kMaxDlas]
  const double* log_nhis;        // [q_count][kMaxDlas] log10 N_HI
  const double* nhis;            // [q_count][kMaxDlas] N_HI (cm^-2), or nullptr: exp10(log_nhis) on the device
  const int64_t* cap_offsets;    // [q_count + 1] where a spectrum's per-pixel values go, and how many fit
  double* scratch;               // [3][slot capacity of the batch], read only by spectra over GPDLA_MODEL_SPECTRA_LDS
  int64_t scratch_plane;         // doubles per plane of scratch
  int32_t* pixel_inds;           // per pixel, at cap_offsets[q] + 0 .. n - 1
  double *absorption, *model_mean, *continuum_mean, *continuum_sd;
  double *chi2, *log_likelihood; // [q_count]
  int32_t* num_pixels;           // [q_count]
  int32_t* status;               // bit 0: a pivot of B not positive; bit 1: a spectrum over its capacity
};
// The absorbers of a searched batch (gpdla_engine_process_spectra_models): per spectrum the level -- given, or
// the DLA level d in 1..levels with the largest ll_dla[d - 1] + lp_dla[d - 1] (first maximum, NaN ignored, level 1
// when every one is NaN: catalog.absorber_table's rule) -- and that level's MAP pairs of the summary launch
struct ModelLevelArgs {
  int32_t rows, levels;          // spectra of the batch, D
  const double* ll_dla;          // [levels][rows] evidences
  const double* lp_dla;          // [levels][rows] log priors, or nullptr (all equal)
  const int32_t* given;          // [rows] levels 0..D, or nullptr: the best
  const double* map_z;           // [levels][rows][kMaxDlas]
  const double* map_n;           // [levels][rows][kMaxDlas] log10 N_HI
  int32_t* counts;               // [rows] out = the level
  double* z_dlas;                // [rows][kMaxDlas] out
  double* log_nhis;              // [rows][kMaxDlas] out
  int32_t* level_out;            // [rows] out, or nullptr
};
hipError_t launch_model_levels(const ModelLevelArgs& a, hipStream_t s);
// the ranks the fused fp64 kernels are compiled for (kernels.hip, multi_dla.hip and forest.hip spell the same list)
#ifndef GPDLA_FOR_EACH_RANK
#define GPDLA_FOR_EACH_RANK(X) X(4) X(8) X(10) X(12) X(16) X(20) X(24)
#endif
bool model_spectra_supported(int K);
hipError_t launch_model_spectra(int K, const ModelSpectraArgs& a, hipStream_t s);

// host-side table fitting (faddeeva_host.cpp)
void fit_core_table(int line, double* core);
void fit_wing_line(int line, double* wing);
double line_profile_error(int line);

}  // namespace gpdla
