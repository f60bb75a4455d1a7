// tuning.h -- the launch-shape constants chosen by measurement, in one place.
//
// Each value below was picked by an A/B on the MI355X (records under profiles/, DESIGN.md section
// 4); the alternatives lost and their code paths were deleted.  These are the only compile-time
// knobs in the product sources: tools/build_variants.py may override one with -D to rebuild a
// variant library for a new A/B, the product build never does.
#pragma once

// gemm_f64_kernel (fp64 panel path): waves per block, 32 samples each (profiles/r4f, r4g)
#ifndef GPDLA_F64_WAVES
#define GPDLA_F64_WAVES 4
#endif

// gemm_i8_bst_kernel: XCDs sharing a sample tile's A digits (4 / 8 measured -1.3% / -5%, profiles/r5j)
#ifndef GPDLA_BST_EX
#define GPDLA_BST_EX 2
#endif

// panel paths: largest sample chunk per spectrum (2 / 4 / 6 equal chunks lost 2-15%, profiles/r2/c5_ab, r7e)
#ifndef GPDLA_MAX_CHUNK
#define GPDLA_MAX_CHUNK 131072
#endif

// multi_level_kernel (multi_dla.hip): blocks per CU by compiled rank and DLAs per sample.  Not tuned
// by an A/B: the largest occupancy at which every instantiation compiles without scratch (register
// report in DESIGN.md "Multi-DLA"); 2 blocks up to this rank, 1 above it.
#ifndef GPDLA_MULTI_2BLOCK_MAXK_D2
#define GPDLA_MULTI_2BLOCK_MAXK_D2 16
#endif
#ifndef GPDLA_MULTI_2BLOCK_MAXK_D3
#define GPDLA_MULTI_2BLOCK_MAXK_D3 12
#endif
#ifndef GPDLA_MULTI_2BLOCK_MAXK_D4
#define GPDLA_MULTI_2BLOCK_MAXK_D4 0
#endif

// resample_kernel (multi_dla.hip): doubles of the prefix sum kept in LDS (128 KiB of the CU's 160);
// rows with more samples keep it in a global workspace
#ifndef GPDLA_RESAMPLE_LDS
#define GPDLA_RESAMPLE_LDS 16384
#endif

// gemm_i8_bst_kernel: share of an XCD's u sample tiles taken by its two spare blocks (the Gram
// blocks take the rest after their columns); configs[4]: 0.15 / 0.25 / 0.35 / 0.40 / 0.45 / 0.50 /
// 0.55 / 0.65 -> 9.96 / 9.97 / 9.99 / 10.08 / 10.03 / 9.79 / 9.44 / 8.93e7 evals/s (profiles/round5/r10h-j)
#ifndef GPDLA_BST_USPARE
#define GPDLA_BST_USPARE 0.40f
#endif

// bootstrap_gemm_kernel (bootstrap.hip): waves per block (32 replicas each; a block is 32 x waves replicas
// by 128 columns), spectra per LDS stage, spectra per split-K slice (a multiple of the stage) and the most
// replicas of one device chunk (a multiple of the block's replicas).  The slice fixes the reduction order
// over the spectra; chosen for the DR12Q shape (profiles/bootstrap), not swept.
#ifndef GPDLA_BOOT_WAVES
#define GPDLA_BOOT_WAVES 4
#endif
#ifndef GPDLA_BOOT_STAGE_K
#define GPDLA_BOOT_STAGE_K 16
#endif
#ifndef GPDLA_BOOT_KSLICE
#define GPDLA_BOOT_KSLICE 16384
#endif
#ifndef GPDLA_BOOT_MAX_CHUNK
#define GPDLA_BOOT_MAX_CHUNK 1024
#endif

// mix_stage_kernel (count_mixture.hip): lattice cells per 256-thread workgroup (a multiple of 256; each thread
// carries tile / 256 independent FMA chains, and one LDS read of a tap serves that many cells) and taps staged
// in LDS per pass (12 bytes each).  The tile is also the step of mix_scan_kernel, so it fixes the cdf's summation
// order.  Neither was swept; both are first guesses, timed at one shape (profiles/omega_cddf): at these
// values the stage kernel compiles to 27 VGPRs, no scratch and 3 KiB of LDS, so neither registers nor LDS limit
// its occupancy (8 waves per SIMD).
#ifndef GPDLA_MIX_TILE
#define GPDLA_MIX_TILE 1024
#endif
#ifndef GPDLA_MIX_TAPS
#define GPDLA_MIX_TAPS 256
#endif

// model_spectra_kernel (model_spectra.hip): pixel positions of one spectrum whose per-pixel weights (a^2 / d,
// a r / d, a: 24 bytes each) stay in LDS between the kernel's passes; a longer spectrum keeps them in its
// stretch of a global workspace.  Not swept.  At 1e-4 dex the modelled range holds at most 1,250 pixels, so
// 1,024 keeps all but the longest spectra in LDS and lets the tests reach the workspace path with a spectrum
// of the usual kind (n = 1,100).
#ifndef GPDLA_MODEL_SPECTRA_LDS
#define GPDLA_MODEL_SPECTRA_LDS 1024
#endif
