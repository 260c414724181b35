/* libm2h diagnostic surface -- NOT part of the product contract of include/m2h.h.
 *
 * Tuning / test knobs of the library's dispatch code: they only choose between kernels that compute the same values (0 = automatic
 * everywhere).  tests/ use them to pit one engine against another, tools/ for A/B timing, __graft_entry__.smoke() to force the
 * benchmark batch's engine at a small batch.  The state is THREAD-LOCAL (like m2h_set_math_mode: the library holds no process-global
 * mutable state; two host threads may A/B engines side by side): a launch reads the knobs of the host thread that makes it.
 * m2h_tuning_snapshot / m2h_tuning_restore copy the calling thread's whole state (M2H_TUNING_KNOBS ints) out / in: m2h.functional
 * uses them to carry a forward pass's knobs into the autograd thread that runs its backward.
 *
 * Live knobs, one per line: number, macro in csrc/m2h_internal.h, values, the test (or entry point) that uses it as a reference.
 *    0  g_force_splitk    > 0: force this split-K factor of the register engine (and keep the other engines off), -1: never split
 *                         -- tests/test_gpu_unet.py::test_dma_engine_matches_register_engine
 *   10  g_patch_grid      n >= 8: the shared-patch engine's persistent launches take n workgroups instead of one per CU
 *                         -- tests/test_gpu_patch.py (the grid-size test)
 *   11  g_wgrad_blocks    > 0: block-count target of a weight-gradient launch -- tests/grad_routes.py (rows with S = ...)
 *   12  g_wgrad_kt3       -1: narrow weight-gradient blocks always take three k sub-tiles when K allows (0: two where that leaves
 *                         fewer padding columns) -- tests/grad_routes.py
 *   14  (api.hip)         = m2h_set_math_mode (kept for older callers; thread-local like it)
 *   18  g_tap_window      -1: walk every tap even where a whole kernel row / column lies in the padding -- tests/test_gpu_unet.py
 *   21  g_wgrad_row3x3    -1: no image-row 3x3 weight-gradient kernel -- tests/test_gpu_train.py
 *   22  g_row3x3          -1: no image-row 3x3 conv kernels -- tests/test_gpu_train.py
 *   23  g_skinny_linear   -1: no skinny rows kernel for M <= 16 -- tests/test_gpu_rl.py, tests/test_gpu_unet.py
 *   24  g_skinny_gather   -1: no skinny gather kernel, > 0: its pixel limit -- tests/test_gpu_unet.py, tests/test_cabi.py
 *   25  g_wgrad_small_m   -1: weight gradients of layers with at most 1024 rows keep the 128-wide blocks (0: 64-wide, twice as many)
 *                         -- tests/grad_routes.py
 *   27  g_dma             the LDS-DMA engine for split32 operands (csrc/conv_dma.hip): -1 off, 2 = below the tile-count threshold
 *                         too -- tests/test_gpu_unet.py, tests/test_gpu_patch.py
 *   28  g_dma_shape       32: 32x32x16 instead of 16x16x32 MFMA fragments in that engine -- tests/test_gpu_unet.py
 *   30  g_quad            the four-phase transposed-conv kernel (csrc/convt_quad.hip): -1 off, 1 = wherever its shape conditions
 *                         hold -- tests/test_gpu_unet.py
 *   35  g_strip           -1: the whole-network runner does not take the strip-walker kernels (csrc/conv_strip.hip)
 *                         -- tests/test_gpu_strip.py, tests/test_gpu_unet.py
 *   36  g_patch           the shared-patch LDS-DMA engine (csrc/conv_patch.hip): -1 off, 2 = below the tile-count threshold too,
 *                         3 = as 2 with the whole-image patch wherever it fits (4..7: stamp variants of the M2H_CLOCK_DIAG build)
 *                         -- tests/test_gpu_patch.py, __graft_entry__.smoke()
 *   37  g_bn_small        train-mode BatchNorm (csrc/bn.hip): -1 always the three-launch path, 0: layers of at most 256 rows take
 *                         one launch per direction, > 0: layers of at most that many rows (up to 4 096) -- tests/test_gpu_passive_train.py
 *   39  g_strip_rev       walking direction of the strip kernels' images (bit 0: the masked first stage downwards, bit 1: the last
 *                         stage upwards, bit 2: the unmasked first stage downwards; same values either way) -- tests/test_gpu_unet.py
 *   40  g_patch_skip      -1: the shared-patch engine's whole-image 256 x 128 tile keeps the MFMAs of pixel fragments that are
 *                         all top / bottom padding (0: pixel grids 2 x 16, 4 x 16, 2 x 32 skip them; the same bits either way)
 *                         -- tests/test_gpu_patch_padding.py
 *   41  (unassigned: read by nothing)
 *   42  g_splitk_rows     -1: every split-K reduce launch takes the one-item-per-thread kernel with the run-time slab loop (0: the
 *                         row-owning kernel with all S slab loads of an item in flight and 8 channels per thread; same bits)
 *                         -- tests/test_gpu_splitk_reduce.py
 *   43  g_dma_slab_wt     -1: the LDS-DMA engine's split-K slab stores stay plain (0: write-through, `sc1`; same bits)
 *                         -- tests/test_gpu_splitk_reduce.py
 * Retired -- experiments that were measured (results in DESIGN.md) and removed; m2h_tuning_set accepts and stores these numbers, and
 * nothing reads them: 1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 15, 16, 17, 19, 20, 26, 29, 31, 32, 33, 34, 38 (and value 8 of knob 36). */
#ifndef M2H_TUNING_H
#define M2H_TUNING_H
#ifdef __cplusplus
extern "C" {
#endif
#define M2H_TUNING_KNOBS 44
int m2h_tuning_set(int knob, int value);
int m2h_tuning_snapshot(int* out, int n /* == M2H_TUNING_KNOBS */);
int m2h_tuning_restore(const int* in, int n /* == M2H_TUNING_KNOBS */);
#ifdef __cplusplus
}
#endif
#endif
