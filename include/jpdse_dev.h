/*
 * jpdse_dev.h -- the extra entry points of the developer build libjpdse_hip_dev.so (compiled with -DJPDSE_DEV from
 * the same sources as libjpdse_hip.so).  Not part of the drop-in boundary: the shipped library neither exports this
 * symbols nor contains the run-time switches behind them (they are compile-time constants there).  Used by scripts/ (same-process A/B measurements) and by the tests that compare two kernels of one
 * layer with each other; no reference counterpart.
 */
#ifndef JPDSE_DEV_H_
#define JPDSE_DEV_H_

#include "jpdse.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Developer A/B switch (kernel SELECTION only: results stay correct under every code):
 * 0 = every convolution on the generic register-staged kernels; 1 (default) = all specialised bf16 kernels; 3 = no halo kernel;
 * 4 = no all-nine-taps weight gradient; 5 = heads without the Toeplitz GEMM; 6 = no split-K, no head kernel, no tap programs
 * (same summation order as the generic kernels: bit-comparable); 7 = reflect data gradient on the padded domain;
 * 8 = halo kernel always double buffered; 9 / 10 = long-K-only phase merging / no 128-row tiles; 12 = no all-taps weight gradient;
 * 13 = no tap-sum forward; 14 = no head kernel; 15 / 16 = XCD-aware halo tile orders; 18 = no thin-input forward kernel;
 * 26 = merged stride-phase data gradient only from 384 tiles on; 27 = InstanceNorm
 * always as three kernels; 29 = the 64-channel / thin-input layers on
 * the halo / fast kernels instead of the row-streaming family; 32 = no InstanceNorm moments in conv epilogues; 35 = stride-2 data
 * gradients on the merged-phase fast kernel instead of the tap-program halo kernel (gemm_taps.h); 36 = 4x4 stride-1 layers on the
 * fast kernel alone; 38 = 3x3 layers with 32-pixel-wide grids on the split-K fast kernel instead of the nine-tap program;
 * 40 = reflect data gradient as halo kernel + four ring-strip GEMMs + ring_fold_kernel instead of the folded frame (gemm_halo.h
 * VIRT); 41 = the one-output-channel layers backward on the GEMM paths instead of thin_out1.h;
 * 48 = fp32 generic kernel without split-K; 55 = 32-pixel-wide 1024-channel weight gradients on the per-tap kernel
 * instead of the row-pair nine-tap form; 57 = the 32 -> 3 head forward on head_fwd_kernel instead of head_rows_kernel<7, 32>;
 * 58 = all-taps weight gradient (wgrad_taps.h) with the tiles of a pixel range co-located on one XCD (measured slower);
 * 60 = halo kernel without the XCD-aware tile order on its one-round grids (15 / 16 / 17 force an order on every grid);
 * 59 = the few-tile medium-K layers of the fast kernel on 256-row tiles as before round 4;
 * Any other code that is not retired selects the shipped dispatch, like 1.
 * Retired in round 4 with their negative results on record (profiles/r0*_ab.txt; the code paths are gone):
 * 21 / 22 / 24 (unpipelined loop forms of the nine-tap weight gradient), 23 (halo kernel, staggered DMA issue), 25 (halo kernel,
 * hand-pipelined fragment reads), 30 (fast kernel, XCD-aware tile order), 31 (ring strips on 128-row tiles), 44 / 45 (3- / 4-stage
 * rings for the 128-row short-K configurations), 46 (no 64-row tiles for the short loops).
 * Retired later, once their measurements were settled (the code paths are gone; these codes return JPDSE_EINVAL so that a sweep
 * cannot measure the shipped dispatch under their label): 53 / 56 (halo forward on four / sixteen waves, gemm_halo4.h / gemm_halo16.h:
 * profiles/r04_halo_wavetile_ab.txt), 54 (dgrad2_rows with conflict-free LDS addresses, timing only:
 * profiles/r04_dgrad2_rows_conflicts_ab.txt), 100-199 (100 + bits: timing-only ablations of the halo loop:
 * profiles/r01_ablation_resblock.txt, profiles/r04_virt_conflicts_ab.txt), 201-203 (timing-only ablations of the all-taps
 * weight-gradient loop: profiles/r04_wgrad_taps_ab.txt), 210-225 (timing-only ablations of gemm_fast_kernel's loader, loop and
 * epilogue: profiles/r04_fast_astage_ablation.txt, profiles/r04_epilogue_act_ab.txt).
 * Retired in a second pass, each a complete kernel alternative that had lost its A/B (same rule: JPDSE_EINVAL):
 * 19 (halo kernel on 16x16x32 MFMA fragments, the MF16 form of gemm_halo_kernel: 1020 vs 1032 TFLOP/s),
 * 28 (InstanceNorm as one kernel with an in-launch exchange between workgroups: profiles/r02_norm_forms.txt),
 * 42 / 43 (4x4 stride-2 data gradients off / on the tap program + fringe: profiles/r03_taps_dgrad4_ab.txt),
 * 50 / 51 / 52 / 61 (the persistent form of the fast kernel, gemm_pers.h, and the label of the dispatch without it:
 * profiles/r04_pers_v1_ab.txt, profiles/r04_pers_v2_ab.txt).
 * Each call resets the others to their defaults.
 * The kernel names above are prose; which kernel family a layer runs on under a mode is a ROUTE, and the routes' names come from
 * route_name() in jpd-se_amd/csrc/conv_route.h (jpdse_debug_conv_route / jpdse_debug_route_name below). */
int jpdse_debug_set_fast_path(int32_t enable);

/* The routes (conv_route.h: FwdRoute, DgradRoute, WgradRoute) the forward, data gradient and weight gradient of a layer take under
 * the current switch setting: out[0..2].  Launches nothing.  flags = what the caller would ask for: 1 forward moments, 2 pooled
 * output; data gradient: 4 mask, 8 addend, 16 the mask has a non-zero (LeakyReLU) slope, 32 moments, 64 norm-backward sums.
 * jpdse_debug_route_name(direction 0 | 1 | 2, route) is the route's printable name, NULL when there is no such route. */
int jpdse_debug_conv_route(const jpdse_conv_desc* d, int32_t flags, int32_t out[3]);
const char* jpdse_debug_route_name(int32_t direction, int32_t route);

/* CU occupier for the one-GPU rehearsal of "compute kernels share the chip with a collective" (scripts/cu_contention.py,
 * profiles/r03_cu_contention.txt): launches `blocks` (1..128) workgroups on `stream`, each holding a whole CU's 160 KiB of LDS,
 * that sleep until *release_flag (host-visible memory, e.g. pinned) becomes non-zero or max_ms (<= 20000) of wall clock have
 * passed -- every wave exits by itself, the grid always drains.  No reference counterpart. */
int jpdse_debug_occupy_cus(int32_t blocks, const int32_t* release_flag, int32_t max_ms, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* JPDSE_DEV_H_ */
