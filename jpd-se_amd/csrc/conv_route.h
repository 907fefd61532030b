// Which kernel a layer runs on, stated once per direction: select_fwd / select_dgrad / select_wgrad are pure host functions of
// the descriptor, its plan and what the caller asked for; they return a named route.  The launches (conv_dispatch_*.h), the
// moment / norm-sum slot queries and the weight-gradient slab query all read that one choice, so a query cannot answer for
// another kernel than the one that runs.  Every predicate of the choice and every JPDSE_SWITCH it reads lives here; the order of
// the enumerators is the order of the cascades.  Host code only: no kernel, no launch.  Part of conv_gemm.hip (one translation unit).
#pragma once

namespace jpdse {

enum class FwdRoute { thin_in_rows, thin_rows, thin_fwd, head_rows, head_fwd, tapsum, rows, taps4, taps9, halo, fast, toeplitz, generic };
// (DgradRoute::head: the 3 <- 64 data gradient of VGG conv1_1; its launcher takes head_rows_kernel where head_rows_ok holds, else head_fwd_kernel)
enum class DgradRoute { rows, halo, taps9, ring_taps9_frame, ring_halo_frame, ring_taps9_strips, ring_halo_strips, head, dgrad2_rows,
                        thin_dgrad2_rows, thin_in_rows, taps_dgrad2, taps4, thin1, fast, generic };
enum class WgradRoute { thin1, tap_expanded, taps, nine, head, thin, fast, generic };

static const char* const kFwdRouteNames[] = {"thin_in_rows", "thin_rows", "thin_fwd", "head_rows", "head_fwd", "tapsum", "rows",
                                             "taps4", "taps9", "halo", "fast", "toeplitz", "generic"};
static const char* const kDgradRouteNames[] = {"rows", "halo", "taps9", "ring_taps9_frame", "ring_halo_frame", "ring_taps9_strips",
                                               "ring_halo_strips", "head", "dgrad2_rows", "thin_dgrad2_rows", "thin_in_rows",
                                               "taps_dgrad2", "taps4", "thin1", "fast", "generic"};
static const char* const kWgradRouteNames[] = {"thin1", "tap_expanded", "taps", "nine", "head", "thin", "fast", "generic"};
static_assert(sizeof(kFwdRouteNames) / sizeof(char*) == (size_t)FwdRoute::generic + 1 &&
              sizeof(kDgradRouteNames) / sizeof(char*) == (size_t)DgradRoute::generic + 1 &&
              sizeof(kWgradRouteNames) / sizeof(char*) == (size_t)WgradRoute::generic + 1, "one name per route");
static const char* route_name(FwdRoute r) { return kFwdRouteNames[(int)r]; }
static const char* route_name(DgradRoute r) { return kDgradRouteNames[(int)r]; }
static const char* route_name(WgradRoute r) { return kWgradRouteNames[(int)r]; }

// ---- the developer switches the choice reads (jpdse_debug_set_fast_path; compile-time constants in the shipped library)
JPDSE_SWITCH(bool, g_fast_enabled, true);   // jpdse_debug_set_fast_path(0) forces the generic kernels (A/B tests)
JPDSE_SWITCH(int, g_toep_enabled, 1);       // 5: fast kernels, plain head forward
JPDSE_SWITCH(int, g_halo_enabled, 1);
JPDSE_SWITCH(int, g_halo_single, 1);
JPDSE_SWITCH(int, g_rows_enabled, 1);       // 29: the 64-channel 3x3 layers (conv_rows.h) on the halo / fast kernels (A/B)
JPDSE_SWITCH(int, g_head_rows32, 1);        // 57: the 32-channel head on head_fwd_kernel, as before round 4 (A/B)
JPDSE_SWITCH(int, g_thin_fwd_enabled, 1);
JPDSE_SWITCH(int, g_head_fwd_enabled, 1);
JPDSE_SWITCH(int, g_tapsum_enabled, 1);
JPDSE_SWITCH(int, g_taps_enabled, 1);       // 35: stride-2 data gradients on the merged-phase fast kernel (A/B)
JPDSE_SWITCH(int, g_taps4_enabled, 1);      // 36: the 4x4 stride-1 layers on the fast kernel alone (A/B)
JPDSE_SWITCH(int, g_taps9_enabled, 1);      // 38: the 3x3 layers on 8 x 32 grids on the split-K fast kernel (A/B)
JPDSE_SWITCH(int, g_ring_enabled, 1);
JPDSE_SWITCH(int, g_ring_virt, 1);          // 40: ring strips as four split-K GEMMs + ring_fold_kernel (the round-1..3 form) instead of the folded frame
JPDSE_SWITCH(int, g_merge_min_kt, 4);
JPDSE_SWITCH(int, g_merge_min_tiles, 64);   // merged stride-phase data gradient on the fast kernel from this many 256-row tiles on (26: 384 as in round 1, A/B)
JPDSE_SWITCH(int, g_thin1_enabled, 1);      // 41: the one-output-channel layers on the GEMM paths (A/B)
JPDSE_SWITCH(int, g_wgrad_taps_enabled, 1);
JPDSE_SWITCH(int, g_wgrad_nine_enabled, 1);
JPDSE_SWITCH(int, g_wgrad_nine32_enabled, 1);    // 55: 32-pixel-wide images on the per-tap kernel, as before round 4 (A/B)

// ---- the layer as the single-launch bf16 kernels see it: a conv over an N x IH x IW x Cin_s tensor into OH x OW x Ks_out -- the
// forward of a layer, or one stride phase of its data gradient (a stride-1 conv over dy).  The shape predicates below read it;
// ConvView (conv_launch.h) extends it with the pointers and the addressing.
struct ConvShape {
  int N, IH, IW, Cin_s, OH, OW;
  int R, S, stride, reflect;      // reflect: mirrored instead of zero padding
  int act, Ks_out;
  int tap_r;                      // panel offset per filter-row step (== S * Cin_s: no K padding inside the panel's rows)
};
static ConvShape shape_fwd(const jpdse_conv_desc* d, const ConvPlan& p) {
  return {d->N, d->H, d->W, p.Cs, p.OH, p.OW, d->R, d->S, d->stride, d->pad_mode == JPDSE_PAD_REFLECT, d->act, p.Ks, p.Lk_fwd};
}
// stride phase `i` of the data gradient: Uh x Uw taps over dy
static ConvShape shape_dgrad_phase(const jpdse_conv_desc* d, const ConvPlan& p, int i) {
  const Phase& f = p.ph[i];
  return {d->N, p.OH, p.OW, p.Ks, f.cnth, f.cntw, f.Uh, f.Uw, 1, 0, JPDSE_ACT_NONE, p.Cs, f.Lk};
}

// 3x3 convs over 64-channel inputs (stride 1 | 2, zero padding): filter in registers, input rows streamed once (conv_rows.h)
static bool rows_ok(const ConvShape& v) {
  return g_fast_enabled && g_rows_enabled && v.R == 3 && v.S == 3 && (v.stride == 1 || v.stride == 2) && !v.reflect && v.Cin_s == 64 &&
         v.Ks_out % 64 == 0 && v.OW % 64 == 0 && v.OH % 4 == 0 &&
         (v.act == JPDSE_ACT_NONE || v.act == JPDSE_ACT_RELU || v.act == JPDSE_ACT_LRELU);
}
// 3x3 stride-1 convs whose output grid tiles into 4 x 64 patches (ResnetBlocks, VGG19, and the data
// gradient of the zero-padded ones): LDS-resident input halo, see gemm_halo.h
static bool halo_ok(int R, int S, int stride, int OH, int OW, int Cs_in, int Ks_out) {
  return g_fast_enabled && g_halo_enabled && R == 3 && S == 3 && stride == 1 && OH % 4 == 0 && OW % 64 == 0 &&
         Cs_in % 64 == 0 && Ks_out > 32;
}
static bool halo_ok(const ConvShape& v) { return halo_ok(v.R, v.S, v.stride, v.OH, v.OW, v.Cin_s, v.Ks_out); }
// 4x4 stride-1 zero-padded convs and their (single-phase) data gradient on the tap-program kernel (launch_taps4)
static bool taps4_shape_ok(const ConvShape& v) {
  return v.tap_r == v.S * v.Cin_s && g_fast_enabled && g_taps4_enabled && v.R == 4 && v.S == 4 && v.stride == 1 && v.OH >= 8 && v.OW >= 32 &&
         v.Cin_s % 64 == 0 && v.Cin_s >= 128 && v.Ks_out % 64 == 0 && v.Ks_out >= 64 && (long long)v.N * v.IH * v.IW * v.Cin_s < (1LL << 31) &&
         (long long)v.Ks_out * 16 * v.Cin_s < (1LL << 31);
}
// 3x3 stride-1 convs whose grid tiles into 8 x 32 patches but not into the halo kernel's 4 x 64 (launch_taps9)
static bool taps9_shape_ok(int R, int S, int stride, int OH, int OW, int Cin_s, int Ks_out, long long x_elems, long long b_elems) {
  return g_fast_enabled && g_taps9_enabled && R == 3 && S == 3 && stride == 1 && OH % 8 == 0 && OW % 32 == 0 && OW % 64 != 0 &&
         Cin_s % 64 == 0 && Cin_s >= 128 && Ks_out % 64 == 0 && x_elems < (1LL << 31) && b_elems < (1LL << 31);
}
static bool taps9_shape_ok(const ConvShape& v) {
  return v.tap_r == v.S * v.Cin_s && taps9_shape_ok(v.R, v.S, v.stride, v.OH, v.OW, v.Cin_s, v.Ks_out, (long long)v.N * v.IH * v.IW * v.Cin_s,
                                                    (long long)v.Ks_out * 9 * v.Cin_s);
}

// dense 8-channel inputs, 3x3 zero pad, 64 outputs (VGG conv1_1) on the row-streaming pass of thin_in_rows.h
static bool thin_in_rows_fwd_ok(const jpdse_conv_desc* d, const ConvPlan& p) {
  return g_fast_enabled && g_rows_enabled && p.Cs == 8 && d->R == 3 && d->S == 3 && d->stride == 1 && d->pad == 1 &&
         d->pad_mode == JPDSE_PAD_ZERO && p.Ks == 64 && d->K == 64 && p.Lk_fwd == 32 &&
         (d->act == JPDSE_ACT_NONE || d->act == JPDSE_ACT_RELU || d->act == JPDSE_ACT_LRELU);
}
// geometry of the thin forward kernel for a layer: TH output rows per block (8, or 4 for stride 2 / when LDS is short)
struct ThinFwdGeom { int TH, TW, strip_units, w_units, lds; };
static bool thin_fwd_geom(const jpdse_conv_desc* d, const ConvPlan& p, ThinFwdGeom* g) {
  if (!(g_fast_enabled && g_thin_fwd_enabled && p.thinf)) return false;
  const int st = d->stride;
  g->w_units = (p.Ks * p.KP_thin * 2 + 1023) / 1024;
  static const int cand[3][2] = {{8, 64}, {4, 64}, {4, 32}};
  // 8-channel inputs (VGG conv1_1) are output-write bound: the smaller block keeps the epilogue tile at 48 KiB so that
  // three blocks share a CU
  for (int c = (p.Cs <= 8 && p.Ks == 64) ? 1 : 0; c < 3; ++c) {
    const int TH = cand[c][0], TW = cand[c][1];
    if (TH == 4 && p.Ks != 64) break;                 // 4 rows x 2 column groups needs K = 64 (32 per group)
    g->strip_units = (((TW - 1) * st + d->S) * p.Cs * 2 + 16 + 1023) / 1024;
    const int lds = (((TH - 1) * st + d->R) * g->strip_units + 2 * g->w_units) * 1024;
    const int epi = TH * TW * (p.Ks * 2 + 64);
    g->TH = TH;
    g->TW = TW;
    g->lds = lds > epi ? lds : epi;
    if (g->lds <= 160 * 1024) return true;
  }
  return false;
}
// among the thin-input layers, PatchGAN layer 0 (40-channel input, 4x4 stride 2, 64 outputs) as a row-streaming pass (thin_rows.h)
static bool thin_rows_ok(const jpdse_conv_desc* d, const ConvPlan& p) {
  return g_rows_enabled && d->stride == 2 && d->R == 4 && d->S == 4 && p.Cs == 40 && p.Ks == 64 && d->K == 64 &&
         d->pad_mode != JPDSE_PAD_REFLECT && p.KP_thin == 168 &&
         (d->act == JPDSE_ACT_NONE || d->act == JPDSE_ACT_RELU || d->act == JPDSE_ACT_LRELU);
}
static bool head_fwd_ok(const jpdse_conv_desc* d, const ConvPlan& p) {
  const int ncols = d->K * d->R * d->S;
  return g_fast_enabled && g_head_fwd_enabled && p.ES == 2 && d->stride == 1 && d->K <= 3 && p.Ks == 8 &&
         (p.Cs == 64 || p.Cs == 32) && d->R == 7 && d->S == 7 && ncols <= 160 && p.Lk_fwd == d->S * p.Cs;
}
// 64 -> <= 3 channel heads (7x7 reflect + Tanh; 3x3 zero-pad data gradient of VGG conv1_1) as a row-streaming pass (head_rows.h):
// a head conv of `cin` storage channels, K outputs stored as Ks_out, over H x W into OH x OW
static bool head_rows_ok(int cin, int R, int K, int Ks_out, int H, int W, int OH, int OW) {
  return g_rows_enabled && (cin == 64 || (cin == 32 && g_head_rows32 && R == 7)) && K <= 3 && Ks_out == 8 && OW % 128 == 0 &&
         OH % 8 == 0 && OH == H && OW == W;
}
// Convs with K*R*S <= 32 outputs-times-taps (the 512 -> 1 PatchGAN map) as a 1x1 GEMM over the input pixels + tapsum_kernel
static bool tapsum_ok(const jpdse_conv_desc* d, const ConvPlan& p) {
  return g_fast_enabled && g_tapsum_enabled && p.ES == 2 && d->stride == 1 && d->K * d->R * d->S <= 32 &&
         p.Cs % 64 == 0 && p.Cs >= 256 && p.Lk_fwd == d->S * p.Cs;
}

static bool prefer_320(int M, int Ks) {
  // one round of 320-row tiles beats two rounds of 256-row tiles (e.g. the ResnetBlock data gradient
  // on the reflect-padded domain: M = 8976 -> 232 tiles instead of 288 on 256 CUs)
  if (Ks <= 64) return false;
  const long long nt = (Ks + 127) / 128;
  const long long t256 = (long long)((M + 255) / 256) * nt, t320 = (long long)((M + 319) / 320) * nt;
  const long long c256 = ((t256 + 255) / 256) * 256, c320 = ((t320 + 255) / 256) * 320;
  return c320 < c256;
}
// The fast kernel runs ONE 256-row tile per CU (144 KiB of LDS), so its grid should either cover
// the 256 CUs many times over or be an exact multiple of them; in between (e.g. the 288 tiles of the
// ResnetBlock data gradient) the generic 128x128 kernel with 3 co-resident blocks per CU wins
// (measured: scripts/bench_conv.py, profiles/r01_conv_layers_*.log).
static bool fast_pays(int M, int Ks, int k_tiles) {
  if (!g_fast_enabled) return false;
  if (k_tiles < 8) return false;   // short reductions (stride-2 sub-pixel phases of 2x2 taps x 64 ch) do not fill the 3-stage ring
  if (Ks <= 32) {
    // measured: the generic 256x32 kernel beats the 8-wave 256x32 fast config on short reductions; with a long
    // one (512 -> 1 PatchGAN map, K = 8192) the fast kernel needs no padded copy and streams the input by DMA
    if (!(g_thin_out_fast && k_tiles >= 64)) return false;
    return splitk_for(M, Ks, k_tiles) > 1 || (M + 255) / 256 >= 128;
  }
  if (splitk_for(M, Ks, k_tiles) > 1) return true;
  const int bn = Ks > 64 ? 128 : (Ks > 32 ? 64 : 32);
  const long long tiles = (long long)((M + 255) / 256) * ((Ks + bn - 1) / bn);
  if (prefer_320(M, Ks)) {
    const long long t320 = (long long)((M + 319) / 320) * ((Ks + 127) / 128);
    if (t320 % 256 == 0 || t320 % 256 >= 192 || t320 >= 448) return true;   // well-filled rounds
  }
  return tiles >= 448 || (tiles >= 256 && tiles % 256 == 0);
}

struct FwdWants { bool mom, pool; };   // InstanceNorm moments of y from the epilogue; MaxPool2d(2, 2) of y as well (no route depends on it: halo fuses it)
static FwdRoute select_fwd(const jpdse_conv_desc* d, const ConvPlan& p, FwdWants w) {
  if (d->dtype == JPDSE_BF16) {
    if (thin_in_rows_fwd_ok(d, p)) return FwdRoute::thin_in_rows;
    ThinFwdGeom tg;
    if (thin_fwd_geom(d, p, &tg)) return thin_rows_ok(d, p) ? FwdRoute::thin_rows : FwdRoute::thin_fwd;
    if (head_fwd_ok(d, p)) return head_rows_ok(p.Cs, d->R, d->K, p.Ks, d->H, d->W, p.OH, p.OW) ? FwdRoute::head_rows : FwdRoute::head_fwd;
    if (tapsum_ok(d, p)) return FwdRoute::tapsum;
    const ConvShape v = shape_fwd(d, p);
    if (rows_ok(v)) return FwdRoute::rows;
    if (!v.reflect && !w.mom && taps4_shape_ok(v)) return FwdRoute::taps4;
    if (!w.mom && taps9_shape_ok(v)) return FwdRoute::taps9;
    if (halo_ok(v)) return FwdRoute::halo;
    if (p.Cs % 64 == 0 && fast_pays(d->N * p.OH * p.OW, p.Ks, d->R * d->S * p.Cs / 64)) return FwdRoute::fast;
  }
  // staged through the workspace; heads: 4 output pixels x 8 channels per 32-wide GEMM row (pack_fwd_toep_kernel)
  return p.toep && g_fast_enabled && g_toep_enabled && p.OW % 4 == 0 ? FwdRoute::toeplitz : FwdRoute::generic;
}

// ---- tap-program halo kernel (gemm_taps.h): all four sub-pixel phases of a stride-2 data gradient / ConvTranspose forward.
// 3x3 (pad 1, even input): phases (0,0) 2x2 taps, (0,1) 2x1, (1,0) 1x2, (1,1) 1x1 over the same dy pixels; every phase covers
// the same core_h x core_w sub-pixels, a multiple of the kernel's 4 x 64 patch.
// (The 4x4 pad-2 layers of the PatchGAN on this kernel plus a fringe on the fast kernel, developer modes 42 / 43, lost to the
// merged-phase fast kernel inside the step and were retired: profiles/r03_taps_dgrad4_ab.txt)
struct TapsDgrad2Geom { int core_h, core_w; };
static bool taps_dgrad2_geom(const jpdse_conv_desc* d, const ConvPlan& p, bool mom, TapsDgrad2Geom* g) {
  if (!(g_fast_enabled && g_taps_enabled) || d->dtype != JPDSE_BF16 || d->pad_mode == JPDSE_PAD_REFLECT) return false;
  if (d->stride != 2 || d->R != 3 || d->S != 3 || d->pad != 1 || p.nph != 4) return false;
  if (mom) return false;
  if (p.Ks % 64 != 0 || p.Ks < 128 || p.Cs % 64 != 0) return false;
  // the kernel's loaders carry 32-bit element offsets into dy and into each phase's panel
  if ((long long)d->N * p.OH * p.OW * p.Ks >= (1LL << 31) || (long long)p.Cs * 4 * p.Ks >= (1LL << 31)) return false;
  const int core_h = p.ph[0].cnth, core_w = p.ph[0].cntw;
  if (core_h < 4 || core_h % 4 != 0 || core_w < 64 || core_w % 64 != 0) return false;
  for (int i = 0; i < 4; ++i) {
    const Phase& f = p.ph[i];
    if (f.Lk != f.Uw * p.Ks) return false;
    if (f.Uh != (f.qh == 0 ? 2 : 1) || f.Uw != (f.qw == 0 ? 2 : 1)) return false;
    if ((f.Uh - 1) - f.i0h != 0 || (f.Uw - 1) - f.i0w != 0) return false;      // every phase starts at dy pixel (oh, ow)
    if (f.cnth != core_h || f.cntw != core_w) return false;                    // the generator's layers have even inputs: no fringe
  }
  if (g != nullptr) *g = {core_h, core_w};
  return true;
}
static bool taps_dgrad2_ok(const jpdse_conv_desc* d, const ConvPlan& p, bool mom) { return taps_dgrad2_geom(d, p, mom, nullptr); }

// one output channel (PatchGAN 512 -> 1) on the FMA kernels of thin_out1.h (data gradient, weight gradient)
static bool thin1_shape_ok(const jpdse_conv_desc* d, int Cs, int Ks) {
  const int cv = Cs >> 3;
  return g_fast_enabled && g_thin1_enabled && d->dtype == JPDSE_BF16 && d->K == 1 && Ks == 8 && d->stride == 1 &&
         d->pad_mode != JPDSE_PAD_REFLECT && d->R == 4 && d->S == 4 && d->pad <= 3 && Cs % 128 == 0 && d->C == Cs &&
         cv <= 256 && (cv & (cv - 1)) == 0;
}

static int live_phases(const ConvPlan& p) {
  int n = 0;
  for (int i = 0; i < p.nph; ++i) n += p.ph[i].cnth > 0 && p.ph[i].cntw > 0;
  return n;
}
// all stride phases of a data gradient go into ONE launch of the fast kernel: judge the merged grid
static bool dgrad_fast_pays(const jpdse_conv_desc* d, const ConvPlan& p) {
  if (p.Ks % 64 != 0) return false;
  long long tiles = 0;
  int kt_max = 0, m_single = 0;
  const int bn = p.Cs > 64 ? 128 : (p.Cs > 32 ? 64 : 32);
  for (int i = 0; i < p.nph; ++i) {
    if (p.ph[i].cnth <= 0 || p.ph[i].cntw <= 0) continue;
    const int Mi = d->N * p.ph[i].cnth * p.ph[i].cntw;
    tiles += (long long)((Mi + 255) / 256) * ((p.Cs + bn - 1) / bn);
    const int kt = p.ph[i].Uh * p.ph[i].Uw * p.Ks / 64;
    kt_max = kt > kt_max ? kt : kt_max;
    m_single = Mi;
  }
  if (live_phases(p) == 1) return fast_pays(m_single, p.Cs, kt_max);
  return g_fast_enabled && p.Cs > 32 && kt_max >= g_merge_min_kt && tiles >= g_merge_min_tiles;   // few tiles / short K loops: generic wins
}

// mask: dx is masked by the sign of a tensor; lrelu: with a non-zero slope (only the fast / generic tile kernels and the unfused pass
// apply it); addend; mom: moments of dx (ConvTranspose -> InstanceNorm); nsum: the caller passes a norm sink, which only the
// folded-frame halo route serves (conv_dgrad_t refuses the others: the choice itself does not read it)
struct DgradWants { bool mask, addend, lrelu, mom, nsum; };
static DgradRoute select_dgrad(const jpdse_conv_desc* d, const ConvPlan& p, DgradWants w) {
  if (d->dtype != JPDSE_BF16) return DgradRoute::generic;
  const bool refl = d->pad_mode == JPDSE_PAD_REFLECT, bare = !w.mask && !w.addend;
  const int st = d->stride;
  const Phase& f = p.ph[0];
  // phase 0 as the single-launch kernels see it; `whole`: it is the whole data gradient, written straight into dx (zero padding, stride 1)
  const ConvShape v = shape_dgrad_phase(d, p, 0);
  const bool whole = !w.lrelu && !refl && p.nph == 1 && v.OH == d->H && v.OW == d->W;
  if (whole && st == 1 && rows_ok(v) && f.Lk == 3 * p.Ks) return DgradRoute::rows;
  if (whole && halo_ok(v)) return DgradRoute::halo;
  // the same for grids of 8 x 32 patches (W = 32): tap-program kernel, nine taps, split-K over the dy channel slabs
  if (whole && st == 1 && taps9_shape_ok(v)) return DgradRoute::taps9;
  // reflect-padded 3x3: the zero-padded data gradient on the image's own grid (pad 1, straight into dx: halo kernel, or the nine-tap
  // program on 8 x 32 patches) + the ring, which rides in a folded frame of dy (one launch) or runs as four strip GEMMs + a fold
  const bool ring_halo = halo_ok(3, 3, 1, d->H, d->W, p.Ks, p.Cs);
  const bool ring_taps = !ring_halo && taps9_shape_ok(3, 3, 1, d->H, d->W, p.Ks, p.Cs, (long long)d->N * d->H * d->W * p.Ks,
                                                      (long long)p.Cs * 9 * p.Ks);
  if (!w.lrelu && refl && g_ring_enabled && d->R == 3 && d->S == 3 && st == 1 && d->pad == 1 && d->H >= 8 &&
      (ring_halo || ring_taps) && f.Lk == 3 * p.Ks) {
    if (ring_taps) return g_ring_virt && d->H >= 16 ? DgradRoute::ring_taps9_frame : DgradRoute::ring_taps9_strips;
    return g_ring_virt && (p.Ks >= 128 || (p.Ks == 64 && g_halo_single)) ? DgradRoute::ring_halo_frame : DgradRoute::ring_halo_strips;
  }
  // few INPUT channels (VGG conv1_1: 3 <- 64): the data gradient is itself a conv with <= 3 output channels; the
  // single-phase dgrad panel [c][u'][w'][k] is exactly the "plain forward panel" head_fwd_kernel expects
  if (g_fast_enabled && g_head_fwd_enabled && !refl && st == 1 && d->R == 3 && d->S == 3 && d->pad == 1 && d->C <= 3 &&
      p.Cs == 8 && p.Ks == 64 && p.nph == 1 && f.Lk == 3 * p.Ks && bare) return DgradRoute::head;
  // data gradient of the 64 -> 128 3x3 stride-2 conv / forward of the 128 -> 64 ConvTranspose2d at full resolution (dgrad2_rows.h)
  if (g_fast_enabled && g_rows_enabled && !refl && st == 2 && d->R == 3 && d->S == 3 && d->pad == 1 && p.Ks == 128 && p.Cs == 64 &&
      d->C == 64 && d->H == 2 * p.OH && d->W == 2 * p.OW && p.OW % 64 == 0 && p.OH % 4 == 0 && p.nph == 4 && bare) return DgradRoute::dgrad2_rows;
  // data gradient of PatchGAN layer 0 with respect to the image channels (thin_dgrad2_rows.h)
  if (g_fast_enabled && g_rows_enabled && !refl && st == 2 && d->R == 4 && d->S == 4 && d->pad == 2 && p.Cs == 8 && d->C <= 3 &&
      p.Ks == 64 && d->H % 8 == 0 && d->W % 256 == 0 && p.OH == d->H / 2 + 1 && p.OW == d->W / 2 + 1 && p.nph == 4 &&
      f.Lk == 128 && bare) return DgradRoute::thin_dgrad2_rows;
  // data gradient of the 64 -> 3 7x7 reflect-padded head (thin_in_rows.h: padded-domain conv + ring fold)
  if (g_fast_enabled && g_rows_enabled && refl && st == 1 && d->R == 7 && d->S == 7 && d->pad == 3 && p.Ks == 8 && p.Cs == 64 &&
      d->C == 64 && d->H >= 8 && d->W >= 8 && p.nph == 1 && f.Lk == 64 && bare) return DgradRoute::thin_in_rows;
  if (taps_dgrad2_ok(d, p, w.mom)) return DgradRoute::taps_dgrad2;
  if (whole && st == 1 && !w.mom && taps4_shape_ok(v)) return DgradRoute::taps4;
  if (thin1_shape_ok(d, p.Cs, p.Ks) && p.nph == 1 && !w.mask && !w.mom && f.Uh == 4 && f.Uw == 4 && f.cnth == d->H && f.cntw == d->W)
    return DgradRoute::thin1;
  return dgrad_fast_pays(d, p) ? DgradRoute::fast : DgradRoute::generic;
}

// ---- weight gradient
static bool wgrad_thin_ok(const jpdse_conv_desc* d, const ConvPlan& p) {
  const int n_tiles = (d->S * p.Cs + 31) / 32;
  return g_fast_enabled && p.Cs % 64 != 0 && (p.Ks == 32 || p.Ks == 64) && n_tiles <= 12 &&
         (126 * d->stride * p.Cs + 64 * 12) <= 20 * 1024;
}
// all-taps weight gradient of the narrow high-resolution layers (wgrad_taps.h)
// config id: 0 none; 1: 3x3 s2 K%128 C%64; 2: 3x3 s1 K%64 C%64; 3: 4x4 s2 K%128 C%64; 4: 3x3 s2 K%256 C%128
static int wgrad_taps_cfg(const jpdse_conv_desc* d, const ConvPlan& p) {
  if (!g_fast_enabled || !g_wgrad_taps_enabled || p.ES != 2 || d->R != d->S) return 0;
  if ((long long)d->N * p.OH * ((p.OW + 63) / 64) < 32) return 0;
  if ((long long)d->N * p.OH * p.OW * p.Ks >= (1LL << 31) || (long long)d->N * d->H * d->W * p.Cs >= (1LL << 31)) return 0;
  // 3x3 stride 2 with wide outputs, any width: the down-sampling convs 128 -> 256 ... 512 -> 1024 and, with the roles of
  // x and dy swapped by the caller, the ConvTranspose2d layers 1024 -> 512 ... 128 -> 64 (round 1 sent the wide ones to
  // the per-tap kernel, whose stream-K partial tiles met in fp32 atomics)
  if (d->R == 3 && d->stride == 2 && p.Ks % 256 == 0 && p.Cs % 64 == 0) return 4;      // (round 3: the all-nine-taps config 1 on these wide layers measured -3 ... -11 %, +5 % only at 512 -> 1024)
  if (p.Ks > 256 || p.Cs > 128) return 0;
  if (d->R == 3 && d->stride == 2 && p.Ks % 128 == 0 && p.Cs % 64 == 0) return 1;
  if (d->R == 3 && d->stride == 1 && p.Ks % 64 == 0 && p.Ks <= 128 && p.Cs % 64 == 0) return 2;
  if (d->R == 4 && d->stride == 2 && p.Ks % 128 == 0 && p.Cs % 64 == 0) return 3;
  return 0;
}
// images 32 pixels wide (the LocalEnhancer's 1024-channel trunk at 16 x 32): the row-pair form of the kernel (wgrad_nine.h, W32)
static bool wgrad_nine32_shape(const jpdse_conv_desc* d, const ConvPlan& p) {
  return g_wgrad_nine32_enabled && d->W == 32 && p.OW == 32 && d->H % 2 == 0 && d->H >= 4 && d->pad_mode == JPDSE_PAD_REFLECT &&
         p.Ks >= 256 && p.Cs >= 256;         // wide layers only: 64 k x 64 c tiles must fill the chip
}
// all-nine-taps weight gradient of the wide 3x3 stride-1 layers (wgrad_nine.h): no atomics, no partial tiles
static bool wgrad_nine_ok(const jpdse_conv_desc* d, const ConvPlan& p) {
  return g_fast_enabled && g_wgrad_nine_enabled && p.ES == 2 && d->R == 3 && d->S == 3 && d->stride == 1 && d->pad == 1 &&
         (p.OW % 64 == 0 || wgrad_nine32_shape(d, p)) && p.Ks % 64 == 0 && p.Cs % 64 == 0 && d->H >= 2 && d->W >= 8 &&
         (long long)d->N * d->H * d->W * (p.Ks > p.Cs ? p.Ks : p.Cs) < (1LL << 31);
}
// heads with <= 8 output channels on a 32- / 64-channel input, stride 1 (64->3, 32->3 7x7)
static bool wgrad_head_ok(const jpdse_conv_desc* d, const ConvPlan& p) {
  return g_fast_enabled && p.Ks == 8 && d->stride == 1 && (p.Cs == 32 || p.Cs == 64) && d->S * 8 <= 64 && d->R <= 7 &&
         d->R == d->S;
}
// few output channels: dense 1x1 weight gradient over the tap-expanded dy (expand_dy_taps_kernel)
static bool wgrad_tap_expanded_ok(const jpdse_conv_desc* d, const ConvPlan& p) {
  return g_fast_enabled && !wgrad_head_ok(d, p) && p.Ks == 8 && d->stride == 1 && p.Cs % 64 == 0 && round_up(d->K * d->R * d->S, 64) <= 256;
}
// the fast kernel's loader uses 32-bit element offsets
static bool fits32(const jpdse_conv_desc* d, const ConvPlan& p) {
  return (long long)d->N * p.OH * p.OW * p.Ks < (1LL << 31) && (long long)d->N * p.Hp * p.Wp * p.Cs < (1LL << 31);
}
static WgradRoute select_wgrad(const jpdse_conv_desc* d, const ConvPlan& p) {
  if (d->dtype != JPDSE_BF16) return WgradRoute::generic;
  if (thin1_shape_ok(d, p.Cs, p.Ks)) return WgradRoute::thin1;
  if (wgrad_tap_expanded_ok(d, p)) return WgradRoute::tap_expanded;
  if (wgrad_taps_cfg(d, p)) return WgradRoute::taps;
  if (wgrad_nine_ok(d, p) && ((long long)d->K * 9 * d->C) % 4 == 0) return WgradRoute::nine;
  if (wgrad_head_ok(d, p)) return WgradRoute::head;
  if (wgrad_thin_ok(d, p)) return WgradRoute::thin;        // thin inputs (40-channel network inputs)
  return g_fast_enabled && p.Ks % 64 == 0 && fits32(d, p) ? WgradRoute::fast : WgradRoute::generic;
}

}  // namespace jpdse
