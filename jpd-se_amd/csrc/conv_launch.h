// Launchers of the forward / data-gradient kernel families (generic, fast, halo, tap-program, row-streaming, thin, head)
// and the in-library GEMM timer; which layer takes which kernel is conv_route.h's business.  Every launcher re-checks the
// divisibility / extent assumptions of its kernel's grid before it enqueues anything (a wrong launch argument must be an error
// code, not a GPU memory fault: DESIGN.md 9).  Part of conv_gemm.hip (one translation unit).
#pragma once

namespace jpdse {

// ---- in-library kernel timer (bench.py "roofline"): hipEvent pairs around the GEMM launches whose
// (N, K) signature was selected, recorded on the stream the kernel runs on.
struct GemmProf {
  bool on = false;
  int Ks = 0;
  long long kdim = 0;
  int used = 0;
  std::vector<hipEvent_t> ev;   // 2 per launch
  std::vector<double> flops;
  std::vector<int> cls;         // 0: forward / data-gradient GEMM; 1: reflect ring strips + fold; 2: weight gradient
};
static GemmProf g_prof;
// Launch-argument guard shared by the tiled launchers: the kernels assume an exact tile grid and 32-bit in-tensor offsets;
// the dispatch predicates guarantee both, a launcher that is handed anything else refuses before enqueueing.
static int check_tile_grid(const char* who, int N, int OH, int OW, int th, int tw, int Cs_in, long long in_elems, long long out_elems) {
  if (N <= 0 || OH <= 0 || OW <= 0 || OH % th != 0 || OW % tw != 0)
    return set_error(JPDSE_EINVAL, "%s: output grid %d x %d x %d does not tile into %d x %d patches", who, N, OH, OW, th, tw);
  if (Cs_in <= 0 || Cs_in % 64 != 0) return set_error(JPDSE_EINVAL, "%s: %d input channels (a multiple of 64 is required)", who, Cs_in);
  if (in_elems >= (1LL << 31) || out_elems >= (1LL << 40))
    return set_error(JPDSE_EINVAL, "%s: tensor too large for the kernel's offsets (%lld input elements)", who, in_elems);
  return JPDSE_OK;
}

// Opts `Kernel` into `bytes` of dynamic LDS (more than the 64 KiB a launch gets by default), once per kernel instantiation.
template <auto Kernel>
static int opt_in_lds(const char* who, int bytes) {
  static bool configured = false;
  if (configured) return JPDSE_OK;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) return set_error(JPDSE_ELAUNCH, "%s: hipFuncSetAttribute(%d B LDS): %s", who, bytes, hipGetErrorString(e));
  configured = true;
  return JPDSE_OK;
}

// A timed region on stream s (every launcher that times itself brackets its launches with these two): the slot, or -1 when
// the timer is off, full, or (Ks, kdim) is not the GEMM signature that was selected.  prof_end files the region under its class.
static int prof_begin(hipStream_t s, int Ks, long long kdim) {
  if (!g_prof.on || Ks != g_prof.Ks || kdim != g_prof.kdim || (size_t)(2 * g_prof.used + 2) > g_prof.ev.size()) return -1;
  (void)hipEventRecord(g_prof.ev[2 * g_prof.used], s);
  return g_prof.used;
}
static void prof_end(int slot, int cls, double flops, hipStream_t s) {
  if (slot < 0) return;
  (void)hipEventRecord(g_prof.ev[2 * slot + 1], s);
  g_prof.flops[slot] = flops;
  g_prof.cls[slot] = cls;
  g_prof.used = slot + 1;
}

// ---- the layer as the bf16 single-launch kernels see it: a conv over X with panel B into Y (its ConvShape, conv_route.h, plus the
// pointers and the addressing).  Every bf16 path of conv_fwd_t / conv_dgrad_t starts from one of the
// two constructors and hands the view to its kernel family through a converter (to_rows / to_halo / to_fast; the tap-program
// launchers take the view itself): a new fused operand is added here and in the converters, not once per dispatch branch.
struct ConvView : ConvShape {
  const bf16_t* X; const bf16_t* B; const float* bias; bf16_t* Y;
  int py, px, Kout;
  long long ktot;                 // panel row stride (elements)
  int tap_s;                      // panel offset per filter-column step
  long long out_sn, out_sh, out_sw, out_base;
  float slope;
  // optional fused operands, set by the dispatch after construction
  const bf16_t* mask; float mask_slope; const bf16_t* addend;   // data gradient, Y's addressing: Y = (result + addend) * (mask > 0 ? 1 : mask_slope)
  int alias, addend_n;            // batched data gradient (0 = off): images >= alias read the mask of image n - alias; images >= addend_n take no addend
  float* mom;                     // InstanceNorm moments of Y from the epilogue (rows / halo kernels)
  const bf16_t* frame;            // folded frame of X: reflect data gradient in one launch (halo kernel, nine-tap program)
};

static ConvView view_fwd(const jpdse_conv_desc* d, const ConvPlan& p, const void* x, const void* pack, const float* bias, void* y) {
  ConvView v = {};
  static_cast<ConvShape&>(v) = shape_fwd(d, p);
  v.X = reinterpret_cast<const bf16_t*>(x);
  v.B = reinterpret_cast<const bf16_t*>(pack);
  v.bias = bias;
  v.Y = reinterpret_cast<bf16_t*>(y);
  v.py = v.px = d->pad;
  v.Kout = d->K;
  v.ktot = (long long)d->R * p.Lk_fwd; v.tap_s = p.Cs;
  v.out_sn = (long long)p.OH * p.OW * p.Ks; v.out_sh = (long long)p.OW * p.Ks; v.out_sw = p.Ks;
  v.slope = d->slope;
  return v;
}

// stride phase `i` of the data gradient: Uh x Uw taps over dy, written to every stride-th pixel of dx from the phase's first one
static ConvView view_dgrad_phase(const jpdse_conv_desc* d, const ConvPlan& p, int i, const void* dy, const void* pack, void* dx) {
  const Phase& f = p.ph[i];
  const int st = d->stride;
  ConvView v = {};
  static_cast<ConvShape&>(v) = shape_dgrad_phase(d, p, i);
  v.X = reinterpret_cast<const bf16_t*>(dy);
  v.B = reinterpret_cast<const bf16_t*>(reinterpret_cast<const char*>(pack) + f.pack_off);
  v.Y = reinterpret_cast<bf16_t*>(dx);
  v.py = (f.Uh - 1) - f.i0h; v.px = (f.Uw - 1) - f.i0w;
  v.Kout = d->C;
  v.ktot = (long long)f.Uh * f.Lk; v.tap_s = p.Ks;
  v.out_sn = (long long)d->H * d->W * p.Cs; v.out_sh = (long long)st * d->W * p.Cs; v.out_sw = (long long)st * p.Cs;
  v.out_base = ((long long)(st * f.i0h + f.qh - d->pad) * d->W + (st * f.i0w + f.qw - d->pad)) * p.Cs;
  return v;
}

// the fields every argument struct of the tiled kernels shares, under the same names
template <typename Args>
static Args view_to(const ConvView& v) {
  Args a = {};
  a.X = v.X; a.B = v.B; a.bias = v.bias; a.Y = v.Y;
  a.OH = v.OH; a.OW = v.OW; a.IH = v.IH; a.IW = v.IW; a.py = v.py; a.px = v.px;
  a.Kout = v.Kout; a.Ks = v.Ks_out; a.b_rows = v.Ks_out;
  a.out_sn = v.out_sn; a.out_sh = v.out_sh; a.out_sw = v.out_sw; a.out_base = v.out_base;
  a.act = v.act; a.slope = v.slope;
  a.mask = v.mask; a.addend = v.addend;
  return a;
}
static RowsArgs to_rows(const ConvView& v) {        // 64-channel input, 3x3: the stride goes to launch_rows
  RowsArgs r = view_to<RowsArgs>(v);
  r.N = v.N;
  r.mom = v.mom;                                    // (launch_rows_cfg sets the slot count with the band height)
  return r;
}
static int halo_slots(int OH, int OW) { return (OH / 4) * (OW / 64); }      // moment / norm-sum slots per image: one per 4 x 64 output patch
static HaloArgs to_halo(const ConvView& v) {
  HaloArgs h = view_to<HaloArgs>(v);
  h.N = v.N; h.Cs = v.Cin_s; h.reflect = v.reflect;
  h.V = v.frame;
  h.mom = v.mom;
  h.mom_slots = v.mom != nullptr ? halo_slots(v.OH, v.OW) : 0;
  return h;
}
static FastArgs to_fast(const ConvView& v) {        // dense panel (b_stride / b_tap_* = 0); splits and slabs are the caller's
  FastArgs f = view_to<FastArgs>(v);
  f.M = v.N * v.OH * v.OW; f.Cs = v.Cin_s;
  f.R = v.R; f.S = v.S; f.sy = f.sx = v.stride; f.reflect = v.reflect;
  f.mask_slope = v.mask_slope;
  f.alias = v.alias; f.addend_n = v.addend_n;
  return f;
}

template <typename T, int BM, int BN, int WM, int WN>
static int launch_fwd_cfg(const GemmFwdArgs& a_in, hipStream_t s) {
  GemmFwdArgs a = a_in;
  const int tiles_m = (a.M + BM - 1) / BM, tiles_n = (a.Ks + BN - 1) / BN;
  const size_t lds = 2 * (BM + BN) * 64;
  // split-K (fp32, few tiles): only with a slab region big enough behind `partial` (the plan sized it with the same function)
  a.splits = (a.col_mod == 0 && a.partial != nullptr) ? generic_splitk_for((int)sizeof(T), a.M, a.Ks, a.R * a.cpr, a.M / (a.OH * a.OW)) : 1;
  if (a.splits > 1 && (size_t)a.splits * a.M * a.Ks * sizeof(float) > a.partial_cap) a.splits = 1;
  const long long kdim = (long long)a.R * a.cpr * (64 / (int)sizeof(T));
  const int pslot = prof_begin(s, a.Ks, kdim);
  hipLaunchKernelGGL((gemm_fwd_kernel<T, BM, BN, WM, WN>), dim3(tiles_m * tiles_n, a.splits > 1 ? a.splits : 1), dim3(64 * WM * WN), lds, s, a);
  int rc = check_launch("gemm_fwd_kernel");
  if (rc == JPDSE_OK && a.splits > 1) {
    const long long total_vec = (long long)a.M * (a.Ks / 4);
    hipLaunchKernelGGL((gemm_splitk_finish_kernel<T>), dim3((unsigned)((total_vec + 255) / 256)), dim3(256), 0, s, a, total_vec);
    rc = check_launch("gemm_splitk_finish_kernel");
  }
  prof_end(pslot, 0, 2.0 * (double)a.M * (double)a.Ks * (double)kdim, s);
  return rc;
}

template <typename T>
static int launch_fwd(const GemmFwdArgs& a, hipStream_t s) {
  if (a.M <= 0) return JPDSE_OK;
  if (a.Ks > 64) return launch_fwd_cfg<T, 128, 128, 2, 2>(a, s);
  if (a.Ks > 32) return launch_fwd_cfg<T, 128, 64, 2, 2>(a, s);
  return launch_fwd_cfg<T, 256, 32, 4, 1>(a, s);
}

// split count of the generic weight-gradient kernel (shared by the launcher and the workspace query)
template <typename T, int BM, int BN>
static int generic_wgrad_splits(const GemmWgradArgs& a, int* chunks_per_split) {
  const int PIX = WgStage<T>::PIX;
  const int col_tiles = (a.run + BN - 1) / BN, chunks_total = (a.M + PIX - 1) / PIX;
  const int tiles = ((a.K + BM - 1) / BM) * a.R * col_tiles;
  int splits = 1;
  if (tiles < 512) {
    splits = (768 + tiles - 1) / tiles;
    const int max_splits = (chunks_total + 7) / 8;  // >= 8 chunks of work per split
    if (splits > max_splits) splits = max_splits;
    if (splits > 64) splits = 64;
    if (splits < 1) splits = 1;
  }
  const int cps = (chunks_total + splits - 1) / splits;
  if (chunks_per_split) *chunks_per_split = cps;
  return (chunks_total + cps - 1) / cps;
}

template <typename T, int BM, int BN, int WM, int WN>
static int launch_wgrad_cfg(GemmWgradArgs a, float* slabs, hipStream_t s) {
  const int PIX = WgStage<T>::PIX;
  a.col_tiles_per_r = (a.run + BN - 1) / BN;
  a.chunks_total = (a.M + PIX - 1) / PIX;
  const int tiles = ((a.K + BM - 1) / BM) * a.R * a.col_tiles_per_r;
  const int splits = generic_wgrad_splits<T, BM, BN>(a, &a.chunks_per_split);
  const long long n = (long long)a.K * a.R * a.S * a.C;
  a.partial = splits > 1 ? slabs : nullptr;
  a.slab_stride = (n + 3) / 4 * 4;
  const size_t lds = 2 * (BM + BN) * 64;
  hipLaunchKernelGGL((gemm_wgrad_kernel<T, BM, BN, WM, WN>), dim3(tiles, splits), dim3(64 * WM * WN), lds, s, a);
  if (int rc = check_launch("gemm_wgrad_kernel")) return rc;
  return splits > 1 ? launch_slab_reduce(slabs, a.DW, n, a.slab_stride, splits, s) : JPDSE_OK;
}

template <typename T>
static size_t generic_wgrad_slab_bytes(const GemmWgradArgs& a) {
  const int splits = a.K > 64 ? generic_wgrad_splits<T, 128, 128>(a, nullptr)
                              : (a.K > 32 ? generic_wgrad_splits<T, 64, 128>(a, nullptr) : generic_wgrad_splits<T, 32, 256>(a, nullptr));
  const long long n = (long long)a.K * a.R * a.S * a.C;
  return splits > 1 ? (size_t)splits * ((n + 3) / 4 * 4) * sizeof(float) : 0;
}

template <typename T>
static int launch_wgrad(const GemmWgradArgs& a, float* slabs, hipStream_t s) {
  if (a.K > 64) return launch_wgrad_cfg<T, 128, 128, 2, 2>(a, slabs, s);
  if (a.K > 32) return launch_wgrad_cfg<T, 64, 128, 2, 2>(a, slabs, s);
  return launch_wgrad_cfg<T, 32, 256, 1, 4>(a, slabs, s);
}

template <int WM, int WN, int TM, int TN, int STAGES = 3>
static int launch_fast_cfg(FastBatch& b, hipStream_t s) {
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  constexpr int lds = STAGES * (BM + BN) * 128;
  if (int rc = opt_in_lds<&gemm_fast_kernel<WM, WN, TM, TN, STAGES>>("gemm_fast", lds)) return rc;
  int total = 0;
  for (int i = 0; i < b.n; ++i) {
    const FastArgs& a = b.p[i];
    if ((a.Y == nullptr && !a.no_finish) || ((a.splits > 1 || a.no_finish) && a.partial == nullptr))
      return set_error(JPDSE_EINVAL, "gemm_fast: problem %d has no output buffer", i);
    if ((a.x_sh ? a.x_sh : (long long)a.IW * a.Cs) * a.IH >= (1LL << 31))
      return set_error(JPDSE_EINVAL, "gemm_fast: one image spans >= 2^31 elements (in-image offsets are 32-bit)");
    if (a.x_extent > 0 && a.OH > 0 && a.OW > 0) {
      // sub-image problems (the ring strips of the reflect data gradient address rows / columns of a larger tensor through
      // x_sn / x_sh): the last element the loader can touch must lie inside the tensor -- a wrong stride or base here is
      // a GPU memory fault, not a wrong number (the round-1 abort)
      const long long n_img = a.M / ((long long)a.OH * a.OW);
      const long long sn = a.x_sn ? a.x_sn : (long long)a.IH * a.IW * a.Cs, sh = a.x_sh ? a.x_sh : (long long)a.IW * a.Cs;
      const long long last = (n_img - 1) * sn + (long long)(a.IH - 1) * sh + (long long)(a.IW - 1) * a.Cs + a.Cs;
      if (n_img < 1 || last > a.x_extent)
        return set_error(JPDSE_EINVAL, "gemm_fast: problem %d addresses element %lld of a %lld-element input", i, last, a.x_extent);
    }
    b.first_tile[i] = total;
    b.p[i].xcd_map = 0;       // (the XCD-aware tile order, round-3 developer mode 30, measured neutral and was retired: DESIGN.md 4.1 (xi))
    total += ((a.M + BM - 1) / BM) * ((a.Ks + BN - 1) / BN) * (a.splits > 1 ? a.splits : 1);
  }
  for (int i = b.n; i <= kFastBatchMax; ++i) b.first_tile[i] = total;
  const long long kdim = (long long)b.p[0].R * b.p[0].S * b.p[0].Cs;
  const int pslot = b.n == 1 ? prof_begin(s, b.p[0].Ks, kdim) : -1;      // a multi-problem launch is not one GEMM: not timed
  hipLaunchKernelGGL((gemm_fast_kernel<WM, WN, TM, TN, STAGES>), dim3(total), dim3(64 * WM * WN), lds, s, b);
  if (b.n == 1 && b.p[0].splits > 1 && !b.p[0].no_finish) {
    const long long total_vec = (long long)b.p[0].M * (b.p[0].Ks / 8);
    hipLaunchKernelGGL(splitk_finish_kernel, dim3(ew_blocks(total_vec)), dim3(256), 0, s, b.p[0], total_vec);
  }
  prof_end(pslot, 0, 2.0 * (double)b.p[0].M * (double)b.p[0].Ks * (double)kdim, s);
  return check_launch("gemm_fast_kernel");
}

JPDSE_SWITCH(int, g_fast_small, 20);      // K-tile count up to which the 128-row / 2-stage fast configs are used
JPDSE_SWITCH(int, g_fast_fill, 1);                // 59: no small tiles for the few-tile medium-K layers (A/B)
static int launch_fast_batch(FastBatch& b, hipStream_t s) {
  if (b.n <= 0) return JPDSE_OK;
  const int Ks = b.p[0].Ks;
  if (b.n == 1 && b.p[0].splits > 1) {   // split-K
    if (Ks > 64) return launch_fast_cfg<4, 2, 2, 2>(b, s);
    if (Ks > 32) return launch_fast_cfg<4, 2, 2, 1>(b, s);
    return launch_fast_cfg<8, 1, 1, 1>(b, s);
  }
  for (int i = 0; i < b.n; ++i)
    if (b.n > 1 && !b.p[i].no_finish) b.p[i].splits = 1;
  if (b.small_m) {
    if (Ks > 64) return launch_fast_cfg<2, 2, 2, 2, 2>(b, s);
    if (Ks > 32) return launch_fast_cfg<2, 2, 2, 1, 2>(b, s);
  }
  int kt = 0;
  for (int i = 0; i < b.n; ++i) {
    const int k = b.p[i].R * b.p[i].S * (b.p[i].Cs / 64);
    kt = k > kt ? k : kt;
  }
  if (g_fast_small && kt <= g_fast_small && b.p[0].splits <= 1) {
    // short reductions are prologue / epilogue bound: 128-row tiles, 4 waves, 2 stages = 64 (48) KiB of LDS, so two
    // (three) blocks share a CU and overlap each other's fill and store phases
    // (deeper rings for the same tiles -- round-3 developer modes 44 / 45 -- measured 25-50 % slower: profiles/r03_fast_stages_ab.txt)
    // up to 16 K-tiles and wide outputs: 64 x 128 tiles (48 KiB of LDS, three blocks per CU).  Measured per layer in one process
    // (profiles/r03_fast_tile64_ab.txt): PatchGAN layer 1 forward +7 % / +32 % (first / second scale), layer 2 data gradient
    // +10 % / +24 %; longer loops (18-32 tiles) and the 64-wide outputs (64 x 64 tiles) lose 3-6 % and keep the 128-row tiles.
    if (Ks > 64 && kt <= 16) return launch_fast_cfg<2, 2, 1, 2, 2>(b, s);   // 64 x 128
    if (Ks > 64) return launch_fast_cfg<2, 2, 2, 2, 2>(b, s);   // 128 x 128
    if (Ks > 32) return launch_fast_cfg<2, 2, 2, 1, 2>(b, s);   // 128 x 64
  }
  if (g_fast_fill && Ks > 64 && kt <= 64 && b.p[0].splits <= 1) {
    // Few tiles, medium K (round 4): 256-row tiles of a small layer leave most of the chip idle (PatchGAN layer 2 of the second scale:
    // 17,160 pixels x 256 channels = 136 tiles for 256 CUs, 279 TFLOP/s).  Smaller tiles of the same loop (same summation order) fill it.
    long long t256 = 0;
    for (int i = 0; i < b.n; ++i) t256 += (long long)((b.p[i].M + 255) / 256) * ((Ks + 127) / 128);
    if (t256 < 224) {
      if (t256 < 160) return launch_fast_cfg<2, 2, 1, 2, 2>(b, s);   // 64 x 128
      return launch_fast_cfg<2, 2, 2, 2, 2>(b, s);                    // 128 x 128
    }
  }
  if (b.n == 1 && prefer_320(b.p[0].M, Ks)) return launch_fast_cfg<2, 4, 5, 1, 2>(b, s);   // 320 x 128, 2 stages
  if (Ks > 64) return launch_fast_cfg<4, 2, 2, 2>(b, s);   // 256 x 128
  if (Ks > 32) return launch_fast_cfg<4, 2, 2, 1>(b, s);   // 256 x 64
  return launch_fast_cfg<8, 1, 1, 1>(b, s);                // 256 x 32
}

static int launch_fast(const FastArgs& a, hipStream_t s) {
  if (a.M <= 0) return JPDSE_OK;
  FastBatch b = {};
  b.p[0] = a;
  b.n = 1;
  return launch_fast_batch(b, s);
}

template <int TN, bool SINGLE = false, bool MOM = false, bool VIRT = false, bool NSUM = false>
static int launch_halo_cfg_impl(const HaloArgs& a, hipStream_t s) {
  constexpr int BN = 2 * TN * 32;
  constexpr int UH = ((4 + 2) * (64 + 2) + 7) / 8;
  constexpr int lds = (SINGLE ? 1 : 2) * UH * 1024 + 3 * BN * 128;
  if (int rc = opt_in_lds<&gemm_halo_kernel<4, TN, SINGLE, MOM, VIRT, NSUM>>("gemm_halo", lds)) return rc;
  if (int rc = check_tile_grid("gemm_halo", a.N, a.OH, a.OW, 4, 64, a.Cs, (long long)a.N * a.IH * a.IW * a.Cs, (long long)a.N * a.OH * a.OW * a.Ks)) return rc;
  if (VIRT && (a.V == nullptr || a.py != 1 || a.px != 1 || a.IH != a.OH || a.IW != a.OW || a.OH < 8 || a.reflect || (a.Cs < 128) != SINGLE))
    return set_error(JPDSE_EINVAL, "gemm_halo: folded-frame form needs a frame, pad 1, equal grids, >= 8 rows");
  if (MOM && (a.mom == nullptr || a.mom_slots != (a.OH / 4) * (a.OW / 64)))
    return set_error(JPDSE_EINVAL, "gemm_halo: moment epilogue without a moment buffer of %d slots", (a.OH / 4) * (a.OW / 64));
  if (NSUM && (a.nx == nullptr || a.nstats == nullptr || a.nsums == nullptr || a.mom_slots != (a.OH / 4) * (a.OW / 64) ||
               a.out_sw != a.Ks || a.out_sh != (long long)a.OW * a.Ks || a.out_sn != (long long)a.OH * a.OW * a.Ks || a.out_base != 0))
    return set_error(JPDSE_EINVAL, "gemm_halo: norm-backward sums need the norm's input, its statistics, %d slots and a dense output", (a.OH / 4) * (a.OW / 64));
  const int tiles = a.N * (a.OH / 4) * (a.OW / 64) * ((a.Ks + BN - 1) / BN);
  const long long kdim = 9LL * a.Cs;
  const int M = a.N * a.OH * a.OW;
  const int pslot = prof_begin(s, a.Ks, kdim);
  hipLaunchKernelGGL((gemm_halo_kernel<4, TN, SINGLE, MOM, VIRT, NSUM>), dim3(tiles), dim3(512), lds, s, a);
  prof_end(pslot, 0, 2.0 * (double)M * (double)a.Ks * (double)kdim, s);
  return check_launch("gemm_halo_kernel");
}

JPDSE_SWITCH(int, g_halo_xcd, 0);
// One-round grids of the multi-slab form (the ResnetBlock convs: 32 patches x 8 channel tiles on 256 CUs): XCD-aware tile order 2 -- an XCD
// takes 2 channel tiles x half of the patches instead of every 8th tile, so its L2 pulls a quarter of the filter instead of all of it.
// Measured (profiles/r04_halo_xcd_ab.txt): memory-side fetch 172 -> 103 MB per launch, time unchanged (1194-1199 TFLOP/s either way);
// on multi-round and single-slab grids the same order costs 1-4 %, so it is not used there.  60: off (A/B).
JPDSE_SWITCH(int, g_halo_xcd_auto, 1);
template <int TN>
static int launch_halo_cfg(const HaloArgs& a0, hipStream_t s) {
  HaloArgs a = a0;
  a.xcd_mode = g_halo_xcd;
  {
    const long long blocks = (long long)a.N * (a.OH / 4) * (a.OW / 64) * ((a.Ks + TN * 64 - 1) / (TN * 64));
    if (g_halo_xcd == 0 && g_halo_xcd_auto && a.Cs > 64 && blocks <= 256 && blocks % 8 == 0) a.xcd_mode = 2;
  }
  if (a.V != nullptr) {                   // reflect data gradient with the folded frame
    if constexpr (TN == 2) {
      if (a.nsums != nullptr) {           // ... and the sums of the InstanceNorm backward that consumes its output
        if (a.Cs == 64) return set_error(JPDSE_EINVAL, "gemm_halo: norm-backward sums are built for the double-buffered form (>= 128 input channels)");
        return launch_halo_cfg_impl<TN, false, false, true, true>(a, s);
      }
    }
    if (a.nsums != nullptr) return set_error(JPDSE_EINVAL, "gemm_halo: norm-backward sums need the 128-channel tile");
    if (a.Cs == 64) return launch_halo_cfg_impl<TN, true, false, true>(a, s);     // one slab: single patch buffer
    return launch_halo_cfg_impl<TN, false, false, true>(a, s);
  }
  // conv -> InstanceNorm with the moments in this kernel's epilogue (double-buffered form)
  if (a.mom != nullptr) return launch_halo_cfg_impl<TN, false, true>(a, s);
  if (a.Cs == 64 && g_halo_single) return launch_halo_cfg_impl<TN, true>(a, s);   // one slab: single patch buffer
  return launch_halo_cfg_impl<TN, false>(a, s);
}



// band height of the row-streaming kernels: as tall as possible (the filter load and the ring prologue are paid once per block)
// while the grid still fills the chip (`want` blocks); small problems take 16 / 8 / 4
static int rows_band_height(int N, int OH, int strips, int n_tiles, long long want, int min_th = 4) {
  for (int cand = 64; cand >= min_th; cand >>= 1) {
    if (OH % cand != 0) continue;
    if ((long long)N * strips * (OH / cand) * n_tiles >= want) return cand;
  }
  for (int cand = 16; cand >= min_th; cand >>= 1)
    if (OH % cand == 0) return cand;
  return min_th;
}
// the same choice for the thin-input passes, whose last band may be ragged: fewest (rounds of 512 blocks: two per CU) x (rows per
// block + the ~4 rows a block pays for its filter load and prologue)
static int rows_band_height_by_cost(int N, int OH, int tiles_w) {
  int th = 8;
  long long best = -1;
  for (int cand = 64; cand >= 8; cand >>= 1) {
    const long long blocks = (long long)N * ((OH + cand - 1) / cand) * tiles_w;
    const long long cost = ((blocks + 511) / 512) * (cand + 4);
    if (best < 0 || cost < best) { best = cost; th = cand; }
  }
  return th;
}

// 3x3 convs over 64-channel inputs (conv_rows.h): wave-tile width, band height and moment slots per image of a layer -- the
// launcher's geometry, which the slot query (conv_fwd_moment_slots) reads too
static int rows_wc(int Ks) { return Ks % 128 == 0 ? 4 : 2; }
static int rows_band(int N, int OH, int OW, int Ks, int stride) {
  return rows_band_height(N, OH, OW / 64, Ks / (32 * rows_wc(Ks)), 256LL * ((stride == 1 && rows_wc(Ks) == 2) ? 2 : 1));
}
static int rows_slots(int th, int OH, int OW, int Ks) { return (OH / th) * (OW / 64) * (4 / rows_wc(Ks)); }      // th: rows_band(...)

template <int STRIDE, int WC, bool FUSED>
static int launch_rows_cfg(RowsArgs a, hipStream_t s) {
  typedef RowsGeom<STRIDE, WC> G;
  if (int rc = opt_in_lds<&conv_rows_kernel<STRIDE, WC, FUSED>>("conv_rows", G::LDS)) return rc;
  if (int rc = check_tile_grid("conv_rows", a.N, a.OH, a.OW, 4, 64, 64, (long long)a.N * a.IH * a.IW * 64, (long long)a.N * a.OH * a.OW * a.Ks)) return rc;
  if (a.Ks % (32 * WC) != 0) return set_error(JPDSE_EINVAL, "conv_rows: %d output channels do not split into %d-wide wave tiles", a.Ks, 32 * WC);
  a.n_tiles = a.Ks / (32 * WC);
  a.strips = a.OW / 64;
  if (WC != rows_wc(a.Ks)) return set_error(JPDSE_EINVAL, "conv_rows: %d-wide wave tiles for %d output channels", 32 * WC, a.Ks);
  a.TH = rows_band(a.N, a.OH, a.OW, a.Ks, STRIDE);
  a.bands = a.OH / a.TH;
  a.mom_slots = rows_slots(a.TH, a.OH, a.OW, a.Ks);
  const long long blocks = (long long)a.N * a.bands * a.strips * a.n_tiles;
  if (blocks > 0x7fffffffLL) return set_error(JPDSE_EINVAL, "conv_rows: grid too large");
  hipLaunchKernelGGL((conv_rows_kernel<STRIDE, WC, FUSED>), dim3((unsigned)blocks), dim3(256), G::LDS, s, a);
  return check_launch("conv_rows_kernel");
}

static int launch_rows(const RowsArgs& a, int stride, hipStream_t s) {
  const bool fused = a.mask != nullptr || a.addend != nullptr;
  const bool wide = rows_wc(a.Ks) == 4;
  if (stride == 1) {
    if (wide) return fused ? launch_rows_cfg<1, 4, true>(a, s) : launch_rows_cfg<1, 4, false>(a, s);
    return fused ? launch_rows_cfg<1, 2, true>(a, s) : launch_rows_cfg<1, 2, false>(a, s);
  }
  if (wide) return fused ? launch_rows_cfg<2, 4, true>(a, s) : launch_rows_cfg<2, 4, false>(a, s);
  return fused ? launch_rows_cfg<2, 2, true>(a, s) : launch_rows_cfg<2, 2, false>(a, s);
}


// data gradient of the 64 -> 128 3x3 stride-2 conv / forward of the 128 -> 64 ConvTranspose2d at full resolution (dgrad2_rows.h)
static int dgrad2_rows_band(int N, int OH, int OW) { return rows_band_height(N, OH, OW / 64, 1, 256); }
static int dgrad2_rows_slots(int th, int OH, int OW) { return (OH / th) * (OW / 64); }      // moment slots per image; th: dgrad2_rows_band(...)
static int launch_dgrad2_rows(Dgrad2Args a, hipStream_t s) {
  typedef Dgrad2Geom G;
  if (int rc = opt_in_lds<&dgrad2_rows_kernel>("dgrad2_rows", G::LDS)) return rc;
  if (int rc = check_tile_grid("dgrad2_rows", a.N, a.OH, a.OW, 4, 64, 128, (long long)a.N * a.OH * a.OW * 128, 4LL * a.N * a.OH * a.OW * 64)) return rc;
  a.strips = a.OW / 64;
  const int th = dgrad2_rows_band(a.N, a.OH, a.OW);
  a.TH = th;
  a.bands = a.OH / th;
  a.mom_slots = dgrad2_rows_slots(th, a.OH, a.OW);
  hipLaunchKernelGGL(dgrad2_rows_kernel, dim3((unsigned)(a.N * a.bands * a.strips)), dim3(256), G::LDS, s, a);
  return check_launch("dgrad2_rows_kernel");
}


// 64 -> <= 3 channel heads (7x7 reflect + Tanh; 3x3 zero-pad data gradient of VGG conv1_1) as a row-streaming pass (head_rows.h)
template <int R, int CIN = 64>
static int launch_head_rows(const HeadFwdArgs& a, hipStream_t s) {
  typedef HeadRowsGeom<R, CIN> G;
  if (int rc = opt_in_lds<&head_rows_kernel<R, CIN>>("head_rows", G::LDS)) return rc;
  const int strips = a.OW / 128;
  if (a.OH % 8 != 0 || strips == 0 || a.OW % 128 != 0)       // (rows_band_height would answer its minimum for a height no band divides)
    return set_error(JPDSE_EINVAL, "head_rows: output grid %d x %d does not tile into bands of >= 8 rows x 128-pixel strips", a.OH, a.OW);
  const int th = rows_band_height(a.N, a.OH, strips, 1, 512, 8);
  const int bands = a.OH / th;
  hipLaunchKernelGGL((head_rows_kernel<R, CIN>), dim3((unsigned)(a.N * bands * strips)), dim3(256), G::LDS, s, a, th, bands, strips);
  return check_launch("head_rows_kernel");
}


// data gradient of PatchGAN layer 0 with respect to the image channels (thin_dgrad2_rows.h)
static int launch_thin_dgrad2_rows(ThinDgrad2Args a, hipStream_t s) {
  typedef ThinDgrad2Geom G;
  if (int rc = opt_in_lds<&thin_dgrad2_rows_kernel>("thin_dgrad2_rows", G::LDS)) return rc;
  if (a.H % 8 != 0 || a.W <= 0 || a.W % 256 != 0)
    return set_error(JPDSE_EINVAL, "thin_dgrad2_rows: image of %d x %d does not tile into bands of >= 8 rows x 256-pixel strips", a.H, a.W);
  a.strips = a.W / 256;
  a.TH = rows_band_height(a.N, a.H, a.strips, 1, 512, 8);
  a.bands = a.H / a.TH;
  hipLaunchKernelGGL(thin_dgrad2_rows_kernel, dim3((unsigned)(a.N * a.bands * a.strips)), dim3(256), G::LDS, s, a);
  return check_launch("thin_dgrad2_rows_kernel");
}


// PatchGAN layer 0 forward (40-channel input, 4x4 stride 2, 64 outputs) as a row-streaming pass (thin_rows.h)
static int launch_thin_rows(ThinFwdArgs a, hipStream_t s) {
  typedef ThinRowsGeom G;
  if (int rc = opt_in_lds<&thin_rows_kernel>("thin_rows", G::LDS)) return rc;
  a.tiles_w = (a.OW + 63) / 64;
  const int th = rows_band_height_by_cost(a.N, a.OH, a.tiles_w);
  const int bands = (a.OH + th - 1) / th;
  hipLaunchKernelGGL(thin_rows_kernel, dim3((unsigned)(a.N * bands * a.tiles_w)), dim3(256), G::LDS, s, a, th, bands);
  return check_launch("thin_rows_kernel");
}


// dense 8-channel inputs, 64 outputs, as a row-streaming pass (thin_in_rows.h): the data gradient of the 64 -> 3 7x7 reflect-padded
// head (padded-domain conv with the interior written straight into dx, then the ring fold) and VGG conv1_1 forward (3x3, zero pad)
template <int R, bool DUAL>
static int launch_thin_in_rows(ThinInArgs a, hipStream_t s) {
  typedef ThinInGeom<R> G;
  if (int rc = opt_in_lds<&thin_in_rows_kernel<R, DUAL>>("thin_in_rows", G::LDS)) return rc;
  a.strips = (a.OW + 63) / 64;
  a.TH = rows_band_height_by_cost(a.N, a.OH, a.strips);
  a.bands = (a.OH + a.TH - 1) / a.TH;
  hipLaunchKernelGGL((thin_in_rows_kernel<R, DUAL>), dim3((unsigned)(a.N * a.bands * a.strips)), dim3(256), G::LDS, s, a);
  if (int rc = check_launch("thin_in_rows_kernel")) return rc;
  if (DUAL) {
    const int band = G::PAD + 1;
    const long long per_img = 2LL * band * a.W + (long long)(a.H - 2 * band) * 2 * band;
    const long long total_vec = (long long)a.N * per_img * (64 / 8);
    hipLaunchKernelGGL((reflect_ring_fold_kernel<bf16_t>), dim3(ew_blocks(total_vec)), dim3(256), 0, s, a.DXP, a.DX, a.N, a.H, a.W,
                       64, G::PAD, total_vec);
    return check_launch("reflect_ring_fold_kernel");
  }
  return JPDSE_OK;
}

// ---- tap-program halo kernel (gemm_taps.h) on the stride-2 data gradients: taps_dgrad2_geom (conv_route.h) says which
template <int TN>
static int launch_taps_dgrad2_cfg(const TapsArgs& a, int total, hipStream_t s) {
  constexpr int PH = 5, PW = 65;
  constexpr int lds = 2 * ((PH * PW + 7) / 8) * 1024 + 3 * (2 * TN * 32) * 128;
  if (int rc = opt_in_lds<&gemm_taps_kernel<TN, 4, 1, 2, 2, 1, PH, PW>>("gemm_taps", lds)) return rc;
  if (int rc = check_tile_grid("gemm_taps(stride-2 data gradient)", a.N, a.OH, a.OW, 4, 64, a.Cs, (long long)a.N * a.IH * a.IW * a.Cs,
                               4LL * a.N * a.OH * a.OW * a.Ks)) return rc;
  if (total != 2 * a.nblk0 || a.nblk0 != a.N * (a.OH / 4) * (a.OW / 64) * ((a.Ks + 2 * TN * 32 - 1) / (2 * TN * 32)))
    return set_error(JPDSE_EINVAL, "gemm_taps: %d blocks for a grid of 2 x %d", total, a.nblk0);
  hipLaunchKernelGGL((gemm_taps_kernel<TN, 4, 1, 2, 2, 1, PH, PW>), dim3(total), dim3(512), lds, s, a);
  return check_launch("gemm_taps_kernel");
}

static int launch_taps_dgrad2(const jpdse_conv_desc* d, const ConvPlan& p, const void* dy, const void* pack, void* dx, hipStream_t s,
                              const void* mask, const void* addend, float mask_slope = 0.f) {
  TapsDgrad2Geom geo = {};
  if (!taps_dgrad2_geom(d, p, false, &geo)) return set_error(JPDSE_EINVAL, "gemm_taps: not a stride-2 data gradient it covers");
  TapsArgs a = {};
  a.mask = reinterpret_cast<const bf16_t*>(mask);
  a.mask_slope = mask_slope;
  a.addend = reinterpret_cast<const bf16_t*>(addend);
  a.X = reinterpret_cast<const bf16_t*>(dy);
  a.Y = reinterpret_cast<bf16_t*>(dx);
  a.N = d->N;
  a.OH = geo.core_h;
  a.OW = geo.core_w;
  a.IH = p.OH;
  a.IW = p.OW;
  a.Cs = p.Ks;
  a.py = a.px = 0;
  a.Kout = d->C;
  a.Ks = p.Cs;
  a.b_rows = p.Cs;
  a.out_sn = (long long)d->H * d->W * p.Cs;
  a.out_sh = 2LL * d->W * p.Cs;
  a.out_sw = 2LL * p.Cs;
  a.act = JPDSE_ACT_NONE;
  // program 0 = {phase (0,0), phase (1,1)}, program 1 = {phase (0,1), phase (1,0)}: 4 + 1 and 2 + 2 taps
  const Phase* byq[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
  for (int i = 0; i < 4; ++i) byq[p.ph[i].qh][p.ph[i].qw] = &p.ph[i];
  const Phase* sets[2][2] = {{byq[0][0], byq[1][1]}, {byq[0][1], byq[1][0]}};
  constexpr int PW = 65;
  for (int g = 0; g < 2; ++g) {
    int t = 0;
    for (int q = 0; q < 2; ++q) {
      const Phase& f = *sets[g][q];
      a.prog[g].B[q] = reinterpret_cast<const bf16_t*>(reinterpret_cast<const char*>(pack) + f.pack_off);
      a.prog[g].ktot[q] = (long long)f.Uh * f.Lk;
      a.prog[g].out_base[q] = ((long long)(2 * f.i0h + f.qh - d->pad) * d->W + (2 * f.i0w + f.qw - d->pad)) * p.Cs;
      for (int u = 0; u < f.Uh; ++u)
        for (int w = 0; w < f.Uw; ++w) {
          a.prog[g].tap_off[t] = u * PW + w;
          a.prog[g].tap_koff[t] = u * f.Lk + w * p.Ks;
          ++t;
        }
    }
  }
  const int bn = p.Cs % 128 == 0 ? 128 : 64;
  a.nblk0 = d->N * (a.OH / 4) * (a.OW / 64) * ((p.Cs + bn - 1) / bn);
  return bn == 128 ? launch_taps_dgrad2_cfg<2>(a, 2 * a.nblk0, s) : launch_taps_dgrad2_cfg<1>(a, 2 * a.nblk0, s);
}

// ---- 4x4 stride-1 zero-padded convs and their (single-phase) data gradient on the tap-program kernel: PatchGAN layer 3 of
// both scales (networks.py:430-449).  Their grids are odd (66 x 130, 34 x 66): the kernel's 8 x 32 tiles cover the CORE
// (64 x 128: 95 % of the pixels) with the 11 x 35 input patch staged once per 64-channel slab for all 16 taps; the fringe (the
// last OH % 8 rows, the last OW % 32 columns) runs as two sub-rectangle problems of ONE split-K launch of gemm_fast_kernel
// (fp32 slabs, fixed summation order) + its finish kernels.
static int taps4_fringe_splits(int N, int OH, int OW, int Ks_out, int k_tiles) {
  const int OHc = OH / 8 * 8, OWc = OW / 32 * 32;
  const long long m_bot = (long long)N * (OH - OHc) * OW, m_right = (long long)N * OHc * (OW - OWc);
  const long long nt = (Ks_out + 127) / 128;
  const long long tiles = ((m_bot + 255) / 256 + (m_right + 255) / 256) * nt;
  if (tiles <= 0) return 0;
  long long sp = 256 / tiles;
  if (sp > k_tiles / 8) sp = k_tiles / 8;
  if (sp > 8) sp = 8;
  return sp < 1 ? 1 : (int)sp;
}

static size_t taps4_fringe_bytes(int N, int OH, int OW, int Ks_out, int k_tiles) {
  const int OHc = OH / 8 * 8, OWc = OW / 32 * 32;
  const long long m = (long long)N * (OH - OHc) * OW + (long long)N * OHc * (OW - OWc);
  return (size_t)taps4_fringe_splits(N, OH, OW, Ks_out, k_tiles) * m * Ks_out * sizeof(float);
}

template <int TN>
static int launch_taps4_cfg(const TapsArgs& a, int total, hipStream_t s) {
  constexpr int PH = 11, PW = 35;
  constexpr int lds = 2 * ((PH * PW + 7) / 8) * 1024 + 3 * (2 * TN * 32) * 128;
  if (int rc = opt_in_lds<&gemm_taps_kernel<TN, 16, 0, 0, 0, 2, PH, PW>>("gemm_taps(4x4)", lds)) return rc;
  if (int rc = check_tile_grid("gemm_taps(4x4)", a.N, a.OH, a.OW, 8, 32, a.Cs, (long long)a.N * a.IH * a.IW * a.Cs,
                               (long long)a.N * a.OH * a.OW * a.Ks)) return rc;
  if (total != a.N * (a.OH / 8) * (a.OW / 32) * ((a.Ks + 2 * TN * 32 - 1) / (2 * TN * 32)))
    return set_error(JPDSE_EINVAL, "gemm_taps(4x4): %d blocks do not match the tile grid", total);
  hipLaunchKernelGGL((gemm_taps_kernel<TN, 16, 0, 0, 0, 2, PH, PW>), dim3(total), dim3(512), lds, s, a);
  return check_launch("gemm_taps_kernel(4x4)");
}

// one-program TapsArgs of a stride-1 view: every filter tap of the R x S window over a staged patch of `patch_w` pixels per row
static TapsArgs to_taps(const ConvView& v, int patch_w) {
  TapsArgs a = {};
  a.X = v.X;
  a.Y = v.Y;
  a.bias = v.bias;
  a.N = v.N; a.OH = v.OH; a.OW = v.OW; a.IH = v.IH; a.IW = v.IW; a.Cs = v.Cin_s;
  a.py = v.py; a.px = v.px;
  a.Kout = v.Kout; a.Ks = v.Ks_out; a.b_rows = v.Ks_out;
  a.out_sn = v.out_sn; a.out_sh = v.out_sh; a.out_sw = v.out_sw;
  a.act = v.act;
  a.slope = v.slope;
  a.addend = v.addend;
  a.mask = v.mask;
  a.alias = v.alias; a.addend_n = v.addend_n;
  a.prog[0].B[0] = v.B;
  a.prog[0].ktot[0] = v.ktot;
  a.prog[0].out_base[0] = v.out_base;
  for (int r = 0; r < v.R; ++r)
    for (int c = 0; c < v.S; ++c) {
      a.prog[0].tap_off[r * v.S + c] = r * patch_w + c;
      a.prog[0].tap_koff[r * v.S + c] = r * v.tap_r + c * v.tap_s;
    }
  return a;
}

static int launch_taps4(const ConvView& v, void* ws, hipStream_t s) {
  const int OHc = v.OH / 8 * 8, OWc = v.OW / 32 * 32;
  TapsArgs a = to_taps(v, 35);
  a.OH = OHc;                    // the kernel covers the core, the fast kernel the fringe
  a.OW = OWc;
  const int bn = v.Ks_out % 128 == 0 ? 128 : 64;
  a.nblk0 = v.N * (OHc / 8) * (OWc / 32) * ((v.Ks_out + bn - 1) / bn);
  if (int rc = bn == 128 ? launch_taps4_cfg<2>(a, a.nblk0, s) : launch_taps4_cfg<1>(a, a.nblk0, s)) return rc;
  // fringe: bottom rows [OHc, OH) x all columns, right columns [OWc, OW) x rows [0, OHc)
  const int k_tiles = 16 * v.Cin_s / 64;
  const int sp = taps4_fringe_splits(v.N, v.OH, v.OW, v.Ks_out, k_tiles);
  if (sp == 0) return JPDSE_OK;
  FastBatch fb = {};
  float* slab = reinterpret_cast<float*>(ws);
  const int rect[2][4] = {{OHc, 0, v.OH - OHc, v.OW}, {0, OWc, OHc, v.OW - OWc}};     // oh0, ow0, rows, cols
  for (int q = 0; q < 2; ++q) {
    const int oh0 = rect[q][0], ow0 = rect[q][1], rows = rect[q][2], cols = rect[q][3];
    if (rows <= 0 || cols <= 0) continue;
    FastArgs g = to_fast(v);      // (addend / mask are applied by splitk_finish_kernel)
    g.M = v.N * rows * cols;
    g.OH = rows;
    g.OW = cols;
    g.py = v.py - oh0;
    g.px = v.px - ow0;
    g.out_base = v.out_base + oh0 * v.out_sh + ow0 * v.out_sw;
    g.splits = sp;
    g.no_finish = 1;
    g.partial = slab;
    g.b_stride = v.ktot;
    g.b_tap_r = v.tap_r;
    g.b_tap_s = v.tap_s;
    slab += (size_t)sp * g.M * v.Ks_out;
    fb.p[fb.n++] = g;
  }
  if (int rc = launch_fast_batch(fb, s)) return rc;
  for (int q = 0; q < fb.n; ++q) {
    const long long total_vec = (long long)fb.p[q].M * (fb.p[q].Ks / 8);
    hipLaunchKernelGGL(splitk_finish_kernel, dim3(ew_blocks(total_vec)), dim3(256), 0, s, fb.p[q], total_vec);
  }
  return check_launch("taps4 fringe finish");
}

// ---- 3x3 stride-1 convs whose grid does not tile into the halo kernel's 4 x 64 patches but into 8 x 32 ones (W = 32: the
// 1024-channel ResnetBlocks of the LocalEnhancer trunk at 16 x 32 pixels, BASELINE config 3): the tap-program kernel with nine
// taps, zero or mirrored padding in the patch loader, and -- few tiles, K = 9216 -- split-K over the channel slabs.
static int taps9_splits(int N, int OH, int OW, int Cin_s, int Ks_out) {
  const int sp = splitk_for(N * OH * OW, Ks_out, 9 * Cin_s / 64);      // the split-K fast path's choice: its workspace region is reused
  const int cc = Cin_s / 64;
  return sp > cc / 2 ? (cc / 2 > 0 ? cc / 2 : 1) : sp;                 // >= 2 slabs (18 tap steps) per block
}

template <int TN, bool VIRT = false>
static int launch_taps9_cfg(const TapsArgs& a, int total, hipStream_t s) {
  constexpr int PH = 10, PW = 34;
  constexpr int lds = 2 * ((PH * PW + 7) / 8) * 1024 + 3 * (2 * TN * 32) * 128;
  if (int rc = opt_in_lds<&gemm_taps_kernel<TN, 9, 0, 0, 0, 2, PH, PW, VIRT>>("gemm_taps(3x3)", lds)) return rc;
  if (int rc = check_tile_grid("gemm_taps(3x3)", a.N, a.OH, a.OW, 8, 32, a.Cs, (long long)a.N * a.IH * a.IW * a.Cs,
                               (long long)a.N * a.OH * a.OW * a.Ks)) return rc;
  const int sp = a.splits > 1 ? a.splits : 1;
  if (total != sp * a.N * (a.OH / 8) * (a.OW / 32) * ((a.Ks + 2 * TN * 32 - 1) / (2 * TN * 32)) || (sp > 1 && a.partial == nullptr))
    return set_error(JPDSE_EINVAL, "gemm_taps(3x3): %d blocks do not match the tile grid x %d splits", total, sp);
  if (VIRT && (a.V == nullptr || a.py != 1 || a.px != 1 || a.IH != a.OH || a.IW != a.OW || a.OH < 16 || a.reflect))
    return set_error(JPDSE_EINVAL, "gemm_taps(3x3): folded-frame form needs a frame, pad 1, equal grids, >= 16 rows");
  hipLaunchKernelGGL((gemm_taps_kernel<TN, 9, 0, 0, 0, 2, PH, PW, VIRT>), dim3(total), dim3(512), lds, s, a);
  return check_launch("gemm_taps_kernel(3x3)");
}

// `slabs`: fp32 workspace of >= splits * N OH OW * Ks_out floats (the plan's split-K region)
static int launch_taps9(const ConvView& v, float* slabs, hipStream_t s) {
  TapsArgs a = to_taps(v, 34);
  a.reflect = v.reflect;
  a.V = v.frame;
  const int bn = v.Ks_out % 128 == 0 ? 128 : 64;
  const int tiles = v.N * (v.OH / 8) * (v.OW / 32) * ((v.Ks_out + bn - 1) / bn);
  a.splits = taps9_splits(v.N, v.OH, v.OW, v.Cin_s, v.Ks_out);
  a.partial = a.splits > 1 ? slabs : nullptr;
  a.nblk0 = tiles * (a.splits > 1 ? a.splits : 1);
  int rc;
  if (v.frame != nullptr) rc = bn == 128 ? launch_taps9_cfg<2, true>(a, a.nblk0, s) : launch_taps9_cfg<1, true>(a, a.nblk0, s);
  else rc = bn == 128 ? launch_taps9_cfg<2>(a, a.nblk0, s) : launch_taps9_cfg<1>(a, a.nblk0, s);
  if (rc) return rc;
  if (a.splits <= 1) return JPDSE_OK;
  FastArgs f = {};                                  // what splitk_finish_kernel reads
  f.Y = v.Y;
  f.bias = v.bias;
  f.M = v.N * v.OH * v.OW;
  f.OH = v.OH;
  f.OW = v.OW;
  f.Kout = v.Kout;
  f.Ks = v.Ks_out;
  f.out_sn = v.out_sn;
  f.out_sh = v.out_sh;
  f.out_sw = v.out_sw;
  f.out_base = v.out_base;
  f.act = v.act;
  f.slope = v.slope;
  f.splits = a.splits;
  f.partial = slabs;
  f.addend = v.addend;
  f.mask = v.mask;
  const long long total_vec = (long long)f.M * (f.Ks / 8);
  hipLaunchKernelGGL(splitk_finish_kernel, dim3(ew_blocks(total_vec)), dim3(256), 0, s, f, total_vec);
  return check_launch("taps9 split-K finish");
}

// Convs with K*R*S <= 32 outputs-times-taps (the 512 -> 1 PatchGAN map): y[p][k] = sum_taps Z[p + tap][k, tap] with
// Z[q][(k, tap)] = sum_c x[q][c] * w[k][tap][c] -- a 1x1 GEMM over the INPUT pixels (K*R*S <= 32 columns: one MFMA
// tile, every input pixel read once, no padded copy) followed by this gather-sum over the taps.  The direct
// form wastes 31 of 32 MFMA columns and re-reads the input once per tap.
__global__ __launch_bounds__(256) void tapsum_kernel(const float* __restrict__ Z, const float* __restrict__ bias,
                                                    bf16_t* __restrict__ y, int N, int H, int W, int OH, int OW,
                                                    int K, int Ks_out, int R, int S, int pad, int reflect, int zs,
                                                    int act, float slope, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;   // over output pixels x Ks_out
  if (idx >= total) return;
  const int k = (int)(idx % Ks_out);
  long long t = idx / Ks_out;
  const int ow = (int)(t % OW);
  t /= OW;
  const int oh = (int)(t % OH), n = (int)(t / OH);
  float v = 0.f;
  if (k < K) {
    v = bias != nullptr ? bias[k] : 0.f;
    for (int r = 0; r < R; ++r) {
      int ih = oh + r - pad;
      if (reflect) ih = ih < 0 ? -ih : (ih >= H ? 2 * (H - 1) - ih : ih);
      else if ((unsigned)ih >= (unsigned)H) continue;
      for (int s2 = 0; s2 < S; ++s2) {
        int iw = ow + s2 - pad;
        if (reflect) iw = iw < 0 ? -iw : (iw >= W ? 2 * (W - 1) - iw : iw);
        else if ((unsigned)iw >= (unsigned)W) continue;
        v += Z[(((long long)n * H + ih) * W + iw) * zs + (k * R + r) * S + s2];
      }
    }
    v = apply_act(v, act, slope);
  }
  y[idx] = f2bf(v);
}

template <int TN, int TH, int ST, int TW>
static int launch_thin_fwd(const ThinFwdArgs& a, int lds, hipStream_t s) {
  if (int rc = opt_in_lds<&thin_fwd_kernel<TN, TH, ST, TW>>("thin_fwd", 160 * 1024)) return rc;
  hipLaunchKernelGGL((thin_fwd_kernel<TN, TH, ST, TW>), dim3(a.N * a.tiles_h * a.tiles_w), dim3(512), lds, s, a);
  return check_launch("thin_fwd_kernel");
}

template <int CIN, int NT = 5, int FR = 7, int FS = 7>
static int launch_head_fwd(const HeadFwdArgs& a, hipStream_t s) {
  constexpr int lds = NT * 32 * CIN * 2 + 3 * kHeadMR * CIN * 2 + NT * 32 * kHeadZP * 4 + kHeadTH * 64 * 4 * 4;
  if (int rc = opt_in_lds<&head_fwd_kernel<CIN, NT, FR, FS>>("head_fwd", lds)) return rc;
  hipLaunchKernelGGL((head_fwd_kernel<CIN, NT, FR, FS>), dim3(a.N * a.tiles_h * a.tiles_w), dim3(64 * NT), lds, s, a);
  return check_launch("head_fwd_kernel");
}

}  // namespace jpdse
