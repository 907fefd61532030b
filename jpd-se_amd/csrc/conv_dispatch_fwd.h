// Forward dispatch of the convolution family: conv_fwd_t launches the route select_fwd (conv_route.h) chose, one function per
// route, and the moment-slot query reads the same choice.  Part of conv_gemm.hip (one translation unit).
#pragma once

namespace jpdse {

// what a forward route is handed.  pool != nullptr: the caller wants MaxPool2d(2, 2) of y as well; the route that can write it
// from its epilogue sets *pooled.  mom != nullptr: the caller asked jpdse_conv_moment_slots first, so the route is one that writes them
struct FwdCall {
  const jpdse_conv_desc* d; const ConvPlan& p;
  const void* x; const void* pack; const float* bias; void* y; void* ws; hipStream_t s;
  float* mom; void* pool; bool* pooled;
};

static int fwd_thin_in_rows(const FwdCall& c) {      // VGG conv1_1: plain forward panel [k][r][(s, c8) 24 -> 32]
  ThinInArgs g = {};
  g.DY = reinterpret_cast<const bf16_t*>(c.x);
  g.P = reinterpret_cast<const bf16_t*>(c.pack);
  g.DX = reinterpret_cast<bf16_t*>(c.y);
  g.bias = c.bias;
  g.act = c.d->act; g.slope = c.d->slope;
  g.N = c.d->N; g.H = c.d->H; g.W = c.d->W; g.OH = c.p.OH; g.OW = c.p.OW;
  g.py = g.px = 1;
  return launch_thin_in_rows<3, false>(g, c.s);
}

// moment slots per image of the thin forward kernel: one per TH x TW tile, when the tiles divide the output
static int thin_fwd_slots(const ConvPlan& p, const ThinFwdGeom& tg) {
  return (p.OH % tg.TH == 0 && p.OW % tg.TW == 0) ? (p.OH / tg.TH) * (p.OW / tg.TW) : 0;
}
static int fwd_thin(const FwdCall& c, FwdRoute route) {      // thin_rows | thin_fwd
  const jpdse_conv_desc* d = c.d;
  const ConvPlan& p = c.p;
  ThinFwdGeom tg;
  if (!thin_fwd_geom(d, p, &tg)) return set_error(JPDSE_EINVAL, "thin_fwd: not a thin-input layer");
  ThinFwdArgs t = {};
  t.X = reinterpret_cast<const bf16_t*>(c.x);
  t.Wt = reinterpret_cast<const bf16_t*>(reinterpret_cast<const char*>(c.pack) + p.thin_pack_off);
  t.bias = c.bias;
  t.Y = reinterpret_cast<bf16_t*>(c.y);
  t.N = d->N; t.H = d->H; t.W = d->W; t.OH = p.OH; t.OW = p.OW;
  t.Cs = p.Cs; t.K = d->K; t.Ks = p.Ks;
  t.R = d->R; t.S = d->S; t.pad = d->pad;
  t.reflect = d->pad_mode == JPDSE_PAD_REFLECT;
  t.act = d->act; t.slope = d->slope;
  t.KP = p.KP_thin;
  t.ksteps = (p.KP_thin - 8) / 16;
  t.strip_units = tg.strip_units;
  t.w_units = tg.w_units;
  t.tiles_w = (p.OW + tg.TW - 1) / tg.TW;
  t.tiles_h = (p.OH + tg.TH - 1) / tg.TH;
  if (route == FwdRoute::thin_rows) return launch_thin_rows(t, c.s);
  if (c.mom != nullptr) {
    t.mom = c.mom;
    t.mom_slots = t.tiles_w * t.tiles_h;       // == thin_fwd_slots: the query answered > 0, so the tiles divide the output
  }
  if (d->stride == 1) {
    if (tg.TH == 8) return p.Ks == 64 ? launch_thin_fwd<2, 8, 1, 64>(t, tg.lds, c.s) : launch_thin_fwd<1, 8, 1, 64>(t, tg.lds, c.s);
    return tg.TW == 64 ? launch_thin_fwd<1, 4, 1, 64>(t, tg.lds, c.s) : launch_thin_fwd<1, 4, 1, 32>(t, tg.lds, c.s);
  }
  if (tg.TH == 8) return p.Ks == 64 ? launch_thin_fwd<2, 8, 2, 64>(t, tg.lds, c.s) : launch_thin_fwd<1, 8, 2, 64>(t, tg.lds, c.s);
  return tg.TW == 64 ? launch_thin_fwd<1, 4, 2, 64>(t, tg.lds, c.s) : launch_thin_fwd<1, 4, 2, 32>(t, tg.lds, c.s);
}

static int fwd_head(const FwdCall& c, FwdRoute route) {      // head_rows | head_fwd
  const jpdse_conv_desc* d = c.d;
  const ConvPlan& p = c.p;
  HeadFwdArgs h = {};
  h.X = reinterpret_cast<const bf16_t*>(c.x);
  h.Wp = reinterpret_cast<const bf16_t*>(c.pack);
  h.bias = c.bias;
  h.Y = reinterpret_cast<bf16_t*>(c.y);
  h.N = d->N; h.H = d->H; h.W = d->W; h.OH = p.OH; h.OW = p.OW;
  h.K = d->K; h.Ks_out = p.Ks;
  h.R = d->R; h.S = d->S; h.pad = d->pad;
  h.reflect = d->pad_mode == JPDSE_PAD_REFLECT;
  h.act = d->act; h.slope = d->slope;
  h.tiles_w = (p.OW + 63) / 64;
  h.tiles_h = (p.OH + kHeadTH - 1) / kHeadTH;
  if (route == FwdRoute::head_rows) return p.Cs == 64 ? launch_head_rows<7>(h, c.s) : launch_head_rows<7, 32>(h, c.s);
  return p.Cs == 64 ? launch_head_fwd<64>(h, c.s) : launch_head_fwd<32>(h, c.s);
}

static int fwd_tapsum(const FwdCall& c) {
  const jpdse_conv_desc* d = c.d;
  const ConvPlan& p = c.p;
  const int cols = d->K * d->R * d->S, zs = (cols + 7) / 8 * 8;
  FastArgs f = {};
  f.X = reinterpret_cast<const bf16_t*>(c.x);
  f.B = reinterpret_cast<const bf16_t*>(c.pack);     // row k of the plain panel = [R*S][Cs]: K*R*S rows of Cs
  f.M = d->N * d->H * d->W; f.OH = f.IH = d->H; f.OW = f.IW = d->W;
  f.Cs = p.Cs; f.R = f.S = 1; f.sy = f.sx = 1;
  f.Kout = f.b_rows = cols; f.Ks = zs;
  f.act = JPDSE_ACT_NONE;
  f.splits = 1; f.no_finish = 1; f.partial = reinterpret_cast<float*>(c.ws);      // the fp32 Z goes to the workspace
  if (int rc = launch_fast(f, c.s)) return rc;
  const long long total = (long long)d->N * p.OH * p.OW * p.Ks;
  hipLaunchKernelGGL(tapsum_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c.s, f.partial, c.bias,
                     reinterpret_cast<bf16_t*>(c.y), d->N, d->H, d->W, p.OH, p.OW, d->K, p.Ks, d->R, d->S, d->pad,
                     d->pad_mode == JPDSE_PAD_REFLECT ? 1 : 0, zs, d->act, d->slope, total);
  return check_launch("tapsum_kernel");
}

static ConvView fwd_view(const FwdCall& c) {
  ConvView v = view_fwd(c.d, c.p, c.x, c.pack, c.bias, c.y);
  v.mom = c.mom;
  return v;
}
static float* splitk_slabs(const ConvPlan& p, void* ws) { return reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + p.splitk_off); }

static int fwd_halo(const FwdCall& c) {
  HaloArgs h = to_halo(fwd_view(c));
  if (c.pool != nullptr && c.mom == nullptr && c.pooled != nullptr) {
    h.pool = reinterpret_cast<bf16_t*>(c.pool);
    *c.pooled = true;
  }
  return c.p.Ks > 64 ? launch_halo_cfg<2>(h, c.s) : launch_halo_cfg<1>(h, c.s);
}

static int fwd_fast(const FwdCall& c) {
  FastArgs f = to_fast(fwd_view(c));
  f.splits = splitk_for(f.M, c.p.Ks, c.d->R * c.d->S * c.p.Cs / 64);
  f.partial = splitk_slabs(c.p, c.ws);
  return launch_fast(f, c.s);
}

// generic path: staged through the workspace, the GEMM loaders rely on the zeroed slack behind it.  toep (heads): `px` = 4 output
// pixels x 8 channels per 32-wide GEMM row over the Toeplitz panel (see pack_fwd_toep_kernel); the [M/4][32] result IS the NHWC output
template <typename T>
static int fwd_gemm(const FwdCall& c, bool toep) {
  const jpdse_conv_desc* d = c.d;
  const ConvPlan& p = c.p;
  if (int rc = launch_pad<T>(c.x, c.ws, d->N, d->H, d->W, p.Cs, d->pad, d->pad, d->pad, d->pad, d->pad_mode, c.s)) return rc;
  const int px = toep ? 4 : 1, Lk = toep ? p.Lk_toep : p.Lk_fwd;
  GemmFwdArgs a = {};
  a.A = c.ws;
  a.B = toep ? reinterpret_cast<const char*>(c.pack) + p.fwd_pack_plain_bytes : c.pack;
  a.bias = c.bias;
  a.Y = c.y;
  a.OH = p.OH; a.OW = p.OW / px; a.M = d->N * a.OH * a.OW;
  a.Kout = toep ? 32 : d->K; a.Ks = a.b_rows = toep ? 32 : p.Ks;
  a.R = d->R; a.cpr = Lk / p.BKE; a.b_row_stride = (long long)d->R * Lk;
  a.in_sn = (long long)p.Hp * p.Wp * p.Cs; a.in_sr = (long long)p.Wp * p.Cs;
  a.in_sh = (long long)d->stride * p.Wp * p.Cs;      // (the Toeplitz panel exists for stride 1 only)
  a.in_sw = (long long)px * d->stride * p.Cs;
  a.out_sn = (long long)p.OH * p.OW * p.Ks; a.out_sh = (long long)p.OW * p.Ks; a.out_sw = (long long)px * p.Ks;
  a.act = d->act; a.slope = d->slope;
  if (toep) {
    a.col_mod = 8;
    a.k_real = d->K;
  } else {
    a.partial = splitk_slabs(p, c.ws);   // split-K slabs (fp32 layers with few tiles)
    a.partial_cap = p.splitk_bytes;
  }
  return launch_fwd<T>(a, c.s);
}

template <typename T>
static int conv_fwd_t(const jpdse_conv_desc* d, const ConvPlan& p, const void* x, const void* pack,
                      const float* bias, void* y, void* ws, hipStream_t s, float* mom = nullptr, void* pool = nullptr,
                      bool* pooled = nullptr) {
  const FwdCall c = {d, p, x, pack, bias, y, ws, s, mom, pool, pooled};
  const FwdRoute route = select_fwd(d, p, {mom != nullptr, pool != nullptr});
  if constexpr (sizeof(T) == 2) {      // (the bf16 kernels are not instantiated for fp32 layers, which select_fwd sends to the generic GEMM)
    switch (route) {
      case FwdRoute::thin_in_rows: return fwd_thin_in_rows(c);
      case FwdRoute::thin_rows:
      case FwdRoute::thin_fwd: return fwd_thin(c, route);
      case FwdRoute::head_rows:
      case FwdRoute::head_fwd: return fwd_head(c, route);
      case FwdRoute::tapsum: return fwd_tapsum(c);
      case FwdRoute::rows: return launch_rows(to_rows(fwd_view(c)), d->stride, s);
      case FwdRoute::taps4: return launch_taps4(fwd_view(c), ws, s);
      case FwdRoute::taps9: return launch_taps9(fwd_view(c), splitk_slabs(p, ws), s);
      case FwdRoute::halo: return fwd_halo(c);
      case FwdRoute::fast: return fwd_fast(c);
      default: break;
    }
  }
  return fwd_gemm<T>(c, route == FwdRoute::toeplitz);
}

// ---- forward moments for the InstanceNorm that follows a conv (jpdse_conv_fwd_moments): how many slots per image the layer's
// route writes (0: its kernel has no moment epilogue).  The route is selected with moments wanted, as the launch will select
// it.  Invariant (tests/test_host_conv_routes.py): whenever the answer is non-zero that route equals the one selected without
// moments -- asking for moments never moves a layer to another kernel, it only keeps taps4 / taps9 layers (no epilogue) at 0.
JPDSE_SWITCH(int, g_moments_fused, 1);     // 32 (and 6: the rounding-point-preserving comparison mode): no moment epilogues
static int conv_fwd_moment_slots(const jpdse_conv_desc* d, const ConvPlan& p) {
  if (!g_moments_fused || d->dtype != JPDSE_BF16 || d->act != JPDSE_ACT_NONE) return 0;
  ThinFwdGeom tg;
  switch (select_fwd(d, p, {true, false})) {
    case FwdRoute::thin_fwd: return thin_fwd_geom(d, p, &tg) ? thin_fwd_slots(p, tg) : 0;
    case FwdRoute::rows: return rows_slots(rows_band(d->N, p.OH, p.OW, p.Ks, d->stride), p.OH, p.OW, p.Ks);
    case FwdRoute::halo: return p.Cs > 64 ? halo_slots(p.OH, p.OW) : 0;      // the double-buffered form only: inputs of 128+ channels
    default: return 0;
  }
}

}  // namespace jpdse
