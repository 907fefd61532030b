// Data-gradient dispatch of the convolution family (also the forward of ConvTranspose2d): conv_dgrad_t launches the route
// select_dgrad (conv_route.h) chose, one function per route; the ConvTranspose moment-slot and norm-sum slot queries read the same
// choice.  Part of conv_gemm.hip (one translation unit).
#pragma once

namespace jpdse {

// Reflect-padded 3x3 stride-1 data gradient = zero-padded data gradient (halo kernel, written to dx)
// + the ring of the padded domain folded back: padded row -1 -> image row 1, row H -> H-2, column -1 -> 1,
// column W -> W-2.  The four ring strips are small split-K GEMMs (fp32 slabs, FastArgs::no_finish); this
// kernel sums their slabs and adds them into dx.  One thread = 8 channels of one target pixel; targets are
// enumerated without duplicates: rows {1, H-2} completely, columns {1, W-2} without those two rows.
struct RingFoldArgs {
  bf16_t* dx;
  const float* top; const float* bot; const float* left; const float* right;   // slabs [splits][M_q][Cs]
  int splits_tb, splits_lr;
  int N, H, W, Cs;
};
__device__ __forceinline__ void ring_acc(float (&acc)[8], const float* slab, int splits, long long slab_elems,
                                         long long row, int Cs, int c0) {
  // slabs are read four at a time before they are added (same order): one L2 round trip per split otherwise
  const float* base = slab + row * Cs + c0;
  int sp = 0;
  for (; sp + 4 <= splits; sp += 4) {
    float4 lo[4], hi[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float4* src = reinterpret_cast<const float4*>(base + (sp + u) * slab_elems);
      lo[u] = src[0];
      hi[u] = src[1];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      acc[0] += lo[u].x; acc[1] += lo[u].y; acc[2] += lo[u].z; acc[3] += lo[u].w;
      acc[4] += hi[u].x; acc[5] += hi[u].y; acc[6] += hi[u].z; acc[7] += hi[u].w;
    }
  }
  for (; sp < splits; ++sp) {
    const float4* src = reinterpret_cast<const float4*>(base + sp * slab_elems);
    const float4 lo = src[0], hi = src[1];
    acc[0] += lo.x; acc[1] += lo.y; acc[2] += lo.z; acc[3] += lo.w;
    acc[4] += hi.x; acc[5] += hi.y; acc[6] += hi.z; acc[7] += hi.w;
  }
}
__global__ __launch_bounds__(256) void ring_fold_kernel(const RingFoldArgs a, long long total_vec) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= total_vec) return;
  const int cv = a.Cs >> 3;
  const int c0 = (int)(v % cv) * 8;
  long long t = v / cv;
  const int per_n = 2 * a.W + 2 * (a.H - 2);
  const int n = (int)(t / per_n);
  int e = (int)(t - (long long)n * per_n);
  const long long Mtb = (long long)a.N * (a.W + 2), Mlr = (long long)a.N * a.H;
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  int i_row, j_col;
  if (e < 2 * a.W) {                      // row targets
    const bool is_top = e < a.W;
    const int j = is_top ? e : e - a.W;
    i_row = is_top ? 1 : a.H - 2;
    j_col = j;
    const float* slab = is_top ? a.top : a.bot;
    const long long rb = (long long)n * (a.W + 2);
    ring_acc(acc, slab, a.splits_tb, Mtb * a.Cs, rb + j + 1, a.Cs, c0);
    if (j == 1) ring_acc(acc, slab, a.splits_tb, Mtb * a.Cs, rb, a.Cs, c0);                  // corner b = 0
    if (j == a.W - 2) ring_acc(acc, slab, a.splits_tb, Mtb * a.Cs, rb + a.W + 1, a.Cs, c0);  // corner b = W+1
    if (j == 1) ring_acc(acc, a.left, a.splits_lr, Mlr * a.Cs, (long long)n * a.H + i_row, a.Cs, c0);
    if (j == a.W - 2) ring_acc(acc, a.right, a.splits_lr, Mlr * a.Cs, (long long)n * a.H + i_row, a.Cs, c0);
  } else {                                // column targets, rows other than 1 and H-2
    e -= 2 * a.W;
    const bool is_left = e < a.H - 2;
    int i = is_left ? e : e - (a.H - 2);  // index into the H-2 remaining rows
    i = i == 0 ? 0 : i + 1;               // rows 0, 2, 3, ..., H-3, H-1
    if (i >= a.H - 2) i += 1;
    i_row = i;
    j_col = is_left ? 1 : a.W - 2;
    ring_acc(acc, is_left ? a.left : a.right, a.splits_lr, Mlr * a.Cs, (long long)n * a.H + i, a.Cs, c0);
  }
  bf16_t* dst = a.dx + (((long long)n * a.H + i_row) * a.W + j_col) * a.Cs + c0;
  float cur[8];
  Vec16<bf16_t>::load(dst, cur);
#pragma unroll
  for (int q = 0; q < 8; ++q) cur[q] += acc[q];
  Vec16<bf16_t>::store(dst, cur);
}

// The folded frame of dy for the one-launch reflect data gradient (gemm_halo.h, VIRT): per image 2 rows of W + 2 pixels
// (above row 0 / below row H-1), then 2 columns of H pixels (left of column 0 / right of column W-1):
//   row frame t, column b-1:  dy[r0][c] + dy[r1][c] with (r0, r1) = (0, 2) | (H-3, H-1); at b = 0 and b = W+1 the corner, summed
//                             over the column pair (0, 2) | (W-3, W-1) as well
//   column frame t, row h:    dy[h][c0] + dy[h][c1]
// fp32 sums, rounded to bf16 once.  One thread = 8 channels of one frame pixel.
__global__ __launch_bounds__(256) void ring_frame_kernel(const bf16_t* __restrict__ dy, bf16_t* __restrict__ V, int N, int H, int W,
                                                         int Cs, long long total_vec) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total_vec) return;
  const int cv = Cs >> 3;
  const int c0 = (int)(t % cv) * 8;
  long long q = t / cv;
  const int per_n = 2 * (W + 2) + 2 * H;
  const int n = (int)(q / per_n);
  const int e = (int)(q - (long long)n * per_n);
  int rows[2], cols[2], nr, nc;
  if (e < 2 * (W + 2)) {
    const int top = e < W + 2, b = top ? e : e - (W + 2);
    rows[0] = top ? 0 : H - 3;
    rows[1] = top ? 2 : H - 1;
    nr = 2;
    if (b == 0) { cols[0] = 0; cols[1] = 2; nc = 2; }
    else if (b == W + 1) { cols[0] = W - 3; cols[1] = W - 1; nc = 2; }
    else { cols[0] = b - 1; cols[1] = 0; nc = 1; }
  } else {
    const int f = e - 2 * (W + 2);
    const int left = f < H;
    rows[0] = left ? f : f - H;
    rows[1] = 0;
    nr = 1;
    cols[0] = left ? 0 : W - 3;
    cols[1] = left ? 2 : W - 1;
    nc = 2;
  }
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  for (int r = 0; r < nr; ++r)
    for (int c = 0; c < nc; ++c) {
      float v[8];
      Vec16<bf16_t>::load(dy + (((long long)n * H + rows[r]) * W + cols[c]) * Cs + c0, v);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] += v[i];
    }
  Vec16<bf16_t>::store(V + ((long long)n * per_n + e) * Cs + c0, acc);
}

// dx = (dx + addend) * (mask > 0 ? 1 : slope), 16-byte vectors: the unfused form of the data-gradient epilogue
// extras (either pointer may be null); the sum is rounded to T before the slope, as the fused epilogues do
template <typename T>
__global__ void relu_mask_kernel(T* __restrict__ dx, const T* __restrict__ mask, long long total_vec,
                                 const T* __restrict__ addend = nullptr, float slope = 0.f) {
  constexpr int VE = Vec16<T>::N;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total_vec;
       i += (long long)gridDim.x * blockDim.x) {
    float v[VE], m[VE];
    Vec16<T>::load(dx + i * VE, v);
    if (addend != nullptr) {
      Vec16<T>::load(addend + i * VE, m);
#pragma unroll
      for (int e = 0; e < VE; ++e) v[e] += m[e];
    }
    if (mask != nullptr) {
      Vec16<T>::load(mask + i * VE, m);
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        const float r = sizeof(T) == 2 ? bf16_round(v[e]) : v[e];
        v[e] = m[e] > 0.f ? v[e] : (slope == 0.f ? 0.f : r * slope);
      }
    }
    Vec16<T>::store(dx + i * VE, v);
  }
}

// The InstanceNorm (+ activation) whose backward consumes this data gradient (jpdse_conv_dgrad_fused_nsums): its input, its
// (mean, rstd), its activation, and where the per-block sums of its backward go (gemm_halo.h NSUM).
struct NormSink {
  const void* x;
  const float* stats;
  float* sums;
  int act;
  float slope;
};

struct DgradCall {      // what a data-gradient route is handed
  const jpdse_conv_desc* d; const ConvPlan& p;
  const void* dy; const void* pack; void* dx; void* ws; hipStream_t s;
  const void* mask; const void* addend; float* mom; float mask_slope; const NormSink* sink;
  // batched data gradient (jpdse_conv_dgrad_batched; 0 = off): gradient images >= alias read the mask of saved image n - alias,
  // and only images < addend_n take the addend
  int alias, addend_n;
};
static void* dgrad_dxp(const DgradCall& c) { return reinterpret_cast<char*>(c.ws) + c.p.dypad_bytes; }      // dx on the reflect-padded domain

// phase 0 as the single-launch kernels see it
static ConvView dgrad_view(const DgradCall& c) {
  ConvView v = view_dgrad_phase(c.d, c.p, 0, c.dy, c.pack, c.dx);
  v.mask = reinterpret_cast<const bf16_t*>(c.mask);
  v.addend = reinterpret_cast<const bf16_t*>(c.addend);
  v.alias = c.mask != nullptr ? c.alias : 0;
  v.addend_n = c.addend != nullptr ? c.addend_n : 0;
  return v;
}
// reflect-padded 3x3: the zero-padded data gradient on the image's own grid (pad 1, straight into dx).  The mask rides in the
// one-launch (frame) forms only; the strip forms apply it after the fold.
static ConvView ring_view(const DgradCall& c) {
  ConvView r = dgrad_view(c);
  r.OH = c.d->H;
  r.OW = c.d->W;
  r.py = r.px = 1;
  r.out_base = 0;
  r.mask = nullptr;
  return r;
}

// one launch (+ the split-K finish of the nine-tap program): the ring rides in the frame of dy (gemm_halo.h / gemm_taps.h VIRT);
// the mask, if any, in the same epilogue
static int dgrad_ring_frame(const DgradCall& c, DgradRoute route) {      // ring_taps9_frame | ring_halo_frame
  const jpdse_conv_desc* d = c.d;
  const ConvPlan& p = c.p;
  const bool taps = route == DgradRoute::ring_taps9_frame;
  ConvView r = ring_view(c);
  bf16_t* frame = reinterpret_cast<bf16_t*>(c.ws);       // in front of the split-K slabs (splitk_off lies behind the padded-dy region)
  const long long fv = (long long)d->N * (2 * (d->W + 2) + 2 * d->H) * (p.Ks / 8);
  if (taps && (size_t)fv * 16 > p.splitk_off) return set_error(JPDSE_EWORKSPACE, "reflect data gradient: no room for the frame in front of the slabs");
  const int pslot = taps ? -1 : prof_begin(c.s, p.Cs, 9LL * p.Ks);
  hipLaunchKernelGGL(ring_frame_kernel, dim3(ew_blocks(fv)), dim3(256), 0, c.s, r.X, frame, d->N, d->H, d->W, p.Ks, fv);
  const int rc = check_launch("ring_frame_kernel");
  prof_end(pslot, 1, 0.0, c.s);
  if (rc) return rc;
  r.frame = frame;
  r.mask = reinterpret_cast<const bf16_t*>(c.mask);
  if (taps) return launch_taps9(r, splitk_slabs(p, c.ws), c.s);
  HaloArgs h = to_halo(r);
  if (c.sink != nullptr) {
    h.nx = reinterpret_cast<const bf16_t*>(c.sink->x);
    h.nstats = c.sink->stats;
    h.nsums = c.sink->sums;
    h.nact = c.sink->act;
    h.nslope = c.sink->slope;
    h.mom_slots = halo_slots(d->H, d->W);
  }
  return p.Cs > 64 ? launch_halo_cfg<2>(h, c.s) : launch_halo_cfg<1>(h, c.s);
}

// (1) the zero-padded data gradient, (2) the four ring strips of the reflect-padded domain as split-K GEMMs into fp32 slabs,
// (3) ring_fold_kernel, (4) the mask
static int dgrad_ring_strips(const DgradCall& c, DgradRoute route) {      // ring_taps9_strips | ring_halo_strips
  const jpdse_conv_desc* d = c.d;
  const ConvPlan& p = c.p;
  hipStream_t s = c.s;
  const ConvView r = ring_view(c);
  if (route == DgradRoute::ring_taps9_strips) {
    if (int rc = launch_taps9(r, splitk_slabs(p, c.ws), s)) return rc;
  } else if (int rc = p.Cs > 64 ? launch_halo_cfg<2>(to_halo(r), s) : launch_halo_cfg<1>(to_halo(r), s)) return rc;
  const int H = d->H, W = d->W, Ks = p.Ks, Lk = p.ph[0].Lk;
  const bf16_t* dyb = reinterpret_cast<const bf16_t*>(c.dy);
  const bf16_t* pk = reinterpret_cast<const bf16_t*>(c.pack);
  const int Mtb = d->N * (W + 2), Mlr = d->N * H;
  const int nt = (p.Cs + 127) / 128;
  // the strips have few rows (N (W + 2) and N H); 128-row tiles (two blocks per CU) measured slower (round-2 mode 31, retired)
  const int bm = 256;
  const int tiles = 2 * ((Mtb + bm - 1) / bm) * nt + 2 * ((Mlr + bm - 1) / bm) * nt;
  const int kt = 3 * Ks / 64;
  int sp = 256 / tiles;
  if (sp > kt / 8) sp = kt / 8;
  if (sp > 8) sp = 8;
  if (sp < 1) sp = 1;
  float* slab = reinterpret_cast<float*>(c.ws);
  const size_t tb_elems = (size_t)sp * Mtb * p.Cs, lr_elems = (size_t)sp * Mlr * p.Cs;
  FastBatch rb = {};
  rb.small_m = 0;
  for (int q = 0; q < 4; ++q) {
    FastArgs g = {};
    const bool row_strip = q < 2;         // 0 top, 1 bottom, 2 left, 3 right
    g.X = dyb + (q == 1 ? (long long)(H - 1) * W * Ks : (q == 3 ? (long long)(W - 1) * Ks : 0));
    g.x_sn = (long long)H * W * Ks;
    g.x_sh = (long long)W * Ks;
    g.x_extent = (long long)d->N * H * W * Ks - (g.X - dyb);
    g.IH = row_strip ? 1 : H;
    g.IW = row_strip ? W : 1;
    g.Cs = Ks;
    g.R = row_strip ? 1 : 3;
    g.S = row_strip ? 3 : 1;
    g.sy = g.sx = 1;
    g.py = row_strip ? 0 : 1;
    g.px = row_strip ? 2 : 0;
    g.OH = row_strip ? 1 : H;
    g.OW = row_strip ? W + 2 : 1;
    g.M = row_strip ? Mtb : Mlr;
    // panel [c][u'][w'][k] with u' = 2 - r, w' = 2 - s: top r=0 -> u'=2, bottom u'=0, left s=0 -> w'=2, right w'=0
    g.B = pk + (q == 0 ? 2LL * Lk : (q == 2 ? 2LL * Ks : 0));
    g.b_stride = 3LL * Lk;
    g.b_tap_r = Lk;
    g.b_tap_s = Ks;
    g.Kout = d->C;
    g.Ks = p.Cs;
    g.b_rows = p.Cs;
    g.act = JPDSE_ACT_NONE;
    g.splits = sp;
    g.no_finish = 1;
    g.partial = slab + (q == 0 ? 0 : (q == 1 ? tb_elems : (q == 2 ? 2 * tb_elems : 2 * tb_elems + lr_elems)));
    rb.p[rb.n++] = g;
  }
  const int pslot = prof_begin(s, p.Cs, 9LL * p.Ks);
  if (int rc = launch_fast_batch(rb, s)) return rc;
  // fold the ring into rows 1 / H-2 and columns 1 / W-2 of dx
  RingFoldArgs rf = {};
  rf.dx = reinterpret_cast<bf16_t*>(c.dx);
  rf.top = rb.p[0].partial;
  rf.bot = rb.p[1].partial;
  rf.left = rb.p[2].partial;
  rf.right = rb.p[3].partial;
  rf.splits_tb = rf.splits_lr = sp;
  rf.N = d->N;
  rf.H = H;
  rf.W = W;
  rf.Cs = p.Cs;
  const long long tv = (long long)d->N * (2 * W + 2 * (H - 2)) * (p.Cs / 8);
  hipLaunchKernelGGL(ring_fold_kernel, dim3(ew_blocks(tv)), dim3(256), 0, s, rf, tv);
  int rc = check_launch("ring_fold_kernel");
  if (rc == JPDSE_OK && c.mask != nullptr) {
    const long long total_vec = (long long)d->N * H * W * (p.Cs / 8);
    hipLaunchKernelGGL((relu_mask_kernel<bf16_t>), dim3(ew_blocks(total_vec)), dim3(256), 0, s, reinterpret_cast<bf16_t*>(c.dx),
                       reinterpret_cast<const bf16_t*>(c.mask), total_vec);
    rc = check_launch("relu_mask_kernel");
  }
  prof_end(pslot, 1, 0.0, s);
  return rc;
}

static int dgrad_head(const DgradCall& c) {
  const jpdse_conv_desc* d = c.d;
  const ConvPlan& p = c.p;
  HeadFwdArgs h = {};
  h.X = reinterpret_cast<const bf16_t*>(c.dy);
  h.Wp = reinterpret_cast<const bf16_t*>(c.pack);
  h.Y = reinterpret_cast<bf16_t*>(c.dx);
  h.N = d->N; h.H = p.OH; h.W = p.OW; h.OH = d->H; h.OW = d->W;
  h.K = d->C; h.Ks_out = p.Cs;
  h.R = h.S = 3;
  h.pad = 1;
  h.act = JPDSE_ACT_NONE;
  h.tiles_w = (d->W + 63) / 64;
  h.tiles_h = (d->H + kHeadTH - 1) / kHeadTH;
  if (head_rows_ok(64, h.R, h.K, h.Ks_out, h.H, h.W, h.OH, h.OW)) return launch_head_rows<3>(h, c.s);
  return launch_head_fwd<64, 3, 3, 3>(h, c.s);
}

// the two all-phases row-streaming kernels: DY, the four phase panels, DX and the sizes both argument structs name alike
template <typename Args>
static Args phases_rows_args(const DgradCall& c) {
  Args g = {};
  g.DY = reinterpret_cast<const bf16_t*>(c.dy);
  for (int i = 0; i < 4; ++i) g.P[i] = reinterpret_cast<const bf16_t*>(reinterpret_cast<const char*>(c.pack) + c.p.ph[i].pack_off);
  g.DX = reinterpret_cast<bf16_t*>(c.dx);
  g.N = c.d->N; g.OH = c.p.OH; g.OW = c.p.OW;
  return g;
}
static int dgrad_dgrad2_rows(const DgradCall& c) {
  Dgrad2Args g = phases_rows_args<Dgrad2Args>(c);
  g.mom = c.mom;
  return launch_dgrad2_rows(g, c.s);
}
static int dgrad_thin_dgrad2_rows(const DgradCall& c) {
  ThinDgrad2Args g = phases_rows_args<ThinDgrad2Args>(c);
  g.H = c.d->H; g.W = c.d->W; g.K = c.d->C;
  return launch_thin_dgrad2_rows(g, c.s);
}

static int dgrad_thin_in_rows(const DgradCall& c) {
  ThinInArgs g = {};
  g.DY = reinterpret_cast<const bf16_t*>(c.dy);
  g.P = reinterpret_cast<const bf16_t*>(reinterpret_cast<const char*>(c.pack) + c.p.ph[0].pack_off);
  g.DX = reinterpret_cast<bf16_t*>(c.dx);
  g.DXP = reinterpret_cast<bf16_t*>(dgrad_dxp(c));
  g.N = c.d->N; g.H = c.d->H; g.W = c.d->W; g.OH = c.d->H + 6; g.OW = c.d->W + 6;
  g.py = g.px = 6;
  g.act = JPDSE_ACT_NONE;
  return launch_thin_in_rows<7, true>(g, c.s);
}

static int dgrad_thin1(const DgradCall& c) {      // dx is written once by an FMA kernel (thin_out1.h)
  const Phase& f = c.p.ph[0];
  Thin1DgradArgs t = {};
  t.DY = reinterpret_cast<const bf16_t*>(c.dy);
  t.B = reinterpret_cast<const bf16_t*>(reinterpret_cast<const char*>(c.pack) + f.pack_off);
  t.taps = reinterpret_cast<float*>(c.ws);        // 16 x Cs floats: inside the padded-dy region of every plan
  t.DX = reinterpret_cast<bf16_t*>(c.dx);
  t.addend = reinterpret_cast<const bf16_t*>(c.addend);
  t.addend_n = c.addend_n;
  t.N = c.d->N; t.H = c.d->H; t.W = c.d->W; t.Cs = c.p.Cs; t.OH = c.p.OH; t.OW = c.p.OW;
  t.py = (f.Uh - 1) - f.i0h;
  t.px = (f.Uw - 1) - f.i0w;
  t.Lk = f.Lk;
  t.b_stride = (long long)f.Uh * f.Lk;
  return launch_thin1_dgrad(t, c.s);
}

// where stride phase f of the phase loops writes: every stride-th pixel of dx, or (reflect) of dx on the padded domain
template <typename Args>
static void phase_out(Args* a, const DgradCall& c, const Phase& f) {
  const jpdse_conv_desc* d = c.d;
  const ConvPlan& p = c.p;
  const bool refl = d->pad_mode == JPDSE_PAD_REFLECT;
  const int st = d->stride, H = refl ? p.Hp : d->H, W = refl ? p.Wp : d->W, off = refl ? 0 : d->pad;
  a->Y = reinterpret_cast<decltype(a->Y)>(refl ? dgrad_dxp(c) : c.dx);
  a->out_sn = (long long)H * W * p.Cs;
  a->out_sh = (long long)st * W * p.Cs;
  a->out_sw = (long long)st * p.Cs;
  a->out_base = ((long long)(st * f.i0h + f.qh - off) * W + (st * f.i0w + f.qw - off)) * p.Cs;
}
// behind the phase loops: the fold of the padded domain (reflect), then the fused operands no epilogue has applied
template <typename T>
static int dgrad_finish(const DgradCall& c, bool in_epilogue) {
  const jpdse_conv_desc* d = c.d;
  const long long total_vec = (long long)d->N * d->H * d->W * (c.p.Cs / (16 / (int)sizeof(T)));
  int rc = JPDSE_OK;
  if (d->pad_mode == JPDSE_PAD_REFLECT) {
    hipLaunchKernelGGL((reflect_fold_kernel<T>), dim3(ew_blocks(total_vec)), dim3(256), 0, c.s, reinterpret_cast<const T*>(dgrad_dxp(c)),
                       reinterpret_cast<T*>(c.dx), d->N, d->H, d->W, c.p.Cs, d->pad, total_vec);
    rc = check_launch("reflect_fold_kernel");
  }
  if (rc == JPDSE_OK && (c.mask != nullptr || c.addend != nullptr) && !in_epilogue) {
    // one pass per run of images that share their operands: a batched call cuts at addend_n and at alias
    const int cuts[4] = {0, c.addend != nullptr ? c.addend_n : 0, c.mask != nullptr ? c.alias : 0, d->N};
    const long long img = (long long)d->H * d->W * c.p.Cs, img_vec = total_vec / d->N;
    for (int n0 = 0; n0 < d->N && rc == JPDSE_OK;) {
      int n1 = d->N;
      for (int q = 1; q < 3; ++q) if (cuts[q] > n0 && cuts[q] < n1) n1 = cuts[q];
      const T* addend = c.addend != nullptr && (c.addend_n == 0 || n0 < c.addend_n) ? reinterpret_cast<const T*>(c.addend) + n0 * img : nullptr;
      const T* mask = c.mask != nullptr ? reinterpret_cast<const T*>(c.mask) + (n0 >= c.alias ? n0 - c.alias : n0) * img : nullptr;
      if (addend != nullptr || mask != nullptr) {
        const long long nvec = (n1 - n0) * img_vec;
        hipLaunchKernelGGL((relu_mask_kernel<T>), dim3(ew_blocks(nvec)), dim3(256), 0, c.s, reinterpret_cast<T*>(c.dx) + n0 * img, mask, nvec,
                           addend, c.mask_slope);
        rc = check_launch("relu_mask_kernel");
      }
      n0 = n1;
    }
  }
  return rc;
}

// all stride phases in ONE launch of the fast kernel; the fused operands ride in its epilogue unless the padded domain is folded first
static int dgrad_fast(const DgradCall& c) {
  const jpdse_conv_desc* d = c.d;
  const ConvPlan& p = c.p;
  const bool refl = d->pad_mode == JPDSE_PAD_REFLECT;
  const int nlive = live_phases(p);
  FastBatch batch = {};
  for (int i = 0; i < p.nph; ++i) {
    const Phase& f = p.ph[i];
    if (f.cnth <= 0 || f.cntw <= 0) continue;
    FastArgs g = to_fast(view_dgrad_phase(d, p, i, c.dy, c.pack, c.dx));
    phase_out(&g, c, f);
    if (!refl) {
      g.mask = reinterpret_cast<const bf16_t*>(c.mask);
      g.addend = reinterpret_cast<const bf16_t*>(c.addend);
      g.alias = c.mask != nullptr ? c.alias : 0;
      g.addend_n = c.addend != nullptr ? c.addend_n : 0;
    }
    g.mask_slope = c.mask_slope;
    g.splits = nlive == 1 ? splitk_for(g.M, p.Cs, f.Uh * f.Uw * p.Ks / 64) : 1;
    g.partial = splitk_slabs(p, c.ws);
    if ((g.alias != 0 || g.addend_n != 0) && g.splits <= 1) {
      // a batched call whose fused operands ride in the kernel's own epilogue: every run of images with the same operands is a
      // problem of its own (same tiles' arithmetic per row; a tile never spans two runs), addressed by base pointers
      const int cuts[2] = {g.addend_n, g.alias};
      const long long x_img = (long long)g.IH * g.IW * g.Cs;
      for (int n0 = 0; n0 < d->N;) {
        int n1 = d->N;
        for (int q = 0; q < 2; ++q) if (cuts[q] > n0 && cuts[q] < n1) n1 = cuts[q];
        if (batch.n >= kFastBatchMax) return set_error(JPDSE_EINVAL, "conv_dgrad_batched: more than %d problems in one launch", kFastBatchMax);
        FastArgs r = g;
        r.alias = r.addend_n = 0;
        r.X = g.X + n0 * x_img;
        r.Y = g.Y + n0 * g.out_sn;
        r.M = (n1 - n0) * g.OH * g.OW;
        r.addend = g.addend != nullptr && (g.addend_n == 0 || n0 < g.addend_n) ? g.addend + n0 * g.out_sn : nullptr;
        r.mask = g.mask != nullptr ? g.mask + (long long)(n0 >= g.alias ? n0 - g.alias : n0) * g.out_sn : nullptr;
        batch.p[batch.n++] = r;
        n0 = n1;
      }
      continue;
    }
    batch.p[batch.n++] = g;
  }
  if (int rc = launch_fast_batch(batch, c.s)) return rc;
  return dgrad_finish<bf16_t>(c, !refl);
}

// one launch of the generic GEMM per stride phase over the zero-padded copy of dy
template <typename T>
static int dgrad_generic(const DgradCall& c) {
  const jpdse_conv_desc* d = c.d;
  const ConvPlan& p = c.p;
  if (int rc = launch_pad<T>(c.dy, c.ws, d->N, p.OH, p.OW, p.Ks, p.PT, p.PB, p.PL, p.PR, JPDSE_PAD_ZERO, c.s)) return rc;
  for (int i = 0; i < p.nph; ++i) {
    const Phase& f = p.ph[i];
    if (f.cnth <= 0 || f.cntw <= 0) continue;
    GemmFwdArgs a = {};
    a.A = c.ws;
    a.B = reinterpret_cast<const char*>(c.pack) + f.pack_off;
    a.M = d->N * f.cnth * f.cntw; a.OH = f.cnth; a.OW = f.cntw;
    a.Kout = d->C; a.Ks = a.b_rows = p.Cs;
    a.R = f.Uh; a.cpr = f.Lk / p.BKE; a.b_row_stride = (long long)f.Uh * f.Lk;
    a.in_sn = (long long)p.DH * p.DW * p.Ks; a.in_sh = a.in_sr = (long long)p.DW * p.Ks; a.in_sw = p.Ks;
    a.in_base = ((long long)(f.i0h + p.PT - (f.Uh - 1)) * p.DW + (f.i0w + p.PL - (f.Uw - 1))) * p.Ks;
    phase_out(&a, c, f);
    a.act = JPDSE_ACT_NONE;
    a.partial = splitk_slabs(p, c.ws);     // split-K slabs, reused by the phases (stream order)
    a.partial_cap = p.splitk_bytes;
    if (int rc = launch_fwd<T>(a, c.s)) return rc;
  }
  return dgrad_finish<T>(c, false);
}

// moment slots per image of the ConvTranspose2d forward (jpdse_convT_fwd_moments): dgrad2_rows is the route with that epilogue
static int convT_fwd_moment_slots(const jpdse_conv_desc* d, const ConvPlan& p) {
  if (!g_moments_fused || select_dgrad(d, p, {false, false, false, true, false}) != DgradRoute::dgrad2_rows) return 0;
  return dgrad2_rows_slots(dgrad2_rows_band(d->N, p.OH, p.OW), p.OH, p.OW);
}
// blocks per image whose norm-backward sums the data gradient of this layer writes (0: its kernel has no such epilogue): the
// folded-frame halo route with 128-channel output tiles (gemm_halo.h NSUM: the double-buffered form, a dense dx) -- the ResnetBlock convs
static int dgrad_nsum_slots(const jpdse_conv_desc* d, const ConvPlan& p) {
  if (select_dgrad(d, p, {false, false, false, false, true}) != DgradRoute::ring_halo_frame) return 0;
  return p.Ks >= 128 && p.Cs % 128 == 0 && d->C == p.Cs ? halo_slots(d->H, d->W) : 0;
}

template <typename T>
static int conv_dgrad_t(const jpdse_conv_desc* d, const ConvPlan& p, const void* dy, const void* pack, void* dx,
                        void* ws, hipStream_t s, const void* mask = nullptr, const void* addend = nullptr, float* mom = nullptr,
                        float mask_slope = 0.f, const NormSink* sink = nullptr, int alias = 0, int addend_n = 0) {
  // LeakyReLU-backward epilogue (mask_slope != 0): only the fast / generic tile kernels and the unfused pass apply it
  const bool lrelu = mask != nullptr && mask_slope != 0.f;
  if (sink != nullptr && (dgrad_nsum_slots(d, p) == 0 || lrelu))
    return set_error(JPDSE_EINVAL, "conv_dgrad: this layer's data-gradient kernel writes no norm-backward sums (jpdse_conv_dgrad_nsum_slots == 0)");
  const DgradCall c = {d, p, dy, pack, dx, ws, s, mask, addend, mom, mask_slope, sink, alias, addend_n};
  const DgradRoute route = select_dgrad(d, p, {mask != nullptr, addend != nullptr, lrelu, mom != nullptr, sink != nullptr});
  // a batched call: only the routes of the PatchGAN layers resolve the image classes (gemm_fast.h, gemm_taps.h 4x4, thin_out1.h,
  // and the unfused pass behind the generic GEMM)
  if ((alias != 0 || addend_n != 0) && route != DgradRoute::fast && route != DgradRoute::taps4 && route != DgradRoute::thin1 &&
      route != DgradRoute::generic)
    return set_error(JPDSE_EINVAL, "conv_dgrad_batched: this layer's data-gradient kernel does not take a batched call");
  if constexpr (sizeof(T) == 2) {      // (the bf16 kernels are not instantiated for fp32 layers, which select_dgrad sends to the generic GEMM)
    switch (route) {
      case DgradRoute::rows: return launch_rows(to_rows(dgrad_view(c)), 1, s);
      case DgradRoute::halo: return p.Cs > 64 ? launch_halo_cfg<2>(to_halo(dgrad_view(c)), s) : launch_halo_cfg<1>(to_halo(dgrad_view(c)), s);
      case DgradRoute::taps9: return launch_taps9(dgrad_view(c), splitk_slabs(p, ws), s);
      case DgradRoute::ring_taps9_frame:
      case DgradRoute::ring_halo_frame: return dgrad_ring_frame(c, route);
      case DgradRoute::ring_taps9_strips:
      case DgradRoute::ring_halo_strips: return dgrad_ring_strips(c, route);
      case DgradRoute::head: return dgrad_head(c);
      case DgradRoute::dgrad2_rows: return dgrad_dgrad2_rows(c);
      case DgradRoute::thin_dgrad2_rows: return dgrad_thin_dgrad2_rows(c);
      case DgradRoute::thin_in_rows: return dgrad_thin_in_rows(c);
      case DgradRoute::taps_dgrad2: return launch_taps_dgrad2(d, p, dy, pack, dx, s, mask, addend, mask_slope);
      case DgradRoute::taps4: return launch_taps4(dgrad_view(c), ws, s);
      case DgradRoute::thin1: return dgrad_thin1(c);
      case DgradRoute::fast: return dgrad_fast(c);
      default: break;
    }
  }
  return dgrad_generic<T>(c);
}

}  // namespace jpdse
