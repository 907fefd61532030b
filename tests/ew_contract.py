"""Per-kernel contracts of csrc/elementwise.hip: pooling, activation backward, add, channel sum / copy / concat, layout
conversion, the L1 / MSE / MSE-const losses, the quantised evaluation loss, the fp32 <-> bf16 casts and the multi-tensor Adam.

Three kinds of expectation; each kernel gets the strongest one its arithmetic allows.

  bit-exact    one possible rounding sequence: emulated in torch fp32 on the CPU, compared on the stored bits
               (maxpool2 fwd / bwd, channel_copy, concat_channels, insert_channels, both layout conversions, cast, copy, add,
               act_bwd for ReLU / LeakyReLU / none, l1_bwd, l1_bwd_relu, the gradient of l1_fwd_bwd, mse_bwd, mse_const_bwd)
  candidates   device code is built without -ffp-contract=off, so a multiply-add may or may not be fused: the fused and the
               unfused rounding sequence are computed from fp64; an element passes if it equals one of them, otherwise it
               must lie within one ulp (of the storage type) of the fp64 result, and the share of such elements is capped
               (act_bwd for tanh, avgpool3s2 fwd / bwd; Adam is held to fp64 within k u (|value| + |update terms|))
  reductions   integer-valued operands (every fp32 sum exact in any order): the result must equal the integer sum bit for bit;
               randn operands with a non-zero mean: within D u sum|terms| of fp64, D the longest chain of fp32 additions
               (channel_sum, l1_fwd, mse_fwd, mse_const_fwd, the value of l1_fwd_bwd; quant_loss: integer-exact in double)

Everything here works on NHWC storage tensors [N, H, W, Cs] (Cs = C rounded up to 8) held as fp32 CPU tensors whose values are
representable in the storage type.  The emulations take an optional `defect`; tests/test_ew_contract_host.py plants each one and
checks that the criterion meant to catch it does.  Plain torch-CPU: no GPU is needed.
"""
import numpy as np
import torch

import jpdse_hip
from jpdse_hip import F32, BF16, ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH
from bf16_contract import rn_bf16, ulp_bf16, U, CAP
from hip_util import record

VE = {F32: 4, BF16: 8}          # elements of a 16-byte vector
EW_BLOCKS = 2048                # ew_blocks (common.h): grid cap of the grid-stride kernels, blocks of 256
EW_CAP = EW_BLOCKS * 256        # work items of one grid-stride sweep
RED_BLOCKS = 1024               # kRedBlocks: cap of the loss first stage
EXACT_LIMIT = 2 ** 24           # integers below it are exact in fp32
SLOPE = 0.2


def cpad(c):
  return (c + 7) & ~7


def tdtype(dtype):
  return torch.bfloat16 if dtype == BF16 else torch.float32


def st(t, dtype):
  """What the store of the fp32 value t leaves in memory (one RNE to the storage type), as fp32."""
  return t.to(torch.bfloat16).float() if dtype == BF16 else t


def f32(v):
  return torch.tensor(float(v), dtype=torch.float32)


def rn32(t64):
  """fp64 -> fp32 round-to-nearest-even, returned as fp64."""
  return t64.float().double()


def store64(t64, dtype):
  """fp64 holding fp32 values -> the stored value, as fp64."""
  return rn_bf16(t64) if dtype == BF16 else t64


def ulp_f32(v):
  v = torch.as_tensor(v, dtype=torch.float64).abs()
  _, e = torch.frexp(v)
  u = torch.ldexp(torch.ones_like(v), (e - 24).to(torch.float64))
  return torch.where(v < 2.0 ** -126, torch.full_like(v, 2.0 ** -149), u)


def ulp_of(v, dtype):
  return ulp_bf16(v) if dtype == BF16 else ulp_f32(v)


def pad_lanes(x, C):
  """[N, H, W, C] -> [N, H, W, Cs] with zero padding lanes."""
  out = torch.zeros(x.shape[:3] + (cpad(C),), dtype=x.dtype)
  out[..., :C] = x
  return out


def grid_stride_sweeps(work_items):
  return -(-work_items // EW_CAP)


# ---- criterion 1: bit-exact -----------------------------------------------------------------------------------------------------
def bits(t):
  t = t.contiguous()
  return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def bits_differ(got, want, dtype=None):
  """Number of elements whose stored bits differ.  `got`: a tensor of the storage type (or fp32 holding its values),
  `want`: the fp32 emulation; both are taken to `dtype`'s storage type (exact) before the comparison."""
  td = tdtype(dtype) if dtype is not None else got.dtype
  got, want = got.detach().cpu().to(td), want.detach().cpu().to(td)
  assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
  return int((bits(got) != bits(want)).sum())


def assert_bits_equal(got, want, what, dtype=None):
  n = bits_differ(got, want, dtype)
  record(what + ' [bit-exact: elements that differ]', n, 0.0)
  if n:
    td = tdtype(dtype) if dtype is not None else got.dtype
    g, w = got.detach().cpu().to(td), want.detach().cpu().to(td)
    bad = torch.nonzero(bits(g) != bits(w))
    i = tuple(bad[0].tolist())
    raise AssertionError('%s: %d of %d elements differ in their stored bits; first %s: got %r, want %r; last %s'
                         % (what, n, g.numel(), list(i), float(g[i]), float(w[i]), bad[-1].tolist()))


def assert_pad_zero(t, C, what):
  """The padding lanes C..Cs of an NHWC tensor are still zero."""
  if t.shape[-1] > C:
    n = int((t[..., C:] != 0).sum())
    record(what + ' [padding lanes not zero]', n, 0.0)
    assert n == 0, '%s: %d padding-lane elements are not zero' % (what, n)


# ---- criterion 2: candidates ----------------------------------------------------------------------------------------------------
def candidate_figures(got, cands, exact64, dtype):
  """(worst distance of an element that equals no candidate from the fp64 result, in ulps of the storage type at that result;
  share of the elements that equal no candidate)."""
  got = got.detach().cpu().double()
  hit = torch.zeros(got.shape, dtype=torch.bool)
  for c in cands:
    hit |= got == c
  off = ~hit
  if not bool(off.any()):
    return 0.0, 0.0
  d = ((got - exact64).abs() / ulp_of(exact64, dtype))[off]
  d = torch.nan_to_num(d, nan=float('inf'))
  return d.max().item(), off.double().mean().item()


def assert_candidates(got, cands, exact64, dtype, what, cap=CAP):
  worst, share = candidate_figures(got, cands, exact64, dtype)
  record(what + ' [candidates: worst non-candidate, ulps of the fp64 result]', worst, 1.0)
  record(what + ' [candidates: share that equals no candidate]', share, cap)
  assert worst <= 1.0, '%s: an element that equals no candidate lies %.3g ulps from the fp64 result' % (what, worst)
  assert share <= cap, '%s: %.4f %% of the elements equal no candidate (cap %.1f %%)' % (what, 100 * share, 100 * cap)


# ---- criterion 3: reductions ----------------------------------------------------------------------------------------------------
def assert_exact_terms(terms, what):
  """The integer-valued terms of a reduction: integers, and their absolute sum below 2^24, so that every partial sum of every
  summation order is exact in fp32.  Checked on the CPU before any device work."""
  t = torch.as_tensor(terms, dtype=torch.float64)
  assert bool((t == t.round()).all()), what + ': terms are not integers'
  total = t.abs().sum().item()
  assert total < EXACT_LIMIT, '%s: sum|terms| = %d is not below 2^24' % (what, total)


def loss_value_exact(total, count):
  """fl32(total * fl32(1 / float(count))) for an integer total below 2^24: what the final stage must store."""
  assert abs(total) < EXACT_LIMIT
  return np.float32(total) * (np.float32(1.0) / np.float32(count))


def reduction_used(got, ref64, sum_abs, D):
  """|got - ref64| as a share of D u sum|terms| (worst element)."""
  got = torch.as_tensor(got).detach().cpu().double()
  ref64 = torch.as_tensor(ref64, dtype=torch.float64)
  bound = D * U * torch.as_tensor(sum_abs, dtype=torch.float64)
  return ((got - ref64).abs() / bound.clamp_min(1e-300)).max().item()


def assert_reduction(got, ref64, sum_abs, D, what):
  used = reduction_used(got, ref64, sum_abs, D)
  record(what + ' [reduction: |err| / (D u sum|terms|), D = %d]' % D, used, 1.0)
  assert used <= 1.0, '%s: error is %.3g x the bound D u sum|terms| (D = %d)' % (what, used, D)


# ---- maps: emulations -----------------------------------------------------------------------------------------------------------
def plant_map_defect(out, dtype, defect, fill=7.0, items=None):
  """A grid-stride map that leaves part of its output unwritten: the elements keep `fill`.  out: the emulated output, whose flat
  order is the order of the kernel's work items (`items` of them, default: 16-byte vectors)."""
  flat = out.clone().reshape(-1)
  n = items if items is not None else flat.numel() // VE[dtype]
  per = flat.numel() // n
  if defect == 'drop_last_vector':
    flat[(n - 1) * per:] = fill
  elif defect == 'skip_second_sweep':
    flat[EW_CAP * per:2 * EW_CAP * per] = fill
  else:
    raise ValueError(defect)
  return flat.reshape(out.shape)


def emu_add(a, b, dtype):
  return st(a + b, dtype)


def emu_act_bwd(y, dy, act, dtype, slope=SLOPE, defect=None):
  """ReLU / LeakyReLU / none: dz = dy * d in fp32 (one multiply), one RNE to the storage type.  The sign of a zero follows."""
  pos = (y >= 0) if defect == 'mask_ge' else (y > 0)
  one = torch.ones_like(y)
  if act == ACT_RELU:
    d = torch.where(pos, one, torch.zeros_like(y))
  elif act == ACT_LRELU:
    d = torch.where(pos, one, one * f32(slope))
  elif act == ACT_NONE:
    d = one
  else:
    raise ValueError('tanh has candidates: tanh_bwd_candidates')
  return st(dy * d, dtype)


def tanh_bwd_candidates(y, dy, dtype):
  """dz = dy * (1 - y*y): (candidates, fp64 result).  Fused: 1 - y*y rounded once (v_fma); unfused: y*y rounded first."""
  y64, g64 = y.double(), dy.double()
  sq = y64 * y64                                                     # exact in fp64 (24 + 24 bits)
  cands = [store64(rn32(g64 * rn32(1.0 - sq)), dtype), store64(rn32(g64 * rn32(1.0 - rn32(sq))), dtype)]
  return cands, g64 * (1.0 - sq)


def win_count(o, L):
  lo, hi = 2 * o - 1, 2 * o + 1
  return (torch.clamp(hi, max=L - 1) - torch.clamp(lo, min=0) + 1)


def avgpool_counts(H, W):
  OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
  return (win_count(torch.arange(OH), H).view(OH, 1) * win_count(torch.arange(OW), W).view(1, OW)).float()


def emu_avgpool_fwd(x, dtype, defect=None):
  """avgpool3s2 forward (3x3, stride 2, pad 1, count_include_pad = False): the valid taps summed in fp32 in tap order
  (r, then s), times 1 / cnt (fp32 division), one RNE.  An add followed by a multiply cannot be fused: one candidate.
  Returns (candidates, fp64 result)."""
  N, H, W, Cs = x.shape
  OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
  xp = torch.zeros((N, 2 * OH + 1, 2 * OW + 1, Cs), dtype=torch.float32)
  xp[:, 1:H + 1, 1:W + 1] = x                                        # a tap outside the image adds +0: no change
  acc = torch.zeros((N, OH, OW, Cs), dtype=torch.float32)
  acc64 = torch.zeros((N, OH, OW, Cs), dtype=torch.float64)
  for r in range(3):
    for s in range(3):
      v = xp[:, r:r + 2 * OH:2, s:s + 2 * OW:2][:, :OH, :OW]
      acc = acc + v
      acc64 = acc64 + v.double()
  cnt = avgpool_counts(H, W).view(1, OH, OW, 1)
  if defect == 'divisor_9':
    cnt = torch.full_like(cnt, 9.0)
  inv = torch.ones_like(cnt) / cnt
  return [st(acc * inv, dtype).double()], acc64 / avgpool_counts(H, W).view(1, OH, OW, 1).double()


def emu_avgpool_bwd(dy, H, W, dtype, defect=None):
  """avgpool3s2 backward: dx[ih][iw] = sum over the (at most 2 x 2) windows that hold the pixel, oh then ow ascending, of
  dy * inv, inv = 1 / cnt in fp32; `acc += v * inv` fused (fma) or not.  Returns (candidates, fp64 result)."""
  N, OH, OW, Cs = dy.shape
  cnt = avgpool_counts(H, W)
  if defect == 'divisor_9':
    cnt = torch.full_like(cnt, 9.0)
  inv = (torch.ones_like(cnt) / cnt).double()
  inv_true = 1.0 / avgpool_counts(H, W).double()
  ih, iw = torch.arange(H), torch.arange(W)
  d64 = dy.double()
  fused = torch.zeros((N, H, W, Cs), dtype=torch.float64)
  unfused = torch.zeros_like(fused)
  exact = torch.zeros_like(fused)
  for a in range(2):
    oh = (ih + a) // 2
    vh = ((ih % 2 == 1) | (a == 0)) & (oh < OH)
    for b in range(2):
      ow = (iw + b) // 2
      vw = ((iw % 2 == 1) | (b == 0)) & (ow < OW)
      ohc, owc = oh.clamp(max=OH - 1), ow.clamp(max=OW - 1)
      v = d64[:, ohc][:, :, owc]
      i = inv[ohc][:, owc].view(1, H, W, 1)
      it = inv_true[ohc][:, owc].view(1, H, W, 1)
      ok = (vh.view(H, 1) & vw.view(1, W)).view(1, H, W, 1)
      fused = torch.where(ok, rn32(fused + v * i), fused)            # v * i is exact in fp64
      unfused = torch.where(ok, rn32(unfused + rn32(v * i)), unfused)
      exact = torch.where(ok, exact + v * it, exact)
  return [store64(fused, dtype), store64(unfused, dtype)], exact


def emu_maxpool_fwd(x):
  N, H, W, Cs = x.shape
  OH, OW = H // 2, W // 2
  w = [x[:, i:2 * OH:2, j:2 * OW:2] for i in range(2) for j in range(2)]
  return torch.maximum(torch.maximum(w[0], w[1]), torch.maximum(w[2], w[3]))


def emu_maxpool_bwd(x, dy, defect=None):
  """The gradient goes to the FIRST maximal element of each window in row-major order; rows / columns past 2*OH, 2*OW get 0."""
  N, H, W, Cs = x.shape
  OH, OW = H // 2, W // 2
  w = [x[:, i:2 * OH:2, j:2 * OW:2] for i in range(2) for j in range(2)]
  best = torch.zeros(w[0].shape, dtype=torch.int64)
  bv = w[0]
  for k in range(1, 4):
    take = (w[k] >= bv) if defect == 'last_max' else (w[k] > bv)
    best = torch.where(take, torch.full_like(best, k), best)
    bv = torch.where(take, w[k], bv)
  dx = torch.zeros_like(x)
  for k in range(4):
    dx[:, (k >> 1):2 * OH:2, (k & 1):2 * OW:2] = torch.where(best == k, dy, torch.zeros_like(dy))
  return dx


def emu_concat_channels(base, img, c0, nch):
  out = base.clone()
  out[..., c0:c0 + nch] = img[..., :nch]
  return out


def emu_nchw_to_nhwc(src, dtype):
  return pad_lanes(st(src, dtype).permute(0, 2, 3, 1), src.shape[1])


def emu_nhwc_to_nchw(x, C):
  return x[..., :C].permute(0, 3, 1, 2).contiguous()


# ---- losses: gradients (bit-exact) --------------------------------------------------------------------------------------------
def loss_gscale(gout, scale, count):
  """g = gout * (scale / float(count)), evaluated in fp32 in that order (host: scale / (float)count; kernel: gout[0] * that)."""
  return f32(gout) * (f32(scale) / f32(np.float32(count)))


def emu_l1_grad(a, b, g, dtype, relu_a=False, defect=None):
  d = a - b
  z = torch.zeros_like(a)
  out = torch.where(d > 0, z + g, torch.where(d < 0, z - g, z))
  if relu_a:
    alive = (a >= 0) if defect == 'mask_ge' else (a > 0)
    out = torch.where(alive, out, z)
  return st(out, dtype)


def emu_mse_grad(a, b, g, dtype):
  return st((2.0 * (a - b)) * g, dtype)


def emu_mse_const_grad(x, target, g, dtype):
  """x: [N, H, W, Cs] with one logical channel; only channel 0 carries gradient."""
  out = torch.zeros_like(x)
  out[..., 0] = (2.0 * (x[..., 0] - f32(target))) * g
  return st(out, dtype)


# ---- losses: the two-stage reduction --------------------------------------------------------------------------------------------
def loss_partial_count(work_items):
  return int(jpdse_hip.lib().jpdse_loss_partial_count(int(work_items)))


def loss_terms(kind, a, b=None, target=0.0, dtype=F32):
  """([work_items, terms per item] fp32 terms as the first stage forms them, fp64 terms).  l1 / mse: one item per 16-byte
  vector; mse_const: one item per pixel (channel 0)."""
  if kind == 'mse_const':
    x = a[..., 0].reshape(-1, 1)
    d, d64 = x - f32(target), x.double() - float(np.float32(target))
  else:
    d, d64 = (a - b).reshape(-1, VE[dtype]), (a.double() - b.double()).reshape(-1, VE[dtype])
  return (d.abs(), d64.abs()) if kind == 'l1' else (d * d, d64 * d64)


def _acc(acc, t, defect):
  s = acc + t
  return s.to(torch.bfloat16).float() if defect == 'bf16_acc' else s


def block_sum_256(acc, defect=None):
  """[blocks, 256] -> [blocks]: the xor butterfly of each 64-lane wave (offsets 32 .. 1), then red[0] + red[1] + red[2] + red[3]."""
  v = acc.reshape(-1, 4, 64)
  lane = torch.arange(64)
  for off in (32, 16, 8, 4, 2, 1):
    v = _acc(v, v[:, :, lane ^ off], defect)
  w = v[:, :, 0]
  return _acc(_acc(_acc(w[:, 0], w[:, 1], defect), w[:, 2], defect), w[:, 3], defect)


def emu_loss(terms, count, defect=None):
  """Faithful fp32 emulation of loss_partial_kernel + loss_final_kernel on the first stage's terms; returns the fp32 value.
  Defects: drop_last_vector, skip_second_sweep, drop_partial, dup_partial, bf16_acc."""
  total, per = terms.shape
  grid = loss_partial_count(total)
  threads = grid * 256
  sweeps = -(-total // threads)
  t = torch.zeros((sweeps * threads, per), dtype=torch.float32)
  t[:total] = terms
  if defect == 'drop_last_vector':
    t[total - 1] = 0
  t = t.view(sweeps, threads, per)
  acc = torch.zeros(threads, dtype=torch.float32)
  for s in range(sweeps):
    if defect == 'skip_second_sweep' and s == 1:
      continue
    for e in range(per):
      acc = _acc(acc, t[s, :, e], defect)
  partial = block_sum_256(acc.view(grid, 256), defect)
  if defect == 'drop_partial':
    partial[grid - 1] = 0
  if defect == 'dup_partial':
    partial[grid - 1] = partial[grid - 1] * 2
  n2 = -(-grid // 256)
  p2 = torch.zeros(n2 * 256, dtype=torch.float32)
  p2[:grid] = partial
  p2 = p2.view(n2, 256)
  acc = torch.zeros(256, dtype=torch.float32)
  for k in range(n2):
    acc = _acc(acc, p2[k], defect)
  tot = block_sum_256(acc.view(1, 256), defect)[0]
  return (tot * (f32(1.0) / f32(np.float32(count)))).item()


def loss_depth(work_items, per):
  """D of a loss value: the per-thread loop (sweeps x terms per item), the wave tree (6), the block stage (3), the final-stage
  loop (partials / 256), its wave tree and block stage (6 + 3), and 3 for the final multiply and the output rounding.
  Every term is charged the longest chain although only the first lanes walk it; the roundings inside a term (a - b, d * d:
  at most 3 u |term|, once, before the chain) are not counted on top of that."""
  grid = loss_partial_count(work_items)
  sweeps = -(-work_items // (grid * 256))
  return sweeps * per + 6 + 3 + -(-grid // 256) + 6 + 3 + 3


# ---- quantised evaluation loss ---------------------------------------------------------------------------------------------------
def quant_u8(x, mean, std):
  """uint8(clip((double(x) * std[c] + mean[c]) * 255.0, 0, 255)) over the last axis = channels; numpy float64, unfused."""
  v = (x.double().numpy() * np.asarray(std, dtype=np.float64) + np.asarray(mean, dtype=np.float64)) * 255.0
  return np.clip(v, 0, 255).astype(np.uint8).astype(np.int64)


def quant_loss_value(a, b, C, mean, std, mse):
  """a, b: [N, H, W, Cs] values as the device holds them.  float32(total * (1.0 / count)), total an exact integer."""
  d = quant_u8(a[..., :C], mean, std) - quant_u8(b[..., :C], mean, std)
  total = int((d * d).sum() if mse else np.abs(d).sum())
  return np.float32(float(total) * (1.0 / float(d.size)))


# ---- channel_sum ------------------------------------------------------------------------------------------------------------------
def csum_geom(dtype, npix, Cs):
  """Restatement of csum_geom (elementwise.hip): TX column lanes x TY pixel lanes per block of 256, nblk pixel blocks of ppb
  pixels.  `cases` names the paths of channel_sum_kernel / channel_sum_final_kernel this shape takes."""
  cv = Cs // VE[dtype]
  TX = 1
  while TX < cv and TX < 256:
    TX <<= 1
  TY = 256 // TX
  nblk = 512
  if nblk * TY * 4 > npix:
    nblk = (npix + TY * 4 - 1) // (TY * 4)
  nblk = max(nblk, 1)
  ppb = (npix + nblk - 1) // nblk
  nblk = (npix + ppb - 1) // ppb
  per = (nblk + 3) // 4
  sizes = [min((g + 1) * per, nblk) - g * per for g in range(4)]
  last = npix - (nblk - 1) * ppb
  iters = sorted({-(-max(n - ty, 0) // TY) for n in (ppb, last) for ty in range(TY)})
  cases = set()
  cases.add('one_block' if nblk == 1 else 'blocks_%d' % nblk if nblk in (3, 5, 9, 512) else 'blocks_other')
  if any(s <= 0 for s in sizes):
    cases.add('empty_final_group')
  if any(s >= 8 and s % 8 for s in sizes):
    cases.add('final_unrolled8_plus_tail')
  if any(0 < s < 8 for s in sizes):
    cases.add('final_tail_only')
  if last != ppb:
    cases.add('ragged_last_block')
  if any(i % 4 for i in iters):
    cases.add('thread_pixels_not_multiple_of_4')
  if any(i >= 4 for i in iters):
    cases.add('pixel_loop_unrolled4')
  if cv & (cv - 1) or cv < TX:
    cases.add('idle_column_lanes')
  if TY == 1:
    cases.add('ty_1')
  if TY == 2:
    cases.add('ty_2')
  return dict(cv=cv, TX=TX, TY=TY, ppb=ppb, nblk=nblk, per=per, iters=max(iters), cases=cases)


def csum_depth(dtype, npix, Cs):
  """D of channel_sum: the per-thread pixel loop, the block stage (TY additions), the final-stage loop (a group's partials)
  and its two-level tree.  The output is the fp32 sum itself: no multiply, no further rounding."""
  g = csum_geom(dtype, npix, Cs)
  return g['iters'] + g['TY'] + g['per'] + 2


def emu_channel_sum(x, dtype, defect=None):
  """Faithful fp32 emulation of channel_sum_kernel + channel_sum_final_kernel on x: [npix, Cs].  Defects: drop_last_vector,
  drop_group, drop_ragged_block, bf16_acc."""
  npix, Cs = x.shape
  g = csum_geom(dtype, npix, Cs)
  TY, ppb, nblk, per = g['TY'], g['ppb'], g['nblk'], g['per']
  it = -(-ppb // TY)
  t = torch.zeros((nblk, it * TY, Cs), dtype=torch.float32)
  xx = x.clone()
  if defect == 'drop_last_vector':
    xx[npix - 1, Cs - VE[dtype]:] = 0
  full = (nblk - 1) * ppb
  t[:nblk - 1, :ppb] = xx[:full].view(nblk - 1, ppb, Cs)
  if defect != 'drop_ragged_block':
    t[nblk - 1, :npix - full] = xx[full:]
  t = t.view(nblk, it, TY, Cs)
  acc = torch.zeros((nblk, TY, Cs), dtype=torch.float32)
  for k in range(it):
    acc = _acc(acc, t[:, k], defect)
  part = torch.zeros((nblk, Cs), dtype=torch.float32)
  for y in range(TY):
    part = _acc(part, acc[:, y], defect)
  red = []
  for grp in range(4):
    a = torch.zeros(Cs, dtype=torch.float32)
    if not (defect == 'drop_group' and grp == 1):
      for b in range(grp * per, min((grp + 1) * per, nblk)):
        a = _acc(a, part[b], defect)
    red.append(a)
  return _acc(_acc(red[0], red[1], defect), _acc(red[2], red[3], defect), defect)


# ---- Adam ------------------------------------------------------------------------------------------------------------------------
# fp32 operations between the inputs and each output of adam_kernel (a fused multiply-add only removes roundings):
#   gi = g * grad_scale                                            1
#   m' = beta1 * m + (1 - beta1) * gi                              (1 - beta1), its product with gi, beta1 * m, the sum: 4, + gi
#   v' = beta2 * v + (1 - beta2) * gi * gi                         (1 - beta2), two products, beta2 * v, the sum: 5, + gi twice
#   p' = p - lr1 * m' / (sqrt(v') * isb2 + eps)                    lr1 * m', the division, the subtraction: 3; the denominator
#        carries half of v's 7 (3.5), the square root, the product and the sum: 6.5; m' carries its 5
# Every term of v' is non-negative, so its bound is relative to v' itself; m' and p' can cancel, so theirs are relative to the
# sum of the magnitudes of their terms.
K_M = 5
K_V = 7
K_P = 15          # 5 + 3 + 6.5, rounded up


def adam_scalars(lr, beta1, beta2, eps, step, grad_scale, defect=None):
  """The kernel's scalar arguments as jpdse_adam_step forms them: fp32 arguments, bias corrections in double, two roundings."""
  lr, b1, b2, eps, gs = [float(np.float32(v)) for v in (lr, beta1, beta2, eps, grad_scale)]
  s = step - 1 if defect == 'bias_step_minus_1' else step
  bc1, bc2 = 1.0 - b1 ** s, 1.0 - b2 ** s
  with np.errstate(divide='ignore'):
    lr1 = float(np.float32(np.float64(lr) / np.float64(bc1)))
    isb2 = float(np.float32(np.float64(1.0) / np.sqrt(np.float64(bc2))))
  return dict(lr1=lr1, b1=b1, b2=b2, eps=eps, isb2=isb2, gs=gs)


def emu_adam(p, g, m, v, sc, defect=None):
  """Faithful unfused fp32 emulation of one adam_kernel update of a flat tensor; returns (p', m', v').
  Defect drop_tail: the last n % 4 elements are not updated."""
  t = {k: f32(x) for k, x in sc.items()}
  gi = g * t['gs']
  m2 = t['b1'] * m + (f32(1.0) - t['b1']) * gi
  v2 = t['b2'] * v + ((f32(1.0) - t['b2']) * gi) * gi
  p2 = p - (t['lr1'] * m2) / (torch.sqrt(v2) * t['isb2'] + t['eps'])
  if defect == 'drop_tail':
    keep = p.numel() - p.numel() % 4
    p2[keep:], m2[keep:], v2[keep:] = p[keep:], m[keep:], v[keep:]
  return p2, m2, v2


def adam64(p, g, m, v, sc):
  """fp64 Adam from the same fp32 inputs and the kernel's own scalar arguments: (p', m', v', bound_p, bound_m, bound_v)."""
  p, g, m, v = p.double(), g.double(), m.double(), v.double()
  gi = g * sc['gs']
  t1, t2 = sc['b1'] * m, (1.0 - sc['b1']) * gi
  m2 = t1 + t2
  v2 = sc['b2'] * v + (1.0 - sc['b2']) * gi * gi
  den = torch.sqrt(v2) * sc['isb2'] + sc['eps']
  p2 = p - sc['lr1'] * m2 / den
  Tm = t1.abs() + t2.abs()
  return p2, m2, v2, K_P * U * (p.abs() + sc['lr1'] * Tm / den), K_M * U * Tm, K_V * U * v2


def adam_used(got, ref, bound):
  got = torch.as_tensor(got).detach().cpu().double()
  r = (got - ref).abs() / bound.clamp_min(1e-300)
  r = torch.where((got == ref), torch.zeros_like(r), r)
  return torch.nan_to_num(r, nan=float('inf')).max().item() if r.numel() else 0.0


def assert_adam(p, m, v, ref, what):
  """p, m, v: the updated fp32 tensors (flat); ref: adam64's tuple."""
  for name, got, r, b, k in (('p', p, ref[0], ref[3], K_P), ('m', m, ref[1], ref[4], K_M), ('v', v, ref[2], ref[5], K_V)):
    used = adam_used(got, r, b)
    record('%s %s [adam: |err| / (k u (|value| + |update terms|)), k = %d]' % (what, name, k), used, 1.0)
    assert used <= 1.0, '%s: %s is %.3g x its bound away from fp64 Adam (k = %d)' % (what, name, used, k)


# ---- shapes and inputs shared by tests/test_ew_contract_host.py and tests/test_hip_ew_contract.py ---------------------------
def map_shapes(dtype):
  """(N, C, H, W) of the tensor a grid-stride map enumerates: one vector; ragged, under one block; the same with 39 channels,
  so that the last vector of every pixel holds a padding lane; just over the 524288-vector cap of one sweep, so that the
  second sweep is partial (532480 vectors)."""
  return {'one': (1, 3, 1, 1), 'ragged': (2, 24, 5, 7), 'ragged39': (2, 39, 5, 7),
          'cap': (1, 64, 260, 256) if dtype == BF16 else (1, 32, 260, 256)}


MAP_CASES = ['one', 'ragged', 'ragged39', 'cap']
SUB = 2.0 ** -133             # the smallest bf16 subnormal


# channel_copy and insert_channels do not enumerate the tensor's vectors: their own work items, and the wide moves that take
# them past the cap of one sweep at the 'cap' shape
def channel_copy_items(npix, nch):
  return npix * nch


def insert_channels_items(dtype, npix, c0, nch):
  """One item per pixel and 16-byte vector of the destination that holds one of the channels [c0, c0 + nch)."""
  return npix * ((c0 + nch - 1) // VE[dtype] - c0 // VE[dtype] + 1)


WIDE_COPY_NCH = 8             # channel_copy of 8 channels per pixel: 66560 * 8 = 532480 items
WIDE_INSERT_C0 = 4            # insert_channels of the whole 'cap' image at channel 4 of a destination 8 channels wider:
                              # 9 vectors per pixel in bf16 (599040 items), 8 in fp32 (532480)


def edge_y(shape, dtype, seed, tanh=False):
  """An activation output with the mask's edges in it: exact +0.0, -0.0 and the smallest bf16 subnormal of either sign in the
  first and the last pixel; for tanh, |y| = 1 exactly in the last one."""
  y = randn_nhwc(shape, dtype, seed)
  if tanh:
    y = st(torch.tanh(y), dtype)
  flat = y.view(-1, y.shape[-1])
  n = flat.shape[0]
  flat[0, 0], flat[0, 1], flat[0, 2] = 0.0, -0.0, SUB
  flat[n - 1, 0], flat[n - 1, 1], flat[n - 1, 2] = (1.0, -1.0, -SUB) if tanh else (-0.0, 0.0, -SUB)
  return y


def plateau(shape, per_window):
  """A max-pool input whose every 2 x 2 window is a four-way tie: constant per window, or constant everywhere."""
  N, C, H, W = shape
  if not per_window:
    return pad_lanes(torch.full((N, H, W, C), 1.5), C)
  v = torch.randint(-3, 4, (N, H // 2 + 1, W // 2 + 1, C), generator=G(7)).float()
  return pad_lanes(v.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :H, :W].contiguous(), C)


CAST_N = 8 * (EW_CAP + 3)

# loss shapes (N, C, H, W) by the number of 16-byte vectors (bf16: one per pixel of 8 lanes; fp32: two)
LOSS_SHAPES = {
    'v1':        {BF16: (1, 3, 1, 1),     F32: (1, 3, 1, 1)},        # one vector (fp32: the two of one pixel)
    'p255':      {BF16: (1, 3, 255, 256), F32: (1, 3, 255, 128)},    # 256 * 255 vectors: 255 partials
    'p256':      {BF16: (1, 3, 256, 256), F32: (1, 3, 128, 256)},    # 256 partials: the final stage's loop runs once, full
    'p257':      {BF16: (1, 3, 257, 256), F32: (1, 3, 257, 128)},    # 257 partials: thread 0 of the final stage reads two
    'cap':       {BF16: (1, 3, 512, 512), F32: (1, 3, 256, 512)},    # 262144 vectors: the 1024-partial cap, one full sweep
    'cap_ragged': {BF16: (1, 3, 520, 512), F32: (1, 3, 260, 512)},   # 266240 vectors: a ragged second sweep
    'cap_ragged_c8': {BF16: (1, 8, 520, 512), F32: (1, 8, 260, 512)},  # the same with no padding lanes: every vector counts
}
MSE_CONST_SHAPES = {'small': (3, 1, 7, 11), 'cap_ragged': (1, 1, 520, 512)}


def G(seed):
  return torch.Generator().manual_seed(seed)


def randn_nhwc(shape, dtype, seed, mean=0.0, scale=1.0):
  """[N, H, W, Cs] fp32 holding storage-type values, zero padding lanes."""
  N, C, H, W = shape
  return pad_lanes(st(torch.randn((N, H, W, C), generator=G(seed)) * scale + mean, dtype), C)


def int_nhwc(shape, lo, hi, seed):
  """Small integers in [lo, hi] (exact in bf16)."""
  N, C, H, W = shape
  return pad_lanes(torch.randint(lo, hi + 1, (N, H, W, C), generator=G(seed)).float(), C)


def loss_int_pair(shape, seed=1):
  """Integer a in [-1, 2] (zeros and negatives: the ReLU mask), b in [0, 2]; the first and the last pixel differ in every channel,
  so that no edge vector's terms vanish."""
  a, b = int_nhwc(shape, -1, 2, seed), int_nhwc(shape, 0, 2, seed + 1)
  C = shape[1]
  for pix in (0, -1):
    a.view(-1, a.shape[-1])[pix, :C] = 2.0
    b.view(-1, b.shape[-1])[pix, :C] = 0.0
  return a, b


def loss_randn_pair(shape, dtype, seed=3):
  """randn with a non-zero mean: the sum grows with the tensor, which is what an accumulator of too few bits cannot follow."""
  return randn_nhwc(shape, dtype, seed, mean=0.75), randn_nhwc(shape, dtype, seed + 1, mean=-0.5)


# channel_sum: (name, dtype, npix, C) -> the paths named by csum_geom(...)['cases']
CSUM_CASES = [
    ('one_block',      BF16, 35,     24),      # (2, 24, 5, 7)-sized: one pixel block
    ('blocks_3',       BF16, 700,    24),      # 3 blocks: the fourth final group is empty; ragged; 3 or 4 pixels per thread
    ('blocks_5',       F32,  300,    39),      # TX = 16 of which 10 lanes work
    ('blocks_9',       BF16, 2304,   24),      # 9 blocks: 3 + 3 + 3 + 0 partials per final group (tail loop only)
    ('blocks_35',      F32,  2240,   39),      # 35 blocks: 9 + 9 + 9 + 8 partials: the 8-wide unrolled loop, with and without tail
    ('full_512',       BF16, 132072, 24),      # 512 blocks of 258 pixels, the last one of 234
    ('wide_f32',       F32,  2051,   1024),    # TX = 256, TY = 1
    ('wide_bf16_512',  BF16, 5632,   1024),    # TY = 2, 512 blocks of 11 pixels: 6 and 5 pixels per thread
    ('c1',             F32,  1000,   1),       # one logical channel: two vectors per pixel, TY = 128
]
CSUM_REQUIRED = {'one_block', 'blocks_3', 'blocks_5', 'blocks_9', 'blocks_512', 'empty_final_group', 'final_unrolled8_plus_tail',
                 'final_tail_only', 'ragged_last_block', 'thread_pixels_not_multiple_of_4', 'pixel_loop_unrolled4',
                 'idle_column_lanes', 'ty_1', 'ty_2'}


def csum_inputs(dtype, npix, C, kind, seed=5):
  """[npix, Cs]: 'int' = integers in [-2, 3] (mean 0.5), 'randn' = randn + 0.75 in the storage type."""
  if kind == 'int':
    x = int_nhwc((1, C, 1, npix), -2, 3, seed)
    x.view(-1, x.shape[-1])[-1, :C] = 3.0
  else:
    x = randn_nhwc((1, C, 1, npix), dtype, seed, mean=0.75)
  return x.view(npix, -1)


ADAM_SIZES = [1, 3, 1023, 1024, 1025, 2048, 4099]
ADAM_TABLES = [1, 2, 3, 37]
ADAM_STEPS = [1, 2, 1000]
ADAM_HP = dict(lr=1e-2, beta1=0.5, beta2=0.999, eps=1e-8, grad_scale=1.0 / 3.0)


def adam_inputs(n, seed):
  """(p, g, m, v) fp32: parameters of size 0.01 next to lr = 1e-2, so that the update is as large as the value it changes."""
  g = G(seed)
  p = torch.randn(n, generator=g) * 0.01
  gr = torch.randn(n, generator=g)
  m = torch.randn(n, generator=g) * 0.3
  v = torch.rand(n, generator=g) * 0.2 + 0.01
  return p, gr, m, v
