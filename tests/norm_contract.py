"""Contract of the InstanceNorm kernels of csrc/norm.hip against fp64 arithmetic on the stored operands, form by form.

Operands are NHWC storage tensors [N, H, W, Cs] (Cs = C rounded up to 8) held as fp32 CPU tensors whose values are representable
in the storage type, as in tests/ew_contract.py.  The contract has three parts, so that no part hides behind another.

a. Statistics.  stats[n, c] = (mean, rstd) against the fp64 mean, biased variance and 1 / sqrt(var + eps).
   The kernels (norm.hip FwdMoments, finalize_fwd_kernel, inorm_reg_fwd_kernel) sum d = x - shift and d^2 in fp32 with
   shift = x[n, pixel 0, c], then dm = a (1 / HW), var = max(b (1 / HW) - dm^2, 0), mean = shift + dm, rstd = rsqrtf(var + eps).
   With A1 = sum|d|, B = sum d^2 (fp64, d exact), u = 2^-24 and LAMBDA the project's probabilistic constant
   (bf16_contract: an fp32 sum of n roundings errs by at most LAMBDA sqrt(n) u sum|terms|):
     Ea    = LAMBDA sqrt(HW + 2) u A1                 the sum of d: HW additions, the subtraction x - shift
     Eb    = LAMBDA sqrt(HW + 4) u B                  the sum of d^2: also the square (2 u from d, 1 u of its own)
     ddm   = Ea / HW + 2 u |dm|                       1 / HW and the product, one rounding each
     dmean = ddm + u |mean|                           the sum shift + dm; never below one ulp of the mean
     dvar  = Eb / HW + 2 |dm| ddm + ddm^2 + 3 u (B / HW + dm^2)       b / HW - dm^2: the bound is conditioned on the kernel's shift
                                                      (B = sum (x - shift)^2, not HW var): an outlier first pixel widens it
     dv    = dvar + u (var + eps)                     the sum var + eps
     drstd = (v - dv)^-1/2 - v^-1/2  (= 1/2 rstd^3 dv to first order; v - dv is kept >= eps, as the kernel's clamp keeps var >= 0)
             + RSQRT_ULPS ulp(rstd)                   rsqrtf itself
   The slot forms (inorm_reg_*_kernel PHASE 3, finalize_slots_kernel) merge per-slot (mean_s, M2_s) of equal pixel counts
   ns = HW / slots with Chan's formula; their operands are the slots, so the fp64 reference merges the same fp32 slot values:
     dmean = LAMBDA sqrt(slots + 1) u sum|mean_s| / slots + u |mean|
     dT    = LAMBDA sqrt(2 slots + 4) u sum (M2_s + ns dm_s^2) + ns (2 sum|dm_s| dmean + slots dmean^2)      dm_s = mean_s - mean
     dvar  = dT / HW + 2 u var,  then dv and drstd as above.

b. Forward output, given the DEVICE's statistics (read back): act((x - mean) rstd) [+ res] in fp64 with those fp32 stats.
   bf16: assert_bf16_contract with the single rounding of the fp64 value and, where a residual follows, the unfused and the
   fused (contracted multiply-add) fp32 sequences; S = |x - mean| rstd + |res|, n = 3 fp32 operations (4 with a residual).
   fp32: within n u S.  Pad lanes are +0 bit for bit; a constant channel gives y == res (or 0) bit for bit.

c. Backward, given the device's stats: dx = rstd (dz - m1 - yhat m2), dz = dy act'(yhat), yhat recomputed from x and the stats,
   m1 = mean(dz), m2 = mean(dz yhat).  Element-wise bound ulp + LAMBDA sqrt(HW) u S with
   S = rstd (|dz| + mean|dz| + |yhat| mean|dz yhat|); bf16: also the share of elements that equal no correctly rounded candidate,
   counted where LAMBDA sqrt(HW) u S <= one bf16 ulp of the result (elsewhere cancellation leaves the rounding to fp32 noise).  Where yhat is within 4 u |x - mean| rstd of zero the mask may fall either
   way: the other side is a second candidate restricted to those elements, which must be fewer than CAP of the tensor.

Plumbing check: integer operands make every fp32 sum exact in any order, so a lost pixel, a row summed twice or a wrong divisor
changes the stored bits: `int_fwd_case` (mean bit-exact in every form, var + eps one of the fused / unfused candidates),
`int_slot_case` (the merge reproduces the exact totals), `int_bwd_case` (dy antisymmetric over a symmetric x: both sums are
exactly zero, dx must equal dz).

The emulations take an optional `defect`; tests/test_norm_contract_host.py plants each one and checks that the criterion meant
to catch it does.  Plain torch-CPU: no GPU is needed.
"""
import math

import numpy as np
import torch

from jpdse_hip import F32, BF16, ACT_NONE, ACT_RELU, ACT_LRELU
from bf16_contract import rn_bf16, ulp_bf16, U, LAMBDA, CAP, Cand, assert_bf16_contract, contract_figures
from ew_contract import ulp_f32, assert_pad_zero, assert_bits_equal, randn_nhwc, VE, cpad, st, rn32, G
from hip_util import record

EPS = 1e-5
EPS32 = float(np.float32(EPS))            # the kernels' eps and slope are fp32 arguments: the operands of the fp64 reference
SLOPE32 = float(np.float32(0.2))
P = 8                                     # pixels per thread of the register-held forms (reg_geom)
# rsqrtf: ROCm's math-function accuracy table is not shipped with the toolchain, so the allowance is measured:
# tests/test_hip_norm_contract.py::test_rsqrtf_allowance measured a worst error of 0.785 ulp against fp64 1 / sqrt over 20993
# arguments on MI355X (the var + eps values of this suite's own inputs and a log sweep of [eps, 4096]; parity report, 'rsqrtf');
# the test fails if the device ever exceeds half the allowance.  Twice 0.785, rounded up to a whole ulp:
RSQRT_ULPS = 2


def f32(v):
  return torch.tensor(float(v), dtype=torch.float32)


def flat(x):
  """[N, H, W, Cs] -> [N, HW, Cs]"""
  return x.reshape(x.shape[0], -1, x.shape[-1])


def pad_lanes(x, C):
  """[N, HW, C] -> [N, HW, Cs] with zero padding lanes."""
  out = torch.zeros(x.shape[:-1] + (cpad(C),), dtype=x.dtype)
  out[..., :C] = x
  return out


# ---- geometry: restatements of moment_geom, fused_geom, reg_geom (norm.hip) --------------------------------------------------
def _tx(cv, cap):
  tx = 1
  while tx < cv and tx < cap:
    tx <<= 1
  return tx


def moment_geom(N, HW, Cs, ve):
  cv = Cs // ve
  TX = _tx(cv, 256)
  TY = 256 // TX
  col_blocks = -(-cv // TX)
  want = max(2048 // (N * col_blocks), 1)
  want = min(want, max(HW // (TY * 8), 1), 256)
  pps = -(-HW // want)
  return dict(cv=cv, TX=TX, TY=TY, col_blocks=col_blocks, splits=-(-HW // pps), pps=pps, HW=HW)


def fused_geom(N, HW, Cs, ve):
  cv = Cs // ve
  TX = _tx(cv, 16)
  TY = 256 // TX
  span = TY * P
  return dict(cv=cv, TX=TX, TY=TY, col_blocks=-(-cv // TX), span=span, splits=-(-HW // span), nv=TX * ve * 2, HW=HW)


def reg_geom(N, HW, Cs, ve):
  g = fused_geom(N, HW, Cs, ve)
  return None if g['splits'] > 64 or N * g['col_blocks'] * g['splits'] > (1 << 30) else g


def norm_form(dtype, N, HW, C, three_kernel=False, slots=0, alias=0):
  """(form, geometry) a call reaches: 'rows' (two register-held kernels), 'moment' (moment -> finalize -> apply), 'phase3'
  (one kernel from producer slots), 'slots' (slot finalize + apply).  three_kernel: the developer build's mode 27."""
  ve, Cs = VE[dtype], cpad(C)
  rg = None if three_kernel else reg_geom(N, HW, Cs, ve)
  if slots:
    if rg is not None and slots <= 64:
      return 'phase3', rg
    return 'slots', moment_geom(N, HW, Cs, ve)
  if rg is not None:
    return 'rows', rg
  return 'moment', moment_geom(N - alias, HW, Cs, ve)


def reduce_splits_trips(splits):
  """(trips of the four-at-a-time loop, trips of its tail) of each of the 8 lanes of reduce_splits."""
  out = []
  for sub in range(8):
    s, four, tail = sub, 0, 0
    while s + 24 < splits:
      s, four = s + 32, four + 1
    while s < splits:
      s, tail = s + 8, tail + 1
    out.append((four, tail))
  return out


def finalize_slots_trips(slots):
  """The same for the 64 lanes of finalize_slots_kernel's first pass."""
  out = []
  for lane in range(64):
    s, four, tail = lane, 0, 0
    while s + 192 < slots:
      s, four = s + 256, four + 1
    while s < slots:
      s, tail = s + 64, tail + 1
    out.append((four, tail))
  return out


def loop_and_tail(trips):
  """Some lane runs the unrolled loop AND its tail."""
  return any(a > 0 and b > 0 for a, b in trips)


# ---- fp32 emulations of the reductions --------------------------------------------------------------------------------------
def reduce_rows(t, g, defect=None):
  """PHASE 1 + sum_rows of one image: t [HW, Cs] fp32 terms -> [Cs] totals.  A thread adds its P pixels in order, block_row the
  TY thread rows in order, sum_rows the splits in order.  Defects: drop_last_pixel, skip_row_16, dup_row_16."""
  HW, Cs = t.shape
  span, TY, splits = g['span'], g['TY'], g['splits']
  buf = torch.zeros((splits * span, Cs), dtype=torch.float32)
  buf[:HW] = t
  if defect == 'drop_last_pixel':
    buf[HW - 1] = 0
  buf = buf.view(splits, P, TY, Cs)
  acc = torch.zeros((splits, TY, Cs), dtype=torch.float32)
  for i in range(P):
    acc = acc + buf[:, i]
  row = torch.zeros((splits, Cs), dtype=torch.float32)
  for y in range(TY):
    row = row + acc[:, y]
  tot = torch.zeros(Cs, dtype=torch.float32)
  for s in range(splits):
    if defect == 'skip_row_16' and s == 16:
      continue
    tot = tot + row[s]
    if defect == 'dup_row_16' and s == 16:
      tot = tot + row[s]
  return tot


def reduce_moment(t, g, defect=None):
  """moment_kernel + reduce_splits of one image: thread row ty walks the pixels p0 + ty, + TY, ... of its split; the TY rows are
  added in order; lane sub of 8 adds the splits sub, sub + 8, ...; xor butterfly 4, 2, 1.  Defect: drop_last_pixel."""
  HW, Cs = t.shape
  TY, splits, pps = g['TY'], g['splits'], g['pps']
  it = -(-pps // TY)
  buf = torch.zeros((splits, it * TY, Cs), dtype=torch.float32)
  for s in range(splits):
    p0, p1 = s * pps, min((s + 1) * pps, HW)
    buf[s, :p1 - p0] = t[p0:p1]
    if defect == 'drop_last_pixel' and p1 == HW:
      buf[s, p1 - p0 - 1] = 0
  buf = buf.view(splits, it, TY, Cs)
  acc = torch.zeros((splits, TY, Cs), dtype=torch.float32)
  for k in range(it):
    acc = acc + buf[:, k]
  part = torch.zeros((splits, Cs), dtype=torch.float32)
  for y in range(TY):
    part = part + acc[:, y]
  k = -(-splits // 8)
  pp = torch.zeros((k * 8, Cs), dtype=torch.float32)
  pp[:splits] = part
  pp = pp.view(k, 8, Cs)
  v = torch.zeros((8, Cs), dtype=torch.float32)
  for j in range(k):
    v = v + pp[j]
  lane = torch.arange(8)
  for off in (4, 2, 1):
    v = v + v[lane ^ off]
  return v[0]


def reduce_terms(t, form, g, defect=None):
  return reduce_rows(t, g, defect) if form == 'rows' else reduce_moment(t, g, defect)


def finalize_stats(a, b, shift, HW, eps=EPS, defect=None):
  """finalize_fwd_kernel / the PHASE 2 prologue, unfused fp32: [.., 2] = (mean, rstd).  Defect: divisor_hw_minus_1."""
  inv = f32(1.0) / f32(HW - 1 if defect == 'divisor_hw_minus_1' else HW)
  dm = a * inv
  var = (b * inv - dm * dm).clamp_min(0.0)
  return torch.stack([shift + dm, torch.rsqrt(var + f32(eps))], dim=-1)


def emu_stats(x, form, g, eps=EPS, defect=None):
  """x [N, HW, Cs] -> stats [N, Cs, 2] as form `form` ('rows' / 'moment') computes them."""
  out = []
  for n in range(x.shape[0]):
    d = x[n] - x[n, :1]
    out.append(finalize_stats(reduce_terms(d, form, g, defect), reduce_terms(d * d, form, g, defect), x[n, 0], x.shape[1], eps,
                              defect))
  return torch.stack(out)


def _lanes(v, lanes, offs):
  """v [.., slots] -> lane l adds the entries l, l + lanes, ... in order; xor butterfly over `offs`; lane 0's value."""
  n = v.shape[-1]
  k = -(-n // lanes)
  buf = torch.zeros(v.shape[:-1] + (k * lanes,), dtype=torch.float32)
  buf[..., :n] = v
  buf = buf.view(v.shape[:-1] + (k, lanes))
  acc = torch.zeros(v.shape[:-1] + (lanes,), dtype=torch.float32)
  for j in range(k):
    acc = acc + buf[..., j, :]
  lane = torch.arange(lanes)
  for off in offs:
    acc = acc + acc[..., lane ^ off]
  return acc[..., 0]


def _serial(v):
  acc = torch.zeros(v.shape[:-1], dtype=torch.float32)
  for q in range(v.shape[-1]):
    acc = acc + v[..., q]
  return acc


def emu_slot_stats(mom, HW, form, eps=EPS, defect=None):
  """Chan's merge of mom [N, Cs, slots, 2] = (mean_s, M2_s) as PHASE 3 ('phase3': one thread, slot order) or
  finalize_slots_kernel ('slots': 64 lanes, xor tree) performs it.  Defects: no_ns_dm2, mean_div_slots_minus_1."""
  slots = mom.shape[2]
  add = _serial if form == 'phase3' else (lambda v: _lanes(v, 64, (32, 16, 8, 4, 2, 1)))
  mean = add(mom[..., 0]) / f32(slots - 1 if defect == 'mean_div_slots_minus_1' else slots)
  ns = f32(HW) / f32(slots)
  dm = mom[..., 0] - mean[..., None]
  term = mom[..., 1] if defect == 'no_ns_dm2' else mom[..., 1] + ns * dm * dm
  var = (add(term) / f32(HW)).clamp_min(0.0)
  return torch.stack([mean, torch.rsqrt(var + f32(eps))], dim=-1)


def emu_slot_sums(sl, HW, form):
  """sl [N, Cs, slots, 2] = (sum dz, sum dz yhat) per slot -> [N, Cs, 2] = (m1, m2): PHASE 3 adds in slot order,
  finalize_bwd_slots_kernel with 8 lanes and the xor tree 1, 2, 4."""
  add = _serial if form == 'phase3' else (lambda v: _lanes(v, 8, (1, 2, 4)))
  inv = f32(1.0) / f32(HW)
  return torch.stack([add(sl[..., 0]) * inv, add(sl[..., 1]) * inv], dim=-1)


# ---- fp32 emulations of the apply expressions -----------------------------------------------------------------------------------
def emu_apply_fwd(x, stats, act, res, dtype, C=None, slope=SLOPE32, defect=None):
  """x, res [N, HW, Cs]; stats [N, Cs, 2].  Unfused fp32: norm_act, then the residual, one store rounding.
  Defects: res_before_act, slope_on_positive, nonzero_pad (needs C)."""
  t = (x - stats[:, None, :, 0]) * stats[:, None, :, 1]
  if defect == 'res_before_act' and res is not None:
    t = t + res
  if act == ACT_RELU:
    t = torch.where(t > 0, t, torch.zeros_like(t))
  elif act == ACT_LRELU:
    t = torch.where(t > 0, t * f32(slope), t) if defect == 'slope_on_positive' else torch.where(t > 0, t, t * f32(slope))
  if res is not None and defect != 'res_before_act':
    t = t + res
  if defect == 'nonzero_pad':
    t = t.clone()
    t[..., C:] = 2.0 ** -120
  return st(t, dtype)


def image_of(n, alias):
  return n - alias if alias and n >= alias else n


def bwd_terms(x, dy, stats, act, alias=0, slope=SLOPE32, mask_from=None):
  """(yhat, dz) in fp32 per gradient image; mask_from: a stored tensor whose sign replaces that of yhat (defect)."""
  idx = [image_of(n, alias) for n in range(dy.shape[0])]
  xs, ss = x[idx], stats[idx]
  yh = (xs - ss[:, None, :, 0]) * ss[:, None, :, 1]
  pos = (mask_from[idx] if mask_from is not None else yh) > 0
  one = torch.ones_like(yh)
  d = one if act == ACT_NONE else torch.where(pos, one, one * f32(slope if act == ACT_LRELU else 0.0))
  return yh, dy * d, ss


def emu_bwd(x, dy, stats, act, dtype, form, g, alias=0, slope=SLOPE32, defect=None, y=None):
  """The whole backward of form 'rows' / 'moment' in unfused fp32.  Defects: mask_from_stored_y (needs y), yhat_m2_sign,
  alias_off_by_one, and those of the reductions."""
  N, HW = dy.shape[0], dy.shape[1]
  yh, dz, ss = bwd_terms(x, dy, stats, act, alias, slope, y if defect == 'mask_from_stored_y' else None)
  if defect == 'alias_off_by_one':
    idx = [min(n - alias + 1, x.shape[0] - 1) if n >= alias else n for n in range(N)]
    ss = stats[idx]
    yh = (x[[image_of(n, alias) for n in range(N)]] - ss[:, None, :, 0]) * ss[:, None, :, 1]
  inv = f32(1.0) / f32(HW)
  m1 = torch.stack([reduce_terms(dz[n], form, g, defect) for n in range(N)]) * inv
  m2 = torch.stack([reduce_terms(dz[n] * yh[n], form, g, defect) for n in range(N)]) * inv
  return emu_apply_bwd(yh, dz, ss, torch.stack([m1, m2], dim=-1), dtype, defect)


def emu_apply_bwd(yh, dz, ss, sums, dtype, defect=None):
  m1, m2 = sums[:, None, :, 0], sums[:, None, :, 1]
  t = (dz - m1 + yh * m2) if defect == 'yhat_m2_sign' else (dz - m1 - yh * m2)
  return st(ss[:, None, :, 1] * t, dtype)


# ---- a. statistics ----------------------------------------------------------------------------------------------------------
def rstd_bound(v, dv, R=RSQRT_ULPS):
  """|rsqrtf(v') - v^-1/2| for |v' - v| <= dv, v' >= eps (1 - u): the lower side is the wider one."""
  r = v.rsqrt()
  lo = torch.maximum(v - dv, torch.full_like(v, EPS32 * (1.0 - U)))
  return (lo.rsqrt() - r).clamp_min(0.0) + R * ulp_f32(r)


def stats_reference(x, eps32=EPS32, shift_free=False, R=RSQRT_ULPS):
  """x [N, HW, Cs] -> (mean, rstd, bound of the mean, bound of rstd), fp64 [N, Cs].  shift_free: the bound an ideal shift
  (the mean itself) would give, B = HW var -- quoted in the report next to the real one."""
  x = x.double()
  HW = x.shape[1]
  mean = x.mean(dim=1)
  var = ((x - mean[:, None]) ** 2).mean(dim=1)
  v = var + eps32
  d = x - (mean[:, None] if shift_free else x[:, :1])
  A1, B, dm = d.abs().sum(dim=1), (d * d).sum(dim=1), d.mean(dim=1)
  Ea = LAMBDA * math.sqrt(HW + 2) * U * A1
  Eb = LAMBDA * math.sqrt(HW + 4) * U * B
  ddm = Ea / HW + 2 * U * dm.abs()
  bmean = torch.maximum(ddm + U * mean.abs(), ulp_f32(mean))
  dvar = Eb / HW + 2 * dm.abs() * ddm + ddm * ddm + 3 * U * (B / HW + dm * dm)
  return mean, v.rsqrt(), bmean, rstd_bound(v, dvar + U * v, R)


def slot_stats_reference(mom, HW, eps32=EPS32, R=RSQRT_ULPS):
  """mom [N, Cs, slots, 2] fp32 slot operands -> the same four for Chan's merge of them."""
  mom = mom.double()
  slots = mom.shape[2]
  ms, M2 = mom[..., 0], mom[..., 1]
  ns = HW / slots
  mean = ms.mean(dim=-1)
  bmean = torch.maximum(LAMBDA * math.sqrt(slots + 1) * U * ms.abs().sum(dim=-1) / slots + U * mean.abs(), ulp_f32(mean))
  dm = ms - mean[..., None]
  T = (M2 + ns * dm * dm).sum(dim=-1)
  var = T / HW
  dT = LAMBDA * math.sqrt(2 * slots + 4) * U * T + ns * (2 * dm.abs().sum(dim=-1) * bmean + slots * bmean * bmean)
  v = var + eps32
  return mean, v.rsqrt(), bmean, rstd_bound(v, dT / HW + 2 * U * var + U * v, R)


def used(got, ref, bound):
  got = torch.as_tensor(got).detach().cpu().double()
  r = (got - ref).abs() / bound
  r = torch.where(got == ref, torch.zeros_like(r), r)
  return torch.nan_to_num(r, nan=float('inf')).max().item()


def stats_figures(stats, ref):
  return used(stats[..., 0], ref[0], ref[2]), used(stats[..., 1], ref[1], ref[3])


def assert_stats(stats, x, what):
  """stats [N, Cs, 2] (device or emulation) against contract a for the shift forms."""
  ref = stats_reference(x)
  um, ur = stats_figures(stats, ref)
  fm, fr = stats_figures(stats, stats_reference(x, shift_free=True))
  record(what + ' [stats: |mean err| / bound]', um, 1.0, 'of the shift-free bound HW var: %.3g' % fm)
  record(what + ' [stats: |rstd err| / bound]', ur, 1.0, 'of the shift-free bound HW var: %.3g' % fr)
  assert um <= 1.0, '%s: the mean is %.3g x its bound away from fp64' % (what, um)
  assert ur <= 1.0, '%s: rstd is %.3g x its bound away from fp64' % (what, ur)


def assert_slot_stats(stats, mom, HW, what):
  um, ur = stats_figures(stats, slot_stats_reference(mom, HW))
  record(what + ' [slot stats: |mean err| / bound]', um, 1.0)
  record(what + ' [slot stats: |rstd err| / bound]', ur, 1.0)
  assert um <= 1.0, '%s: the merged mean is %.3g x its bound away from fp64' % (what, um)
  assert ur <= 1.0, '%s: the merged rstd is %.3g x its bound away from fp64' % (what, ur)


def rsqrt_ulp_error(got, arg):
  """Worst |got - arg^-1/2| in fp32 ulps of the fp64 value; arg: the fp32 arguments."""
  ref = arg.double().rsqrt()
  return ((got.double() - ref).abs() / ulp_f32(ref)).max().item()


# ---- b. forward given the stats ----------------------------------------------------------------------------------------------
def act_slope(t, act, slope):
  if act == ACT_RELU:
    return t.clamp_min(0.0)
  if act == ACT_LRELU:
    return torch.where(t > 0, t, t * slope)
  return t


def fwd_reference(x, stats, act, res, slope=SLOPE32):
  """(candidates, fp64 value, S, n).  x, res [N, HW, Cs] fp32 operands, stats [N, Cs, 2] fp32 as the device wrote them."""
  x = x.double()
  mean, rstd = stats[:, None, :, 0].double(), stats[:, None, :, 1].double()
  t = (x - mean) * rstd
  if res is None:
    return [Cand(act_slope(t, act, slope))], act_slope(t, act, slope), t.abs(), 3
  r = res.double()
  exact = act_slope(t, act, slope) + r
  t1 = rn32(x - mean)
  t2 = rn32(t1 * rstd)                                                 # 24 x 24 bits: exact in fp64 before the rounding
  a = rn32(act_slope(t2, act, slope))
  cands = [Cand(exact), Cand(rn32(a + r), name='unfused fp32')]
  if act == ACT_NONE:
    cands.append(Cand(rn32(t1 * rstd + r), name='fused multiply-add'))
  elif act == ACT_LRELU:
    cands.append(Cand(torch.where(t2 > 0, rn32(t2 + r), rn32(t2 * slope + r)), name='fused slope multiply-add'))
  return cands, exact, t.abs() + r.abs(), 4


def f32_used(got, ref, bound):
  got = torch.as_tensor(got).detach().cpu().double()
  r = (got - ref).abs() / bound
  return torch.nan_to_num(torch.where(got == ref, torch.zeros_like(r), r), nan=float('inf'))


def assert_pad_bits_zero(t, C, what):
  """Pad lanes are +0 bit for bit."""
  assert_pad_zero(t, C, what)
  if t.shape[-1] > C:
    pad = t[..., C:].contiguous()
    assert_bits_equal(pad, torch.zeros(pad.shape), what + ' pad lanes')


def assert_fwd(y, x, stats, act, res, C, dtype, what, slope=SLOPE32):
  """y [N, HW, Cs]: the device's (or an emulation's) output as fp32 / storage values."""
  y = torch.as_tensor(y).detach().cpu().float()
  cands, exact, S, n = fwd_reference(x, stats, act, res, slope)
  if dtype == BF16:
    assert_bf16_contract(y.double(), cands, S, n, what + ' fwd')
  else:
    r = f32_used(y, exact, n * U * S * (1.0 + 2.0 ** -20))
    record(what + ' fwd [fp32: |err| / (%d u S)]' % n, r.max().item(), 1.0)
    assert r.max().item() <= 1.0, '%s fwd: an element is %.3g x (%d u S) away from fp64' % (what, r.max().item(), n)
  assert_pad_bits_zero(y, C, what + ' fwd')


# ---- c. backward given the stats -----------------------------------------------------------------------------------------------
def bwd_reference(x, dy, stats, act, alias=0, slope=SLOPE32):
  """(candidates, S, HW, number of elements whose mask may fall either way)."""
  idx = [image_of(n, alias) for n in range(dy.shape[0])]
  x, dy, ss = x.double()[idx], dy.double(), stats.double()[idx]
  mean, rstd = ss[:, None, :, 0], ss[:, None, :, 1]
  HW = x.shape[1]
  yh = (x - mean) * rstd
  lo = 0.0 if act == ACT_RELU else slope

  def dx_of(pos):
    dz = dy if act == ACT_NONE else torch.where(pos, dy, dy * lo)
    m1, m2 = dz.mean(dim=1, keepdim=True), (dz * yh).mean(dim=1, keepdim=True)
    S = rstd * (dz.abs() + dz.abs().mean(dim=1, keepdim=True) + yh.abs() * (dz * yh).abs().mean(dim=1, keepdim=True))
    return rstd * (dz - m1 - yh * m2), S

  dx, S = dx_of(yh > 0)
  cands = [Cand(dx)]
  # yhat == 0 exactly (x == mean: a constant channel, a pad lane) is no edge: fl(x - mean) has the sign of x - mean, so the
  # fp32 mask is false there as in fp64; only a non-zero yhat this small could round to either side
  amb = (yh != 0) & (yh.abs() <= 4 * U * (x - mean).abs() * rstd)
  n_amb = 0
  if act != ACT_NONE:
    n_amb = int(amb.sum())
    if n_amb:
      dx2, S2 = dx_of((yh > 0) ^ amb)
      cands.append(Cand(dx2, where=amb, name='mask on the other side'))
      S = torch.maximum(S, S2)
  return cands, S, HW, n_amb


def assert_bwd(dx, x, dy, stats, act, C, dtype, what, alias=0, slope=SLOPE32):
  dx = torch.as_tensor(dx).detach().cpu().float()
  cands, S, HW, n_amb = bwd_reference(x, dy, stats, act, alias, slope)
  record(what + ' bwd [share whose mask may fall either way]', n_amb / dx.numel(), CAP)
  assert n_amb < CAP * dx.numel(), '%s bwd: %d elements sit on the mask edge' % (what, n_amb)
  if dtype == BF16:
    # assert_bf16_contract's two criteria, the share taken over the elements whose rounding the contract settles: where the
    # summation bound alone exceeds one bf16 ulp of the result (dx is what cancellation leaves of dz - m1 - yhat m2; with two
    # pixels it leaves next to nothing) fp32 noise decides the rounding, and only the element-wise bound applies
    got = dx.double()
    worst, _, best = contract_figures(got, cands, S, HW)
    hit = torch.zeros(got.shape, dtype=torch.bool)
    for c in cands:
      eq = got == rn_bf16(c.pre)
      hit |= eq if c.where is None else (eq & c.where)
    settled = LAMBDA * math.sqrt(HW) * U * S <= ulp_bf16(rn_bf16(cands[0].pre))
    share = (~hit & settled).double().mean().item()
    record(what + ' bwd [bf16 contract: element-wise]', worst, 1.0)
    record(what + ' bwd [bf16 contract: share not correctly rounded, of the settled elements]', share, CAP,
           'settled: %.3f of the tensor' % settled.double().mean().item())
    assert worst <= 1.0, '%s bwd: an element is %.3g x its bound away from every candidate' % (what, worst)
    assert share <= CAP, '%s bwd: %.3f %% of the elements equal no correctly rounded candidate' % (what, 100 * share)
  else:
    best = torch.full(dx.shape, float('inf'), dtype=torch.float64)
    for c in cands:
      r = f32_used(dx, c.pre, ulp_f32(c.pre) + LAMBDA * math.sqrt(HW) * U * S)
      best = torch.minimum(best, r if c.where is None else torch.where(c.where, r, torch.full_like(r, float('inf'))))
    record(what + ' bwd [fp32 contract: element-wise]', best.max().item(), 1.0)
    assert best.max().item() <= 1.0, '%s bwd: an element is %.3g x its bound away from every candidate' % (what, best.max().item())
  assert_pad_bits_zero(dx, C, what + ' bwd')


# ---- plumbing: integer operands -------------------------------------------------------------------------------------------------
def is_pow2(n):
  return n & (n - 1) == 0


def _spread(x, corr):
  """Add sign(corr) to the first |corr| of the pixels 1 .. HW - 2 of x [N, HW, C] (corr [N, C] integers)."""
  HW = x.shape[1]
  assert int(corr.abs().max()) <= HW - 2, 'too few pixels to spread the correction over'
  k = torch.arange(HW - 2).view(1, -1, 1)
  x[:, 1:HW - 1] += torch.where(k < corr.abs()[:, None], corr.sign()[:, None], torch.zeros(1)).float()
  return x


def int_fwd_case(N, HW, C, seed):
  """[N, HW, Cs] small integers: first pixel 1, last pixel 3 (a dropped last pixel changes the sums).  HW a power of two:
  a, b, dm = a / HW and the mean are exact in fp32 as they are.  Otherwise the pixels in between are adjusted until
  sum (x - shift) = 0: dm = 0 and mean = shift whatever 1 / HW rounds to, while every split's own sum stays non-zero."""
  x = torch.randint(-2, 5, (N, HW, C), generator=G(seed)).float()
  x[:, 0] = 1.0
  x[:, HW - 1] = 3.0 if HW > 1 else 1.0
  if not is_pow2(HW):
    x = _spread(x, -(x - x[:, :1]).sum(dim=1).round())
  return pad_lanes(x, C)


def int_fwd_expect(x, eps32=EPS32):
  """x [N, HW, Cs] -> (exact mean, the candidate fp32 values of var + eps), fp64 [N, Cs]."""
  x = x.double()
  HW = x.shape[1]
  d = x - x[:, :1]
  a, b = d.sum(dim=1), (d * d).sum(dim=1)
  assert float(b.max()) < 2 ** 24
  inv = float(np.float32(1.0) / np.float32(HW))
  dm = a * inv
  mean = x[:, 0] + dm
  assert torch.equal(rn32(dm), dm) and torch.equal(rn32(mean), mean), 'dm and the mean must be exact in fp32'
  bi = rn32(b * inv)
  vs = [rn32(bi - rn32(dm * dm)), rn32(bi - dm * dm), rn32(b * inv - rn32(dm * dm)), rn32(b * inv - dm * dm)]
  return mean, [rn32(v.clamp_min(0.0) + eps32) for v in vs]


def assert_rstd_candidates(rstd, args, what, R=RSQRT_ULPS):
  rstd = torch.as_tensor(rstd).detach().cpu().double()
  best = torch.full(rstd.shape, float('inf'), dtype=torch.float64)
  for v in args:
    r = v.rsqrt()
    best = torch.minimum(best, (rstd - r).abs() / ulp_f32(r))
  record(what + ' [integer operands: rstd vs rsqrt of the exact var + eps, ulps]', best.max().item(), R)
  assert best.max().item() <= R, '%s: rstd is %.3g ulps from rsqrt of every exact var + eps candidate' % (what, best.max().item())


def assert_int_stats(stats, x, what):
  mean, args = int_fwd_expect(x)
  assert_bits_equal(stats[..., 0].contiguous(), mean.float(), what + ' integer operands: mean')
  assert_rstd_candidates(stats[..., 1], args, what)


def slots_of(x, slots):
  """x [N, HW, Cs] -> mom [N, Cs, slots, 2] = (mean, M2) of each run of HW / slots pixels, from fp64, stored in fp32."""
  N, HW, Cs = x.shape
  assert HW % slots == 0
  v = x.double().view(N, slots, HW // slots, Cs)
  m = v.mean(dim=2)
  M2 = ((v - m[:, :, None]) ** 2).sum(dim=2)
  return torch.stack([m, M2], dim=-1).permute(0, 2, 1, 3).contiguous().float()


def sum_slots_of(x, dy, stats, act, slots, slope=SLOPE32):
  """[N, Cs, slots, 2] = (sum dz, sum dz yhat) per slot, from fp64 on the fp32 (yhat, dz) operands' exact values."""
  N, HW, Cs = x.shape
  yh, dz, _ = bwd_terms(x.double(), dy.double(), stats.double(), act, 0, slope)
  a = dz.view(N, slots, HW // slots, Cs).sum(dim=2)
  b = (dz * yh).view(N, slots, HW // slots, Cs).sum(dim=2)
  return torch.stack([a, b], dim=-1).permute(0, 2, 1, 3).contiguous().float()


def int_slot_case(N, HW, C, slots, seed):
  """Integers whose total is HW / 2 per (image, channel), HW / slots a power of two: every slot mean, every M2, their merge
  (mean = 1/2: the sum of the slot means is slots / 2, which divides exactly) and sum (x - 1/2)^2 are exact in fp32."""
  assert HW % slots == 0 and is_pow2(HW // slots) and HW % 2 == 0
  x = torch.randint(-3, 4, (N, HW, C), generator=G(seed)).float()
  corr = (HW // 2 - x.sum(dim=1)).round()
  q = torch.trunc(corr / HW)                      # the same step for every pixel, then +-1 for the first |remainder| pixels
  rem = corr - q * HW
  k = torch.arange(HW).view(1, -1, 1)
  x = x + q[:, None] + torch.where(k < rem.abs()[:, None], rem.sign()[:, None], torch.zeros(1))
  return pad_lanes(x, C)


def assert_int_slot_stats(stats, x, C, what):
  """The merge reproduces the exact totals: mean = 1/2 bit for bit, var = sum (x - 1/2)^2 / HW rounded once."""
  HW = x.shape[1]
  xd = x.double()[..., :C]
  mean = xd.mean(dim=1)
  assert bool((mean == 0.5).all())
  b = ((xd - 0.5) ** 2).sum(dim=1)
  assert_bits_equal(stats[..., :C, 0].contiguous(), mean.float(), what + ' integer slots: mean')
  inv = float(np.float32(1.0) / np.float32(HW))
  args = [rn32(rn32(b / HW) + EPS32), rn32(rn32(b * inv) + EPS32)]
  assert_rstd_candidates(stats[..., :C, 1], args, what + ' slots')


PLUMB_SLOPE = 0.25        # exact in fp32 and bf16: dz = dy * slope stays on the integer grid / 4


def int_bwd_case(N, HW, C, seed):
  """(x, dy) [N, HW, Cs]: x symmetric under p -> HW - 1 - p, dy antisymmetric, both small integers.  With stats (0, 1):
  yhat = x, and sum dz = sum dz yhat = 0 exactly for every activation while every split's own sums are not: dx == dz."""
  g = G(seed)
  h = (HW + 1) // 2
  xa = torch.randint(-3, 4, (N, h, C), generator=g).float()
  da = torch.randint(1, 4, (N, h, C), generator=g).float() * (torch.randint(0, 2, (N, h, C), generator=g).float() * 2 - 1)
  x = torch.cat([xa, xa.flip(1)[:, HW % 2:]], dim=1)
  dy = torch.cat([da, -da.flip(1)[:, HW % 2:]], dim=1)
  if HW % 2:
    dy[:, h - 1] = 0.0
  return pad_lanes(x, C), pad_lanes(dy, C)


def unit_stats(N, Cs):
  s = torch.zeros((N, Cs, 2), dtype=torch.float32)
  s[..., 1] = 1.0
  return s


def int_bwd_expect(x, dy, act, alias=0):
  idx = [image_of(n, alias) for n in range(dy.shape[0])]
  if act == ACT_NONE:
    return dy.clone()
  return torch.where(x[idx] > 0, dy, dy * (PLUMB_SLOPE if act == ACT_LRELU else 0.0))


def assert_int_bwd(dx, x, dy, act, what, alias=0):
  dx = torch.as_tensor(dx).detach().cpu().float()
  n = int((dx != int_bwd_expect(x, dy, act, alias)).sum())
  record(what + ' [integer operands: dx != dz]', n, 0.0)
  assert n == 0, '%s: %d elements of dx differ from dz although both sums are exactly zero' % (what, n)


# ---- shapes and inputs shared by tests/test_norm_contract_host.py and tests/test_hip_norm_contract.py ------------------------
def main_c(dtype):
  """16 vectors per pixel: TX = 16, one column block, span = 128 pixels in either storage type."""
  return 16 * VE[dtype]


HW_EDGES = [1, 2, 100, 128, 129, 2048, 2049, 8192, 8193]
ROWS_SPLITS = {1: 1, 2: 1, 100: 1, 128: 1, 129: 2, 2048: 16, 2049: 17, 8192: 64}       # 8193: 65 splits, the moment form
# (act, residual) pairs run at every shape: the residual after no activation (the ResnetBlock's use) and after LeakyReLU
ACT_RES = [(ACT_NONE, True), (ACT_RELU, False), (ACT_LRELU, True), (ACT_NONE, False)]
CHANNELS = {BF16: [1, 3, 17, 72, 136], F32: [1, 3, 17, 36, 68]}        # fp32: 36 -> 10 vectors in 16 lanes, 68 -> 18 vectors
MOMENT_EXTRA = [(64, 8453), (8, 100)]      # (C, HW): > 24 splits with a ragged four-at-a-time loop; exactly one split
SLOT_CASES = [(1, 8), (2, 16), (64, 512), (65, 520), (260, 520)]       # (slots, HW)


def images_for(HW):
  return 2 if HW <= 2049 else 1             # keeps every tensor near 2 MB


def norm_inputs(N, HW, C, dtype, seed, mean=0.7, scale=1.5):
  """(x, dy, res) [N, HW, Cs]; dy is correlated with x, so that neither mean(dz) nor mean(dz yhat) is rounding noise."""
  x = flat(randn_nhwc((N, C, 1, HW), dtype, seed, mean=mean, scale=scale))
  e = flat(randn_nhwc((N, C, 1, HW), F32, seed + 1))
  dy = st(e + 0.5 * (x - mean) / scale + 0.25, dtype)
  dy[..., C:] = 0.0
  return x, dy, flat(randn_nhwc((N, C, 1, HW), dtype, seed + 2))


def conditioning_inputs(kind, N, HW, C, dtype, seed):
  if kind == 'mean100':
    return norm_inputs(N, HW, C, dtype, seed, mean=100.0, scale=0.5)
  x, dy, res = norm_inputs(N, HW, C, dtype, seed, mean=0.0, scale=1.0)
  if kind == 'outlier':
    x[:, 0, :C] = 64.0
  elif kind == 'constant':
    x[..., :C] = 1.5
  elif kind == 'constant_but_one':
    x[..., :C] = 1.5
    x[:, HW // 2, :C] = 2.5
  else:
    assert kind == 'plain'
  return x, dy, res


CONDITIONING = ['mean100', 'outlier', 'constant', 'constant_but_one']
