"""Rounding contract of the bf16 convolution kernels, checked against fp64 arithmetic on the kernels' own operands.

A bf16 kernel of this library reads exact bf16 operands, multiplies exactly, sums in fp32 and rounds its output to bf16.
Its output is therefore the fp64 result rounded once (round-to-nearest-even), except where fp32 summation noise moves the
sum across a rounding midpoint, or where the kernel itself rounds a partial result on purpose (a fold of the reflect padding,
the sum of an addend before the LeakyReLU slope).  Each rounding sequence the kernels use is a candidate; `assert_bf16_contract`
accepts an output element when it lies within one bf16 ulp plus the fp32 summation bound of one candidate, and it bounds the
share of elements that equal no correctly rounded candidate.

Plain torch-CPU helpers: no GPU is needed (tests/test_bf16_contract_host.py checks the criterion itself on the CPU).
"""
import zlib

import torch
import torch.nn.functional as F

from jpdse_hip import PAD_REFLECT, ACT_RELU, ACT_LRELU, ACT_TANH, F32
from hip_util import record, assert_close, RTOL

U = 2.0 ** -24          # unit roundoff of fp32
LAMBDA = 8.0            # probabilistic summation bound (Higham & Mary, SISC 2019): fails with probability <= 2n exp(-LAMBDA^2 / 2)
CAP = 0.01              # largest share of elements that may equal no correctly rounded candidate
SLOPE = 0.2             # LeakyReLU slope of every layer of the model

_MIN_NORMAL = 2.0 ** -126
_SUB_ULP = 2.0 ** -133  # bf16 spacing below 2^-125 (subnormals and the smallest binade)


# ---- reference arithmetic -------------------------------------------------------------------------------------------------
def rn_bf16(t):
  """fp64 -> bf16 round-to-nearest-even directly on the fp64 bit pattern (no detour through fp32, which rounds twice and
  gets some midpoints wrong), returned as fp64.  bf16 has 7 stored mantissa bits: the low 45 of the 52 are rounded off."""
  t = torch.as_tensor(t, dtype=torch.float64).contiguous()
  b = t.view(torch.int64)
  r = (b + ((b >> 45) & 1) + ((1 << 44) - 1)) & ~((1 << 45) - 1)
  out = r.view(torch.float64).clone()
  small = t.abs() < _MIN_NORMAL                      # subnormal bf16: a fixed spacing; torch.round is half-to-even
  if bool(small.any()):
    out[small] = torch.round(t[small] / _SUB_ULP) * _SUB_ULP
  return out


def ulp_bf16(v):
  """Spacing of bf16 at |v| (2^(e - 7) for |v| in [2^e, 2^(e+1))); at 0 (and below the normal range) the smallest normal spacing."""
  v = torch.as_tensor(v, dtype=torch.float64).abs()
  _, e = torch.frexp(v)                              # v = m 2^e, m in [0.5, 1)
  u = torch.ldexp(torch.ones_like(v), (e - 8).to(torch.float64))
  return torch.where(v < _MIN_NORMAL, torch.full_like(v, _SUB_ULP), u)


def act64(z, act):
  if act == ACT_RELU:
    return z.clamp_min(0.0)
  if act == ACT_LRELU:
    return torch.where(z > 0, z, z * SLOPE)
  if act == ACT_TANH:
    return torch.tanh(z)
  return z


def _pad(x, pad, mode):
  return F.pad(x, (pad,) * 4, mode='reflect') if mode == PAD_REFLECT else F.pad(x, (pad,) * 4)


def conv64(x, w, st, pad, mode):
  """Cross-correlation of the padded input (NCHW, KCRS), in the dtype of the operands."""
  return F.conv2d(_pad(x, pad, mode), w, stride=st)


def dgrad64(dy, w, x_shape, st, pad, mode):
  x = torch.zeros(x_shape, dtype=dy.dtype, requires_grad=True)
  (dx,) = torch.autograd.grad(conv64(x, w, st, pad, mode), (x,), dy)
  return dx.detach()


def wgrad64(x, dy, w_shape, st, pad, mode):
  w = torch.zeros(w_shape, dtype=x.dtype, requires_grad=True)
  (dw,) = torch.autograd.grad(conv64(x, w, st, pad, mode), (w,), dy)
  return dw.detach()


def dgrad_terms(N, C, H, W, K, R, S, st, pad, mode, oh, ow):
  """Number of products summed into each data-gradient element (contributing taps x K, reflect folds included)."""
  ones = torch.ones((N, 1, oh, ow), dtype=torch.float64)
  return dgrad64(ones, torch.ones((1, 1, R, S), dtype=torch.float64), (N, 1, H, W), st, pad, mode) * K


def border_band(H, W, width):
  """[H, W] mask of the pixels within `width` rows or columns of a border."""
  r = torch.arange(H).view(H, 1)
  c = torch.arange(W).view(1, W)
  return (r < width) | (r >= H - width) | (c < width) | (c >= W - width)


def conv_case_inputs(case, seed):
  """x, w, b, gy of a CONV_CASES entry, drawn as tests/test_hip_ops.py::test_conv_fwd_dgrad_wgrad draws them (same generator,
  seed and order); x, w and gy hold bf16 values (the filter too, so that packing it is exact), b is the fp32 bias."""
  name, N, H, W, C, K, k, st, pad, mode, act = case
  g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % 1000 + 7919 * seed)
  q = lambda t: t.to(torch.bfloat16).float()
  x = q(torch.randn(N, C, H, W, generator=g))
  w = q(torch.randn(K, C, k, k, generator=g) * (1.0 / (C * k * k) ** 0.5))
  b = torch.randn(K, generator=g) * 0.1
  oh, ow = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
  gy = q(torch.randn(N, K, oh, ow, generator=g))
  return x, w, b, gy


def fwd_reference(x, w, b, st, pad, mode, act):
  """(act(conv + b) in fp64, S = the same on |operands|, n = products per output element + the bias)."""
  x, w = x.double(), w.double()
  bb = (b.double() if b is not None else torch.zeros(w.shape[0], dtype=torch.float64)).view(1, -1, 1, 1)
  y = act64(conv64(x, w, st, pad, mode) + bb, act)
  S = conv64(x.abs(), w.abs(), st, pad, mode) + bb.abs()
  return y, S, w.shape[1] * w.shape[2] * w.shape[3] + 1


def dgrad_reference(dy, w, x_shape, st, pad, mode):
  """(exact data gradient, its candidates, S, n per element) for the bf16-valued fp64 operands dy, w."""
  exact, cands = dgrad_candidates(dy, w, x_shape, st, pad, mode)
  S = dgrad64(dy.abs(), w.abs(), x_shape, st, pad, mode)
  K, _, R, Sk = w.shape
  oh, ow = dy.shape[2], dy.shape[3]
  n = dgrad_terms(x_shape[0], x_shape[1], x_shape[2], x_shape[3], K, R, Sk, st, pad, mode, oh, ow).clamp_min(1)
  return exact, cands, S, n


def dz_operand(gy, y, act):
  """The bf16 gradient w.r.t. the pre-activation as the activation backward forms it from the stored output y (fp32 product
  rounded to bf16); fp64 tensors holding bf16 values."""
  gy, y = gy.double(), y.double()
  if act == ACT_RELU:
    return torch.where(y > 0, gy, torch.zeros_like(gy))
  if act == ACT_LRELU:
    return torch.where(y > 0, gy, rn_bf16((gy.float() * SLOPE).double()))
  if act == ACT_TANH:
    return rn_bf16((gy.float() * (1.0 - y.float() * y.float())).double())
  return gy


# ---- candidates --------------------------------------------------------------------------------------------------------------
class Cand(object):
  """One rounding sequence a kernel really performs: `pre` is the exact fp64 value before the output's final rounding (the
  criterion applies rn_bf16 to it).  `where`: the elements the sequence can produce (None: all).  `slack`: the one-ulp
  allowance of every rounding the sequence performs BEFORE the final one, carried to the output -- fp32 summation noise may
  move an intermediate sum across a midpoint exactly as it may move the final one, which the criterion's own ulp term allows
  for the final rounding only (None: no intermediate rounding)."""
  __slots__ = ('pre', 'where', 'slack', 'name')

  def __init__(self, pre, where=None, slack=None, name='single rounding'):
    self.pre, self.where, self.slack, self.name = pre, where, slack, name


def dgrad_candidates(dy, w, x_shape, st, pad, mode):
  """Candidates of a plain data gradient (dy NKHW, w KCRS, both fp64 holding bf16 values).  Single rounding of the exact
  result everywhere; on a reflect-padded layer, near the borders, the folds of the padded domain:
    - padded-domain fold (conv_dispatch_dgrad.h:684-691 reflect_fold_kernel, thin_in_rows.h:209-213 reflect_ring_fold_kernel):
      the gradient on the padded domain is stored in bf16 and its aliases are summed: RN(sum RN(part))
    - 3x3 stride 1 only -- ring fold (conv_dispatch_dgrad.h:44-86 ring_fold_kernel): the interior (zero-padded data gradient)
      is stored in bf16 before the fp32 ring sums are added: RN(RN(interior) + ring)
    - 3x3 stride 1 only -- folded frame (conv_dispatch_dgrad.h:88-133 ring_frame_kernel, gemm_halo.h VIRT): the dy pairs
      (and corner quadruples) that the fold adds are summed in fp32 and rounded to bf16 once before the GEMM reads them."""
  exact = dgrad64(dy, w, x_shape, st, pad, mode)
  cands = [Cand(exact)]
  if mode != PAD_REFLECT:
    return exact, cands
  N, C, H, W = x_shape
  K, _, R, S = w.shape
  band = border_band(H, W, pad + 1).view(1, 1, H, W).expand(x_shape)
  # padded-domain fold
  xp = torch.zeros((N, C, H + 2 * pad, W + 2 * pad), dtype=torch.float64, requires_grad=True)
  (P,) = torch.autograd.grad(F.conv2d(xp, w, stride=st), (xp,), dy)
  x0 = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
  fold = lambda t: torch.autograd.grad(_pad(x0, pad, mode), (x0,), t)[0]
  Pr = rn_bf16(P)
  cands.append(Cand(fold(Pr), band, fold(ulp_bf16(Pr)), 'padded-domain fold'))
  if R == 3 and S == 3 and st == 1 and pad == 1:
    interior = dgrad64(dy, w, x_shape, 1, 1, 0)
    ir = rn_bf16(interior)
    cands.append(Cand(ir + (exact - interior), band, ulp_bf16(ir), 'ring fold'))
    cands.append(Cand(frame_dgrad64(dy, w, round_frame=True), band, None, 'folded frame'))
  return exact, cands


def frame_dgrad64(dy, w, round_frame):
  """Data gradient of a reflect-padded 3x3 stride-1 conv as the folded-frame kernel forms it: dx[h][w] = sum over taps (u, v)
  of w[:, :, u, v]^T applied to the dy operand of that tap, where the operand is dy[h + 1 - u][w + 1 - v], except that output
  row 1 at u = 0 also reads dy row 0 (row -1 of the padded-domain gradient folded back), output row H-2 at u = 2 also reads
  dy row H-1, and columns alike; a multi-term operand is the frame value, rounded to bf16 once when `round_frame`."""
  N, K, H, W = dy.shape

  def sel(L, u):
    A = torch.zeros((L, L), dtype=torch.float64)
    for h in range(L):
      j = h + 1 - u
      if 0 <= j < L:
        A[h, j] = 1.0
      if h == 1 and u == 0:
        A[h, 0] = 1.0
      if h == L - 2 and u == 2:
        A[h, L - 1] = 1.0
    return A

  dx = torch.zeros((N, w.shape[1], H, W), dtype=torch.float64)
  for u in range(3):
    A = sel(H, u)
    for v in range(3):
      B = sel(W, v)
      op = torch.einsum('hr,nkrc,wc->nkhw', A, dy, B)
      if round_frame:
        multi = (A.sum(1).view(H, 1) * B.sum(1).view(1, W)) > 1
        op = torch.where(multi, rn_bf16(op), op)
      dx += torch.einsum('nkhw,kc->nchw', op, w[:, :, u, v])
  return dx


def fused_candidates(plain, addend, m):
  """Candidates of a data gradient with the fan-in addend and the (Leaky)ReLU mask in its epilogue: the sum is rounded
  before the slope (gemm_fast.h:168-176 add_bf16x8 then 203-215 lrelu_mask8; unfused form conv_dispatch_dgrad.h:136-161
  relu_mask_kernel, which also adds the addend to the already stored data gradient):
    RN(RN(dg + a) m)  and  RN(RN(RN(dg) + a) m),  dg ranging over the plain data gradient's candidates."""
  out = []
  for c in plain:
    base = c.slack if c.slack is not None else torch.zeros_like(c.pre)
    s1 = rn_bf16(c.pre + addend)
    not_id = (m != 1.0)
    # RN(dg + a) is an intermediate rounding only where the slope follows it
    out.append(Cand(s1 * m, c.where, (base + torch.where(not_id, ulp_bf16(s1), torch.zeros_like(s1))) * m.abs(),
                    c.name + ', addend, slope'))
    r = rn_bf16(c.pre)
    s2 = rn_bf16(r + addend)
    inter = ulp_bf16(r) * ((addend != 0) | not_id) + torch.where(not_id, ulp_bf16(s2), torch.zeros_like(s2))
    out.append(Cand(s2 * m, c.where, (base + inter) * m.abs(), c.name + ' (stored), addend, slope'))
  return out


# ---- the criteria -----------------------------------------------------------------------------------------------------------
def contract_figures(got, candidates, S, n):
  """(worst element's share of its bound, share of elements that equal no correctly rounded candidate)."""
  got = torch.as_tensor(got, dtype=torch.float64)
  summ = LAMBDA * torch.sqrt(torch.as_tensor(n, dtype=torch.float64)) * U * S
  best = torch.full_like(got, float('inf'))
  exact = torch.zeros(got.shape, dtype=torch.bool)
  for c in candidates:
    rc = rn_bf16(c.pre)
    bound = ulp_bf16(rc) + summ + (c.slack if c.slack is not None else 0.0)
    ratio = (got - rc).abs() / bound
    eq = got == rc
    if c.where is not None:
      ratio = torch.where(c.where, ratio, torch.full_like(ratio, float('inf')))
      eq = eq & c.where
    best = torch.minimum(best, ratio)
    exact |= eq
  share = 1.0 - exact.double().mean().item()
  return best.max().item(), share, best


def assert_bf16_contract(got, candidates, S, n, what, cap=CAP):
  """Element-wise: min over the candidates c of |got - RN(c)| <= ulp(RN(c)) + LAMBDA sqrt(n) u S (+ c's intermediate-rounding
  slack); and at most `cap` of the elements equal no RN(c).  Both figures go into the parity report."""
  worst, share, best = contract_figures(got, candidates, S, n)
  record(what + ' [bf16 contract: element-wise]', worst, 1.0)
  record(what + ' [bf16 contract: share not correctly rounded]', share, cap)
  if not worst <= 1.0:
    i = int(torch.argmax(torch.nan_to_num(best, nan=float('inf'))).item())
    idx = list(torch.unravel_index(torch.tensor(i), best.shape))
    g = float(torch.as_tensor(got, dtype=torch.float64).reshape(-1)[i])
    vals = ', '.join('%s %.8e' % (c.name, float(rn_bf16(c.pre).reshape(-1)[i])) for c in candidates)
    raise AssertionError('%s: element %s = %.8e is %.2fx its bound away from every candidate (%s)'
                         % (what, [int(v) for v in idx], g, worst, vals))
  assert share <= cap, '%s: %.3f %% of the elements equal no correctly rounded candidate (cap %.1f %%)' % (what, 100 * share, 100 * cap)
  return worst, share


def assert_fp32_vs_fp64(got, ref64, what):
  """An fp32 output whose only legitimate error is fp32 summation (bf16 operands and their products are exact in fp32):
  the fp32 pair of bounds RTOL[F32] / ETOL[F32], against fp64 arithmetic on the same operands."""
  assert_close(torch.as_tensor(got, dtype=torch.float64), ref64, RTOL[F32], what)
