"""GPU tests of the rate term of the vector-quantizer bottleneck (vq_bottleneck.hip: jpdse_vq_rate_fwd,
jpdse_vq_quantize_bwd_grouped; ops.vq_rate_fwd, ops.vq_quantize_bwd(groups, dhist), S2HVQ.rate) against the
float64 restatement tests/vq_rate_ref.py, the exact contracts (hard-mode counts, zeros of dhist), determinism, the refusals and
the module's autograd.

Cases (M, D, L, G): (1, 1, 2, 1) the smallest shape; (66, 8, 64, 2) a partial wave; (255, 3, 5, 3) G not a power of two, padded
D; (304, 32, 512, 16) the global-memory book, one wave per block; (4112, 8, 64, 16) the workload's grouping, 17 tiles, several
blocks; (4100, 8, 64, 20) the general path over many tiles; (1040, 4, 16, 130) G > 64; and the two sizes at which the launch
changes with the table's size: (320, 4, 64, 64) two waves per block, (256, 4, 512, 32) a power of two whose table does not fit
LDS (general path; the backward reads dhist from global memory)."""
import ctypes

import pytest
import torch

import jpdse_hip
from jpdse_hip import ops, F32, BF16
import hip_util as hu
import vq_util
import vq_rate_ref as ref
from test_hip_quantizers import _check_dx

pytestmark = pytest.mark.gpu
DEV = hu.DEV
TOL = hu.RTOL[F32]          # with ETOL[F32] through hip_util.assert_close
SIGMA = 10.0
DENOM, SCALE = 7.0, 0.5
CASES = [(1, 1, 2, 1), (66, 8, 64, 2), (255, 3, 5, 3), (304, 32, 512, 16), (4112, 8, 64, 16), (4100, 8, 64, 20),
         (1040, 4, 16, 130), (320, 4, 64, 64), (256, 4, 512, 32)]
_cache = {}


def _dev(t, dtype=None):
  t = t.to(DEV)
  return t.to(torch.bfloat16) if dtype == BF16 else t


def _inputs(case, dtype):
  """Seeded inputs scaled by (sigma D)^-1/2 and the float64 reference of every output, computed once per (case, dtype) and
  never modified.  The backward's dhist is the reference's own, rounded to float32: both sides read the same numbers."""
  key = (case, dtype)
  if key not in _cache:
    M, D, L, G = case
    n = M // G
    g = torch.Generator().manual_seed(4160 + M + L + G)
    scale = (SIGMA * D) ** -0.5
    x = hu.quantize_like((torch.rand(M, D, generator=g) * 2 - 1) * scale, dtype)
    c = (torch.rand(L, D, generator=g) * 2 - 1) * scale
    dy = hu.quantize_like(torch.randn(M, D, generator=g), dtype)
    x64, c64, dy64 = x.double(), c.double(), dy.double()
    rate_s, hist_s = ref.rate(x64, c64, SIGMA, G, DENOM)
    rate_h, hist_h = ref.rate(x64, c64, SIGMA, G, DENOM, hard=True)
    dhist = ref.dhist_of(hist_s, n, DENOM, SCALE)
    dh32 = dhist.float()
    dx, dc = ref.quantize_bwd_grouped(dy64, x64, c64, SIGMA, G, dh32.double())
    two = torch.topk(vq_util.scores(x64, c64), 2, dim=-1, largest=False).values
    decided = (two[:, 1] - two[:, 0]) > 1e-5 * two[:, 0]
    _cache[key] = (x, c, dy, dh32, bool(decided.all()),
                   dict(rate_s=rate_s.view(1), q_s=hist_s / n, rate_h=rate_h.view(1), q_h=hist_h / n, dhist=dhist, dx=dx, dc=dc))
  return _cache[key]


@pytest.mark.parametrize('dtype', hu.DTYPES)
@pytest.mark.parametrize('case', CASES, ids=str)
def test_kernels_match_fp64_and_repeat_bit_identically(case, dtype):
  M, D, L, G = case
  n = M // G
  x, c, dy, dh32, all_decided, want = _inputs(case, dtype)
  xd, cd, dyd, dhd = _dev(x, dtype), _dev(c), _dev(dy, dtype), _dev(dh32)
  # soft: hist / n, rate, dhist
  rate, hist, dhist = ops.vq_rate_fwd(xd, cd, SIGMA, G, DENOM, SCALE, want_hist=True)
  assert rate.shape == (1,) and hist.shape == (G, L) and dhist.shape == (G, L)
  assert rate.dtype == hist.dtype == dhist.dtype == torch.float32
  hu.assert_close(hist.cpu() / n, want['q_s'], TOL, 'vq_rate_fwd soft hist / n')
  hu.assert_close(rate.cpu(), want['rate_s'], TOL, 'vq_rate_fwd soft rate')
  hu.assert_close(dhist.cpu(), want['dhist'], TOL, 'vq_rate_fwd dhist')
  assert abs(float(hist.sum()) - M) <= 1e-5 * M
  # hard: the counts of the fused forward's index per group, exactly
  rate_h, hist_h, none = ops.vq_rate_fwd(xd, cd, SIGMA, G, DENOM, hard=True, want_hist=True, want_grad=False)
  assert none is None
  _, index, _ = ops.vq_quantize_fwd(xd, cd, SIGMA)
  idx = index.cpu().long()
  counts = torch.stack([torch.bincount(idx[gi::G], minlength=L) for gi in range(G)]).float()
  assert torch.equal(hist_h.cpu(), counts)
  if all_decided:          # every row's nearest centre is clear of the runner-up in float64: the reference's counts are the same
    hu.assert_close(hist_h.cpu() / n, want['q_h'], TOL, 'vq_rate_fwd hard hist / n')
    hu.assert_close(rate_h.cpu(), want['rate_h'], TOL, 'vq_rate_fwd hard rate')
  else:                    # the rate of the device's own counts, in float64
    hu.assert_close(rate_h.cpu(), ref.rate_of_hist(counts.double(), n, DENOM).view(1), TOL, 'vq_rate_fwd hard rate (own counts)')
  # outputs that were not asked for change nothing
  rate2, none_h, none_d = ops.vq_rate_fwd(xd, cd, SIGMA, G, DENOM, SCALE, want_grad=False)
  assert none_h is None and none_d is None and torch.equal(rate2, rate)
  # grouped backward with a non-zero dhist
  dx, dc = ops.vq_quantize_bwd(dyd, xd, cd, SIGMA, groups=G, dhist=dhd)
  assert dx.dtype == xd.dtype and dc.dtype == torch.float32
  _check_dx(dx, want['dx'], dtype, 'vq_quantize_bwd_grouped dx')
  hu.assert_close(dc.cpu(), want['dc'], TOL, 'vq_quantize_bwd_grouped dC')
  only_dx, none = ops.vq_quantize_bwd(dyd, xd, cd, SIGMA, want_dc=False, groups=G, dhist=dhd)
  assert none is None and torch.equal(only_dx, dx)
  # determinism: second calls on the same buffers
  rate3, hist3, dhist3 = ops.vq_rate_fwd(xd, cd, SIGMA, G, DENOM, SCALE, want_hist=True)
  dx3, dc3 = ops.vq_quantize_bwd(dyd, xd, cd, SIGMA, groups=G, dhist=dhd)
  assert torch.equal(rate, rate3) and torch.equal(hist, hist3) and torch.equal(dhist, dhist3)
  assert torch.equal(dx, dx3) and torch.equal(dc, dc3)


@pytest.mark.parametrize('dtype', hu.DTYPES)
@pytest.mark.parametrize('case', [(66, 8, 64, 2), (4112, 8, 64, 16), (4100, 8, 64, 20)], ids=str)
def test_grouped_backward_against_the_existing_one(case, dtype):
  M, D, L, G = case
  x, c, dy, _, _, _ = _inputs(case, dtype)
  xd, cd, dyd = _dev(x, dtype), _dev(c), _dev(dy, dtype)
  dpmf = torch.randn(L, generator=torch.Generator().manual_seed(M)).to(DEV)
  # one group with dhist = dpmf / M is the existing call with dpmf, up to the rounding of the division
  dx_old, dc_old = ops.vq_quantize_bwd(dyd, xd, cd, SIGMA, dpmf)
  dx_new, dc_new = ops.vq_quantize_bwd(dyd, xd, cd, SIGMA, groups=1, dhist=(dpmf / M).view(1, L).contiguous())
  _check_dx(dx_new, dx_old.float().cpu().double(), dtype, 'grouped (G = 1, dhist = dpmf / M) dx vs existing')
  hu.assert_close(dc_new.cpu(), dc_old.cpu().double(), TOL, 'grouped (G = 1, dhist = dpmf / M) dC vs existing')
  # without a dhist: the existing call's bits, for any group count and through ops' default path
  dx0, dc0 = ops.vq_quantize_bwd(dyd, xd, cd, SIGMA)
  for groups in (1, G):
    dx1, dc1 = ops.vq_quantize_bwd(dyd, xd, cd, SIGMA, groups=groups, dhist=None)
    assert torch.equal(dx1, dx0) and torch.equal(dc1, dc0), groups
  # a zero dhist adds exact zeros
  dx2, dc2 = ops.vq_quantize_bwd(dyd, xd, cd, SIGMA, groups=G, dhist=torch.zeros(G, L, device=DEV))
  assert torch.equal(dx2, dx0) and torch.equal(dc2, dc0)


@pytest.mark.parametrize('G', [4, 3], ids=['shuffle path', 'general path'])
def test_dhist_is_exactly_zero_where_hist_is_zero(G):
  """One centre so far away that its exp underflows for every vector: hist 0, dhist exactly 0, the rate unchanged by it."""
  M, D, L = 120, 4, 6
  g = torch.Generator().manual_seed(77)
  scale = (SIGMA * D) ** -0.5
  x = (torch.rand(M, D, generator=g) * 2 - 1) * scale
  c = (torch.rand(L, D, generator=g) * 2 - 1) * scale
  c[4] = 100.0
  rate, hist, dhist = ops.vq_rate_fwd(_dev(x), _dev(c), SIGMA, G, DENOM, SCALE, want_hist=True)
  hist, dhist = hist.cpu(), dhist.cpu()
  assert bool((hist[:, 4] == 0).all()) and bool((dhist[:, 4] == 0).all())
  assert bool((hist[:, :4] > 0).all()) and bool((dhist[:, :4] != 0).all())
  want, _ = ref.rate(x.double(), c.double(), SIGMA, G, DENOM)
  hu.assert_close(rate.cpu(), want.view(1), TOL, 'rate with an unused centre')
  assert bool(torch.isfinite(dhist).all())


def test_limits_are_refused_before_any_launch():
  lib = jpdse_hip.lib()
  EINVAL = -1
  M, D, Lc, G = 32, 8, 64, 4
  x = torch.zeros(M, D, device=DEV)
  c = torch.zeros(Lc, D, device=DEV)
  hist = torch.full((G, Lc), 7.0, device=DEV)
  dhist = torch.full((G, Lc), 7.0, device=DEV)
  rate = torch.full((1,), 7.0, device=DEV)
  dx = torch.full((M, D), 7.0, device=DEV)
  dc = torch.full((Lc, D), 7.0, device=DEV)
  ws = torch.zeros(max(lib.jpdse_vq_rate_workspace_size(M, D, Lc, G), lib.jpdse_vq_quantize_workspace_size(M, D, Lc)),
                   dtype=torch.uint8, device=DEV)
  st = torch.cuda.current_stream().cuda_stream
  ptr = lambda t: t.data_ptr() if t is not None else None

  def fwd(dtype=F32, M=M, D=D, Lc=Lc, G=G, sigma=1.0, x=x, c=c, scale=1.0, denom=1.0, hist=hist, rate=rate, dhist=dhist,
          ws_ptr=ws.data_ptr(), ws_bytes=ws.numel()):
    a = jpdse_hip.VqRateFwdArgs(dtype, M, D, Lc, G, sigma, 0, ptr(x), ptr(c), scale, denom, ptr(hist), ptr(rate), ptr(dhist),
                                ws_ptr, ws_bytes, st)
    return lib.jpdse_vq_rate_fwd(ctypes.byref(a))

  def bwd(dtype=F32, M=M, D=D, Lc=Lc, G=G, sigma=1.0, dy=x, x=x, c=c, dhist=dhist, dx=dx, dc=dc, ws_ptr=ws.data_ptr(),
          ws_bytes=ws.numel()):
    a = jpdse_hip.VqQuantizeBwdGroupedArgs(dtype, M, D, Lc, G, sigma, ptr(dy), ptr(x), ptr(c), ptr(dhist), ptr(dx), ptr(dc),
                                           ws_ptr, ws_bytes, st)
    return lib.jpdse_vq_quantize_bwd_grouped(ctypes.byref(a))

  need = lib.jpdse_vq_rate_workspace_size(M, D, Lc, G)
  shared = [dict(D=0), dict(D=33), dict(Lc=1), dict(Lc=513), dict(M=0), dict(M=2 ** 22, Lc=512, G=1), dict(sigma=0.0),
            dict(sigma=-1.0), dict(sigma=float('inf')), dict(sigma=float('nan')), dict(dtype=2), dict(x=None), dict(c=None),
            dict(ws_ptr=None), dict(G=0), dict(G=-4), dict(G=3), dict(G=64), dict(M=2048, Lc=64, G=2048)]
  for kw in shared + [dict(ws_bytes=need - 1), dict(rate=None), dict(denom=0.0), dict(denom=-1.0), dict(denom=float('inf')),
                      dict(denom=float('nan')), dict(scale=float('inf')), dict(scale=float('nan'))]:
    assert fwd(**kw) == EINVAL, kw
    assert jpdse_hip.last_error().startswith('vq_rate_fwd'), kw
  for kw in shared + [dict(dy=None), dict(ws_bytes=lib.jpdse_vq_quantize_workspace_size(M, D, Lc) - 1)]:
    assert bwd(**kw) == EINVAL, kw
    assert jpdse_hip.last_error().startswith('vq_quantize_bwd_grouped'), kw
  assert lib.jpdse_vq_rate_fwd(None) == EINVAL and lib.jpdse_vq_quantize_bwd_grouped(None) == EINVAL
  torch.cuda.synchronize()
  for t in (hist, dhist, rate, dx, dc):          # nothing ran: the would-be outputs still hold their fill
    assert bool((t == 7.0).all())
  # the calls themselves are accepted; hist, dhist, dx, dC are optional
  assert fwd(hist=None, dhist=None) == 0 and bwd(dc=None, ws_ptr=None, ws_bytes=0) == 0 and bwd(dx=None, dc=None) == 0
  assert fwd() == 0 and bwd() == 0
  torch.cuda.synchronize()


# ---- the module --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', hu.DTYPES)
def test_module_rate_gives_the_fp64_gradients(dtype):
  """S2HVQ.rate(...).backward() against float64 autograd of the restatement, alone and inside a loss with quantize; one group
  against the module's own get_pmf / get_cross_entropy."""
  from ctu.quantizers import S2HVQ
  n, code_len, D, L, G = 36, 4, 8, 16, 4
  M = n * code_len
  g = torch.Generator().manual_seed(16)
  scale = (SIGMA * D) ** -0.5
  x = hu.quantize_like((torch.rand(n, code_len * D, generator=g) * 2 - 1) * scale, dtype)
  c = (torch.rand(L, D, generator=g) * 2 - 1) * scale
  x64, c64 = x.double().view(-1, D).requires_grad_(True), c.double().requires_grad_(True)
  value64, _ = ref.rate(x64, c64, SIGMA, G, float(M))
  (3.0 * value64).backward()
  vq = S2HVQ(c.clone(), sigma=SIGMA).to(DEV)
  xd = _dev(x, dtype).requires_grad_(True)
  value = vq.rate(xd, code_len, groups=G)
  assert value.dim() == 0 and value.dtype == torch.float32 and value.requires_grad
  hu.assert_close(value.detach().cpu().view(1), value64.detach().view(1), TOL, 'module rate')
  (3.0 * value).backward()
  _check_dx(xd.grad.view(-1, D), x64.grad, dtype, 'module rate dx')
  hu.assert_close(vq.code_book.grad.cpu(), c64.grad, TOL, 'module rate dC')
  # hard: the same gradient (the soft form's), the entropy of the hard code as the value
  vq.code_book.grad = None
  xh = _dev(x, dtype).requires_grad_(True)
  hard = vq.rate(xh, code_len, groups=G, hard=True)
  want_h, _ = ref.rate(x64.detach(), c64.detach(), SIGMA, G, float(M), hard=True)
  hu.assert_close(hard.detach().cpu().view(1), want_h.view(1), TOL, 'module hard rate')
  # one group: the module's own pmf and cross entropy
  with torch.no_grad():
    one = vq.rate(_dev(x, dtype), code_len, groups=1)
    assert not one.requires_grad
    pmf = S2HVQ.get_pmf(vq.encode(_dev(x, dtype), code_len, train=True, raw=True))
    ce = S2HVQ.get_cross_entropy(pmf, pmf)
  hu.assert_close(one.cpu().view(1), ce.cpu().double().view(1), TOL, 'rate (G = 1) vs get_cross_entropy(get_pmf)')
  with pytest.raises(ValueError, match='groups must divide'):
    vq.rate(_dev(x, dtype), code_len, groups=7)
  with pytest.raises(ValueError, match='denom'):
    vq.rate(_dev(x, dtype), code_len, denom=0.0)
