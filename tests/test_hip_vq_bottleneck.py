"""GPU tests of the vector-quantizer bottleneck kernels (vq_bottleneck.hip, ops.vq_quantize_fwd / _bwd, S2HVQ.quantize;
DESIGN.md 4.15) against the float64 restatement tests/vq_bottleneck_ref.py, the exact contracts (the gather, integer inputs,
the tie rule), determinism, a saturated sigma, the refusals and the module's autograd.

Shapes (M, D, L): (1, 1, 2) one vector; (65, 8, 64) one past a wave; (257, 3, 5) odd D, an L that is no power of two, one past a
256-thread block; (300, 32, 512) both limits at once, a 64 KiB code book (read from global memory, 64-vector tiles); (4099, 8, 64)
several blocks with a ragged last tile for the dC and pmf merges."""
import ctypes

import pytest
import torch

import jpdse_hip
from jpdse_hip import ops, F32, BF16
import hip_util as hu
import vq_util
import vq_bottleneck_ref as ref
from test_hip_quantizers import _check_dx, _integer_inputs

pytestmark = pytest.mark.gpu
DEV = hu.DEV
TOL = hu.RTOL[F32]          # with ETOL[F32] through hip_util.assert_close
SIGMA = 10.0
GAP = 1e-5                  # rows whose two nearest centres are closer than GAP * the nearest score are not held to the fp64 index
SHAPES = [(1, 1, 2), (65, 8, 64), (257, 3, 5), (300, 32, 512), (4099, 8, 64)]
_cache = {}


def _dev(t, dtype=None):
  t = t.to(DEV)
  return t.to(torch.bfloat16) if dtype == BF16 else t


def _decided(x64, c64):
  """Rows whose float64 nearest centre is ahead of the runner-up by more than GAP times its score."""
  two = torch.topk(vq_util.scores(x64, c64), 2, dim=-1, largest=False).values
  return (two[:, 1] - two[:, 0]) > GAP * two[:, 0]


def _inputs(shape, dtype):
  """Seeded inputs, scaled by (sigma D)^-1/2 as the fixture of 4.13, and the float64 reference of every output; computed once
  per (shape, dtype) and never modified.  The seed is the first, counted up from a base, whose float64 reference alone leaves
  fewer than 1 % of the rows undecided."""
  key = (shape, dtype)
  if key not in _cache:
    M, D, L = shape
    scale = (SIGMA * D) ** -0.5
    for seed in range(4150 + M + L, 4150 + M + L + 50):
      g = torch.Generator().manual_seed(seed)
      x = hu.quantize_like((torch.rand(M, D, generator=g) * 2 - 1) * scale, dtype)
      c = (torch.rand(L, D, generator=g) * 2 - 1) * scale
      decided = _decided(x.double(), c.double())
      if int((~decided).sum()) < 0.01 * M:
        break
    assert int((~decided).sum()) < 0.01 * M, 'no seed leaves fewer than 1 %% of the rows undecided for %s' % (shape,)
    dy = hu.quantize_like(torch.randn(M, D, generator=g), dtype)
    dpmf = torch.randn(L, generator=g)
    x64, c64, dy64 = x.double(), c.double(), dy.double()
    y_soft, index, pmf = ref.quantize_fwd(x64, c64, SIGMA, hard_forward=False)
    dx, dc = ref.quantize_bwd(dy64, x64, c64, SIGMA, dpmf.double())
    dx0, dc0 = ref.quantize_bwd(dy64, x64, c64, SIGMA, None)
    _cache[key] = (x, c, dy, dpmf, decided, dict(y=y_soft, index=index, pmf=pmf, dx=dx, dc=dc, dx0=dx0, dc0=dc0))
  return _cache[key]


@pytest.mark.parametrize('dtype', hu.DTYPES)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_kernels_match_fp64_and_repeat_bit_identically(shape, dtype):
  M, D, L = shape
  x, c, dy, dpmf, decided, want = _inputs(shape, dtype)
  xd, cd, dyd, dpmfd = _dev(x, dtype), _dev(c), _dev(dy, dtype), _dev(dpmf)
  # soft forward with a pmf
  y, index, pmf = ops.vq_quantize_fwd(xd, cd, SIGMA, hard_forward=False, want_pmf=True)
  assert y.dtype == xd.dtype and index.dtype == torch.int32 and pmf.dtype == torch.float32
  _check_dx(y, want['y'], dtype, 'vq_quantize_fwd soft y')
  hu.assert_close(pmf.cpu(), want['pmf'], TOL, 'vq_quantize_fwd pmf')
  got = index.cpu().long()
  assert bool(((got >= 0) & (got < L)).all())
  assert torch.equal(got[decided], want['index'][decided]), 'index differs from float64 on a decided row'
  # hard forward: the same index, a bit-exact gather, the same pmf whether asked with it or without
  yh, index_h, none = ops.vq_quantize_fwd(xd, cd, SIGMA, hard_forward=True)
  assert none is None and torch.equal(index_h, index)
  gathered = c[got]
  assert torch.equal(yh.cpu(), gathered.to(torch.bfloat16) if dtype == BF16 else gathered)
  yh2, index_h2, pmf_h = ops.vq_quantize_fwd(xd, cd, SIGMA, hard_forward=True, want_pmf=True)
  assert torch.equal(yh2, yh) and torch.equal(index_h2, index) and torch.equal(pmf_h, pmf)
  # backward, with and without a gradient on the pmf
  dx, dc = ops.vq_quantize_bwd(dyd, xd, cd, SIGMA, dpmfd)
  assert dx.dtype == xd.dtype and dc.dtype == torch.float32
  _check_dx(dx, want['dx'], dtype, 'vq_quantize_bwd dx')
  hu.assert_close(dc.cpu(), want['dc'], TOL, 'vq_quantize_bwd dC')
  dx0, dc0 = ops.vq_quantize_bwd(dyd, xd, cd, SIGMA)
  _check_dx(dx0, want['dx0'], dtype, 'vq_quantize_bwd dx (no dpmf)')
  hu.assert_close(dc0.cpu(), want['dc0'], TOL, 'vq_quantize_bwd dC (no dpmf)')
  only_dx, none = ops.vq_quantize_bwd(dyd, xd, cd, SIGMA, dpmfd, want_dc=False)
  none2, only_dc = ops.vq_quantize_bwd(dyd, xd, cd, SIGMA, dpmfd, want_dx=False)
  assert none is None and none2 is None and torch.equal(only_dx, dx) and torch.equal(only_dc, dc)
  # determinism: a second call on the same buffers
  y2, index2, pmf2 = ops.vq_quantize_fwd(xd, cd, SIGMA, hard_forward=False, want_pmf=True)
  dx2, dc2 = ops.vq_quantize_bwd(dyd, xd, cd, SIGMA, dpmfd)
  assert torch.equal(y, y2) and torch.equal(index, index2) and torch.equal(pmf, pmf2)
  assert torch.equal(dx, dx2) and torch.equal(dc, dc2)


@pytest.mark.parametrize('dtype', hu.DTYPES)
@pytest.mark.parametrize('shape', [(1, 1, 2), (65, 8, 64), (257, 3, 5), (300, 32, 512)], ids=str)
def test_integer_inputs_are_bit_exact(shape, dtype):
  M, D, L = shape
  x, c = _integer_inputs(M, D, L, seed=91 + M + L)
  two = torch.topk(vq_util.scores(x, c), 2, dim=-1, largest=False).values
  assert bool((two[:, 0] < two[:, 1]).all()), 'the nearest centre is not unique'
  want = vq_util.hard_index(x, c)
  xd, cd = _dev(x, dtype), _dev(c)                # integers up to 8 are exact in bf16
  for hard in (True, False):
    y, index, _ = ops.vq_quantize_fwd(xd, cd, SIGMA, hard_forward=hard)
    assert torch.equal(index.cpu().long(), want)
    if hard:
      assert y.dtype == xd.dtype and torch.equal(y.float().cpu(), vq_util.decode(want, c))


def test_ties_go_to_the_lowest_index():
  """Against the stated rule: equal scores inside one LDS chunk of 16 centres, across chunks, and everywhere."""
  c = torch.full((130, 1), 3.0)
  c[[5, 70, 129], 0] = torch.tensor([1.0, -1.0, 1.0])          # three nearest at distance 1
  x = torch.zeros(3, 1)
  y, index, _ = ops.vq_quantize_fwd(_dev(x), _dev(c), SIGMA)
  assert index.cpu().tolist() == [5, 5, 5] and torch.equal(y.cpu(), torch.ones(3, 1))
  c[5, 0] = 2.0                                                 # now 70 and 129 tie
  y, index, _ = ops.vq_quantize_fwd(_dev(x), _dev(c), SIGMA)
  assert index.cpu().tolist() == [70, 70, 70] and torch.equal(y.cpu(), -torch.ones(3, 1))
  c[[6, 7], 0] = torch.tensor([-1.0, 1.0])                      # 6 and 7 join: the lowest of one chunk
  assert ops.vq_quantize_fwd(_dev(x), _dev(c), SIGMA)[1].cpu().tolist() == [6, 6, 6]
  same = torch.ones(7, 2)                                       # all equal: centre 0, and a uniform soft row
  y, index, pmf = ops.vq_quantize_fwd(_dev(torch.zeros(2, 2)), _dev(same), SIGMA, hard_forward=False, want_pmf=True)
  assert index.cpu().tolist() == [0, 0]
  assert float((pmf.cpu() - 1.0 / 7).abs().max()) <= 1e-7 and float((y.cpu() - 1).abs().max()) <= 1e-6
  # a NaN never wins; a row of NaNs still gives an index inside the code book
  xn = torch.tensor([[float('nan'), 0.0], [0.0, 0.0]])
  cn = torch.tensor([[float('nan'), 0.0], [2.0, 0.0], [1.0, 0.0]])
  assert ops.vq_quantize_fwd(_dev(xn), _dev(cn), SIGMA)[1].cpu().tolist()[1] == 2
  assert 0 <= ops.vq_quantize_fwd(_dev(xn), _dev(cn), SIGMA)[1].cpu().tolist()[0] < 3


@pytest.mark.parametrize('dtype', hu.DTYPES)
def test_large_sigma_is_finite(dtype):
  g = torch.Generator().manual_seed(9)
  x, c = _dev(torch.randn(300, 8, generator=g), dtype), _dev(torch.randn(64, 8, generator=g))
  dy, dpmf = _dev(torch.randn(300, 8, generator=g), dtype), _dev(torch.randn(64, generator=g))
  y, index, pmf = ops.vq_quantize_fwd(x, c, 1e4, hard_forward=False, want_pmf=True)
  dx, dc = ops.vq_quantize_bwd(dy, x, c, 1e4, dpmf)
  for t in (y, pmf, dx, dc):
    assert bool(torch.isfinite(t.float()).all())
  assert abs(float(pmf.sum()) - 1) <= 1e-5
  # finite inputs whose scores overflow float32: still finite, the row uniform
  y, index, pmf = ops.vq_quantize_fwd(torch.full((2, 4), 3e19, device=DEV), torch.zeros(3, 4, device=DEV), 0.5,
                                      hard_forward=False, want_pmf=True)
  assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(pmf).all()) and index.cpu().tolist() == [0, 0]


def test_limits_are_refused_before_any_launch():
  L = jpdse_hip.lib()
  EINVAL = -1
  M, D, Lc = 16, 8, 64
  x = torch.zeros(M, D, device=DEV)
  c = torch.zeros(Lc, D, device=DEV)
  y = torch.full((M, D), 7.0, device=DEV)
  index = torch.full((M,), 7, dtype=torch.int32, device=DEV)
  pmf = torch.full((Lc,), 7.0, device=DEV)
  dc = torch.full((Lc, D), 7.0, device=DEV)
  ws = torch.zeros(L.jpdse_vq_quantize_workspace_size(M, D, Lc), dtype=torch.uint8, device=DEV)
  st = torch.cuda.current_stream().cuda_stream
  ptr = lambda t: t.data_ptr() if t is not None else None

  def fwd(dtype=F32, M=M, D=D, Lc=Lc, sigma=1.0, x=x, c=c, y=y, index=index, pmf=pmf, ws_ptr=ws.data_ptr(), ws_bytes=ws.numel()):
    a = jpdse_hip.VqQuantizeFwdArgs(dtype, M, D, Lc, sigma, 1, ptr(x), ptr(c), ptr(y), ptr(index), ptr(pmf), ws_ptr, ws_bytes, st)
    return L.jpdse_vq_quantize_fwd(ctypes.byref(a))

  def bwd(dtype=F32, M=M, D=D, Lc=Lc, sigma=1.0, dy=x, x=x, c=c, dx=y, dc=dc, ws_ptr=ws.data_ptr(), ws_bytes=ws.numel()):
    a = jpdse_hip.VqQuantizeBwdArgs(dtype, M, D, Lc, sigma, ptr(dy), ptr(x), ptr(c), None, ptr(dx), ptr(dc), ws_ptr, ws_bytes, st)
    return L.jpdse_vq_quantize_bwd(ctypes.byref(a))

  shared = [dict(D=0), dict(D=33), dict(Lc=1), dict(Lc=513), dict(M=0), dict(M=2 ** 22, Lc=512), dict(sigma=0.0), dict(sigma=-1.0),
            dict(sigma=float('inf')), dict(sigma=float('nan')), dict(dtype=2), dict(x=None), dict(c=None), dict(ws_ptr=None),
            dict(ws_bytes=ws.numel() - 1)]
  for kw in shared + [dict(y=None), dict(index=None)]:
    assert fwd(**kw) == EINVAL, kw
    assert jpdse_hip.last_error().startswith('vq_quantize_fwd'), kw
  for kw in shared + [dict(dy=None)]:
    assert bwd(**kw) == EINVAL, kw
    assert jpdse_hip.last_error().startswith('vq_quantize_bwd'), kw
  assert L.jpdse_vq_quantize_fwd(None) == EINVAL and L.jpdse_vq_quantize_bwd(None) == EINVAL
  torch.cuda.synchronize()
  # nothing ran: the would-be outputs still hold their fill
  assert bool((y == 7.0).all()) and bool((index == 7).all()) and bool((pmf == 7.0).all()) and bool((dc == 7.0).all())
  # without a pmf / a code-book gradient no workspace is needed
  assert fwd(pmf=None, ws_ptr=None, ws_bytes=0) == 0 and bwd(dc=None, ws_ptr=None, ws_bytes=0) == 0
  assert fwd() == 0 and bwd() == 0 and bwd(dx=None, dc=None) == 0


# ---- the module --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', hu.DTYPES)
def test_module_quantize_gives_the_fp64_gradients(dtype):
  """loss = sum(y * q) + sum(pmf * r) through S2HVQ.quantize: the gradients on x and the code book are float64 autograd's of the
  soft form, and the same bits whether the forward was hard or soft."""
  from ctu.quantizers import S2HVQ
  n, code_len, D, L = 37, 5, 8, 64
  g = torch.Generator().manual_seed(15)
  scale = (SIGMA * D) ** -0.5
  x = hu.quantize_like((torch.rand(n, code_len * D, generator=g) * 2 - 1) * scale, dtype)
  c = (torch.rand(L, D, generator=g) * 2 - 1) * scale
  q = hu.quantize_like(torch.randn(n, code_len * D, generator=g), dtype)
  r = torch.randn(L, generator=g)
  x64, c64 = x.double().view(-1, D).requires_grad_(True), c.double().requires_grad_(True)
  y64, pmf64 = ref.soft_value(x64, c64, SIGMA)
  ((y64 * q.double().view(-1, D)).sum() + (pmf64 * r.double()).sum()).backward()
  grads = {}
  for hard in (True, False):
    vq = S2HVQ(c.clone(), sigma=SIGMA).to(DEV)
    xd = _dev(x, dtype).requires_grad_(True)
    y, code, pmf = vq.quantize(xd, code_len, hard_forward=hard, want_pmf=True)
    assert y.shape == (n, code_len * D) and y.dtype == xd.dtype and code.shape == (n, code_len) and code.dtype == torch.int64
    decided = _decided(x64.detach(), c64.detach())
    assert torch.equal(code.view(-1).cpu()[decided], vq_util.hard_index(x64.detach(), c64.detach())[decided])
    if hard:
      book = vq.code_book.detach().cpu()[code.view(-1).cpu()]
      assert torch.equal(y.detach().view(-1, D).cpu(), book.to(torch.bfloat16) if dtype == BF16 else book)
    hu.assert_close(pmf.detach().cpu(), pmf64.detach(), TOL, 'module pmf')
    ((y.float() * _dev(q).float()).sum() + (pmf * _dev(r)).sum()).backward()
    _check_dx(xd.grad.view(-1, D), x64.grad, dtype, 'module dx (hard_forward=%s)' % hard)
    hu.assert_close(vq.code_book.grad.cpu(), c64.grad, TOL, 'module dC (hard_forward=%s)' % hard)
    grads[hard] = (xd.grad.clone(), vq.code_book.grad.clone())
    # without a pmf the third output is None and the gradient is dy's alone
    y2, code2, none = vq.quantize(xd, code_len, hard_forward=hard)
    assert none is None and torch.equal(y2, y) and torch.equal(code2, code)
  assert torch.equal(grads[True][0], grads[False][0]) and torch.equal(grads[True][1], grads[False][1])
  # eval mode: always the hard forward, nothing saved
  vq.eval()
  ye, codee, _ = vq.quantize(_dev(x, dtype).requires_grad_(True), code_len, hard_forward=False)
  assert not ye.requires_grad and torch.equal(codee, code)
  book = vq.code_book.detach().cpu()[codee.view(-1).cpu()]
  assert torch.equal(ye.view(-1, D).cpu(), book.to(torch.bfloat16) if dtype == BF16 else book)
  with pytest.raises(ValueError, match='code_len must divide'):
    vq.quantize(_dev(x, dtype), 7)
