"""GPU tests of the soft-to-hard vector quantizer (vq.hip, ctu.quantizers.S2HVQ) against the torch-CPU
restatement tests/vq_util.py in float64, the exact contracts (integer inputs, the tie rule, pmf of one-hots), the reference's
golden fixture, autograd through a reference-style loop, determinism and the guards.

Shapes: M in {1, 63, 64, 65, 1025} (one lane, the wave's edges, several blocks), D in {1, 3, 8, 32}, L in {2, 10, 64, 257, 512},
sigma in {0.5, 10, 1e4}; every value appears, and so does the corner (1025, 32, 512).  A block of the code-book gradients covers
at most 64 vectors (soft) or 256 (decode) per tile and pmf at most 64 rows per block, so M = 1025 merges at least 5 partials."""
import ctypes

import numpy as np
import os
import pytest
import torch

import jpdse_hip
from jpdse_hip import ops, F32, BF16
import hip_util as hu
import vq_util

pytestmark = pytest.mark.gpu
DEV = hu.DEV
TOL = hu.RTOL[F32]          # with ETOL[F32] through hip_util.assert_close

# name, M, D, L, sigma
CASES = [('one', 1, 1, 2, 0.5), ('m63', 63, 3, 10, 10.), ('m64', 64, 8, 64, 1e4), ('m65', 65, 32, 257, 0.5),
         ('corner', 1025, 32, 512, 10.), ('bench-like', 1025, 8, 64, 10.), ('two-centres', 65, 8, 2, 1e4)]
_ref_cache = {}


def _inputs(name, M, D, L, sigma, dtype):
  """Seeded inputs and the float64 reference of every kernel, computed once per (case, dtype) and never modified.  x and the
  centres are uniform in (-1, 1) times (sigma D)^-1/2, so every logit sigma d lies in [0, 4]: no entry of a row is below
  e^-4 / L.  The gradient p (dp - <p, dp>) is a difference that cancels to the size of the row's smallest entries; float32
  holds it to the fp32 pair while those are >= 1e-4, and with a single vector (M = 1) nothing else sets the scale the error is
  measured against.  A saturated row is the subject of test_large_sigma_is_finite."""
  key = (name, dtype)
  if key not in _ref_cache:
    g = torch.Generator().manual_seed(1000 + sum(ord(ch) for ch in name))
    scale = (sigma * D) ** -0.5
    x = hu.quantize_like((torch.rand(M, D, generator=g) * 2 - 1) * scale, dtype)
    c = (torch.rand(L, D, generator=g) * 2 - 1) * scale
    dp = torch.randn(M, L, generator=g)
    idx = torch.randint(0, L, (M,), generator=g, dtype=torch.int32)
    dy = hu.quantize_like(torch.randn(M, D, generator=g), dtype)
    dpmf = torch.randn(L, generator=g)
    x64, c64 = x.double(), c.double()
    p = vq_util.soft(x64, c64, sigma)
    dx, dc = vq_util.soft_bwd(dp.double(), p, x64, c64, sigma)
    ref = dict(p=p, dx=dx, dc=dc, pmf=vq_util.pmf(p), ddec=vq_util.decode_bwd(idx, dy.double(), L),
               ds=(dpmf.double() / M).expand(M, L))
    _ref_cache[key] = (x, c, dp, idx, dy, dpmf, ref)
  return _ref_cache[key]


def _dev(t, dtype=None):
  t = t.to(DEV)
  return t.to(torch.bfloat16) if dtype == BF16 else t


def _bf16_ulp(b):
  b = b.abs().clamp_min(2.0 ** -126)
  return torch.pow(2.0, torch.floor(torch.log2(b)) - 7)


def _check_dx(dx, ref, dtype, what):
  if dtype == F32:
    hu.assert_close(dx.float().cpu(), ref, TOL, what)
    return
  # bf16 storage: the fp32 pair plus one bf16 ulp of the value for the final rounding
  a, b = dx.float().cpu().double(), ref
  bound = hu.ETOL[F32] * (b.pow(2).mean().sqrt() + b.abs()) + _bf16_ulp(b)
  worst = ((a - b).abs() / bound).max().item()
  hu.record(what + ' [fp32 pair + 1 bf16 ulp, fraction of bound]', worst, 1.0)
  assert worst <= 1.0, '%s: %.3f of the bound' % (what, worst)


@pytest.mark.parametrize('dtype', hu.DTYPES)
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_kernels_match_fp64_and_repeat_bit_identically(case, dtype):
  name, M, D, L, sigma = case
  x, c, dp, idx, dy, dpmf, ref = _inputs(name, M, D, L, sigma, dtype)
  xd, cd, dpd, idxd, dyd, dpmfd = _dev(x, dtype), _dev(c), _dev(dp), _dev(idx), _dev(dy, dtype), _dev(dpmf)
  p = ops.vq_soft_fwd(xd, cd, sigma)
  hu.assert_close(p.cpu(), ref['p'], TOL, 'vq_soft_fwd p')
  # the backward consumes the device's own p, as autograd does
  dx, dc = ops.vq_soft_bwd(dpd, p, xd, cd, sigma)
  assert dx.dtype == xd.dtype and dc.dtype == torch.float32
  _check_dx(dx, ref['dx'], dtype, 'vq_soft_bwd dx')
  hu.assert_close(dc.cpu(), ref['dc'], TOL, 'vq_soft_bwd dC')
  only_dx, none = ops.vq_soft_bwd(dpd, p, xd, cd, sigma, want_dc=False)
  none2, only_dc = ops.vq_soft_bwd(dpd, p, xd, cd, sigma, want_dx=False)
  assert none is None and none2 is None and torch.equal(only_dx, dx) and torch.equal(only_dc, dc)
  pmf = ops.vq_pmf(p)
  hu.assert_close(pmf.cpu(), ref['pmf'], TOL, 'vq_pmf')
  ds = ops.vq_pmf_bwd(dpmfd, M)
  hu.assert_close(ds.cpu(), ref['ds'], TOL, 'vq_pmf_bwd')
  ddec, status = ops.vq_decode_bwd(idxd, dyd, L)
  hu.assert_close(ddec.cpu(), ref['ddec'], TOL, 'vq_decode_bwd dC')
  assert int(status.item()) == 0
  # determinism: a second call on the same buffers
  p2 = ops.vq_soft_fwd(xd, cd, sigma)
  dx2, dc2 = ops.vq_soft_bwd(dpd, p, xd, cd, sigma)
  assert torch.equal(p, p2) and torch.equal(dx, dx2) and torch.equal(dc, dc2)
  assert torch.equal(pmf, ops.vq_pmf(p)) and torch.equal(ddec, ops.vq_decode_bwd(idxd, dyd, L)[0])


# ---- exact contracts -------------------------------------------------------------------------------------------------------
def _integer_inputs(M, D, L, seed):
  """Integer-valued x and centres, |value| <= 8: every score is an exact float32 integer.  L <= 64: vectors are drawn by
  rejection until NO two centres are equidistant from any of them.  L >= 257: 257 or more distinct integer scores per vector
  are out of reach of rejection sampling at |value| <= 8, so there only the nearest centre must be unique -- the one
  property the index depends on."""
  g = torch.Generator().manual_seed(seed)
  c = torch.randint(-8, 9, (L, D), generator=g).float()
  while torch.unique(c, dim=0).shape[0] != L:
    c = torch.randint(-8, 9, (L, D), generator=g).float()
  rows = []
  have = 0
  for _ in range(200):
    cand = torch.randint(-8, 9, (4096, D), generator=g).float()
    d = vq_util.scores(cand, c)
    if L <= 64:
      srt = d.sort(dim=-1).values
      keep = (srt[:, 1:] != srt[:, :-1]).all(dim=-1)
    else:
      two = torch.topk(d, 2, dim=-1, largest=False).values
      keep = two[:, 0] < two[:, 1]
    rows.append(cand[keep])
    have += int(keep.sum())
    if have >= M:
      break
  x = torch.cat(rows)[:M]
  assert x.shape[0] == M, 'no %d tie-free vectors for D %d, L %d' % (M, D, L)
  return x, c


@pytest.mark.parametrize('dtype', hu.DTYPES)
@pytest.mark.parametrize('shape', [(1, 2, 2), (63, 3, 10), (65, 8, 64), (64, 32, 257), (1025, 32, 512)], ids=str)
def test_integer_inputs_are_bit_exact(shape, dtype):
  M, D, L = shape
  x, c = _integer_inputs(M, D, L, seed=77 + M + L)
  d = vq_util.scores(x, c)
  if L <= 64:
    srt = d.sort(dim=-1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), 'two centres equidistant from a vector'
  two = torch.topk(d, 2, dim=-1, largest=False).values
  assert bool((two[:, 0] < two[:, 1]).all()), 'the nearest centre is not unique'
  want = vq_util.hard_index(x, c)
  xd, cd = _dev(x, dtype), _dev(c)                # integers up to 8 are exact in bf16
  index, onehot = ops.vq_hard_fwd(xd, cd, want_onehot=True)
  assert index.dtype == torch.int32 and torch.equal(index.cpu().long(), want)
  assert torch.equal(onehot.cpu(), vq_util.onehot(want, L))
  assert torch.equal(ops.vq_hard_fwd(xd, cd)[0], index)
  assert torch.equal(ops.vq_argmax(onehot).cpu().long(), want)
  s = -d                                            # distinct integers per row (L <= 64) or a unique maximum
  assert torch.equal(ops.vq_argmax(s.to(DEV).contiguous()).cpu().long(), vq_util.argmax_lowest(s))
  out_dtype = torch.bfloat16 if dtype == BF16 else torch.float32
  y, status = ops.vq_decode(index, cd, out_dtype)
  assert y.dtype == out_dtype and torch.equal(y.float().cpu(), vq_util.decode(want, c)) and int(status.item()) == 0


def test_ties_go_to_the_lowest_index():
  """Against the stated rule, not against torch: equal scores within a lane's centres, across lanes and across waves' slots."""
  # D = 1, x = 0: the score of centre k is c[k]^2
  c = torch.full((130, 1), 3.0)
  c[[5, 70, 129], 0] = torch.tensor([1.0, -1.0, 1.0])          # three nearest at distance 1: slots 0, 1 and 2 of lanes 5, 6, 1
  x = torch.zeros(3, 1)
  index, onehot = ops.vq_hard_fwd(_dev(x), _dev(c), want_onehot=True)
  assert index.cpu().tolist() == [5, 5, 5]
  assert onehot.cpu().sum().item() == 3 and bool((onehot.cpu()[:, 5] == 1).all())
  c[5, 0] = 2.0                                                 # now 70 and 129 tie
  assert ops.vq_hard_fwd(_dev(x), _dev(c))[0].cpu().tolist() == [70, 70, 70]
  same = torch.ones(7, 2)                                       # all equal: centre 0
  assert ops.vq_hard_fwd(_dev(torch.zeros(2, 2)), _dev(same))[0].cpu().tolist() == [0, 0]
  s = torch.zeros(4, 200)
  s[0, [199, 64, 3]] = 2.0
  s[1, [199, 64]] = 2.0
  s[2, 199] = 2.0
  assert ops.vq_argmax(_dev(s)).cpu().tolist() == [3, 64, 199, 0]
  # a soft row whose scores all tie is uniform, exactly
  p = ops.vq_soft_fwd(_dev(torch.zeros(2, 2)), _dev(torch.ones(8, 2)), 10.)
  assert torch.equal(p.cpu(), torch.full((2, 8), 0.125))


@pytest.mark.parametrize('L', [2, 10, 64, 257, 512])
def test_pmf_of_one_hots_is_exact(L):
  M = 1024
  index = torch.randint(0, L, (M,), generator=torch.Generator().manual_seed(L))
  pmf = ops.vq_pmf(_dev(vq_util.onehot(index, L)))
  assert torch.equal(pmf.cpu(), torch.bincount(index, minlength=L).float() / M)


# ---- the module --------------------------------------------------------------------------------------------------------------
def _golden(golden_dir):
  z = np.load(os.path.join(golden_dir, 's2hvq.npz'))
  n = len({k.split('_')[0] for k in z.files})
  return [{k[len('c%d_' % i):]: torch.from_numpy(z[k]) for k in z.files if k.startswith('c%d_' % i)} for i in range(n)]


def test_module_reproduces_the_reference_golden(golden_dir):
  from ctu.quantizers import S2HVQ
  for i, gold in enumerate(_golden(golden_dir)):
    n, d, code_len, L = (int(v) for v in gold['cfg'][:4])
    sigma = float(gold['cfg'][4])
    vq = S2HVQ(gold['code_book'].clone(), sigma=sigma).to(DEV)
    assert list(vq.state_dict().keys()) == ['_code_book']
    x = gold['x'].to(DEV).requires_grad_(True)
    soft = vq.encode(x, code_len)
    assert soft.shape == (n, code_len, L) and soft.dtype == torch.float32
    dec = vq.decode(soft)
    assert dec.shape == (n, d) and dec.dtype == torch.float32
    ((soft * gold['r'].to(DEV)).sum() + (dec * gold['q'].to(DEV)).sum()).backward()
    tag = 'golden %d ' % i
    hu.assert_close(soft.detach().cpu(), gold['soft'], TOL, tag + 'soft code_raw')
    hu.assert_close(x.grad.cpu(), gold['gx'], TOL, tag + 'dx')
    hu.assert_close(vq.code_book.grad.cpu(), gold['gc'], TOL, tag + 'dC')
    assert torch.equal(dec.detach().cpu(), gold['decode'])
    x2 = gold['x'].to(DEV).requires_grad_(True)
    pmf = S2HVQ.get_pmf(vq.encode(x2, code_len))
    (pmf * torch.arange(L, dtype=torch.float32, device=DEV)).sum().backward()
    hu.assert_close(pmf.detach().cpu(), gold['pmf'], TOL, tag + 'pmf')
    hu.assert_close(x2.grad.cpu(), gold['gpmf_x'], TOL, tag + 'd pmf / dx')
    vq.eval()
    with torch.no_grad():
      xe = gold['x'].to(DEV)
      hard = vq.encode(xe, code_len, train=False)
      assert hard.dtype == torch.float32 and torch.equal(hard.cpu(), gold['hard'])
      code = vq.encode(xe, code_len, train=False, raw=False)
      assert code.dtype == torch.int64 and torch.equal(code.cpu(), gold['hard_code'])
      assert torch.equal(vq.encode(xe, code_len, raw=False).cpu(), gold['soft_code'])
      assert torch.equal(vq.decode(hard).cpu(), gold['decode_hard'])
      pmf_hard = S2HVQ.get_pmf(hard)
      hu.assert_close(pmf_hard.cpu(), gold['pmf_hard'], TOL, tag + 'pmf of the hard code')
      xent = torch.stack([S2HVQ.get_cross_entropy(pmf.detach(), pmf.detach()), S2HVQ.get_cross_entropy(pmf_hard, pmf.detach())])
      hu.assert_close(xent.cpu(), gold['xent'], TOL, tag + 'cross entropy')


@pytest.mark.parametrize('dtype', hu.DTYPES)
def test_reference_style_loop_gives_the_fp64_gradients(dtype):
  """loss = H(pmf, pmf) + sum(decode(code_raw) * q) + sum(code_raw * r): backward through encode -> get_pmf ->
  get_cross_entropy plus decode."""
  from ctu.quantizers import S2HVQ
  n, code_len, D, L, sigma = 37, 5, 8, 64, 10.
  g = torch.Generator().manual_seed(5)
  scale = (sigma * D) ** -0.5
  x = hu.quantize_like(torch.randn(n, code_len * D, generator=g) * scale, dtype)
  c = torch.randn(L, D, generator=g) * scale
  r = torch.randn(n, code_len, L, generator=g) * 0.01
  q = torch.randn(n, code_len * D, generator=g)
  x64, c64 = x.double().requires_grad_(True), c.double().requires_grad_(True)
  raw64 = vq_util.encode(x64, c64, code_len, sigma)
  pm64 = vq_util.pmf(raw64)
  (vq_util.cross_entropy(pm64, pm64) + (vq_util.decode_raw(raw64, c64) * q.double()).sum() + (raw64 * r.double()).sum()).backward()
  vq = S2HVQ(c.clone(), sigma=sigma).to(DEV)
  xd = _dev(x, dtype).requires_grad_(True)
  raw = vq.encode(xd, code_len)
  pm = S2HVQ.get_pmf(raw)
  loss = S2HVQ.get_cross_entropy(pm, pm) + (vq.decode(raw) * q.to(DEV)).sum() + (raw * r.to(DEV)).sum()
  loss.backward()
  hu.assert_close(pm.detach().cpu(), pm64.detach(), TOL, 'loop pmf')
  _check_dx(xd.grad.view(-1, D), x64.grad.view(-1, D), dtype, 'loop dx')
  hu.assert_close(vq.code_book.grad.cpu(), c64.grad, TOL, 'loop dC')


def test_large_sigma_is_finite():
  from ctu.quantizers import S2HVQ
  g = torch.Generator().manual_seed(9)
  vq = S2HVQ(torch.randn(64, 8, generator=g), sigma=1e4).to(DEV)
  x = torch.randn(65, 24, generator=g).to(DEV).requires_grad_(True)
  raw = vq.encode(x, 3)
  assert bool(torch.isfinite(raw).all())
  assert float((raw.detach().sum(dim=-1) - 1).abs().max()) <= 1e-6
  pm = S2HVQ.get_pmf(raw)
  (S2HVQ.get_cross_entropy(pm, pm) + vq.decode(raw).pow(2).sum() + (raw * torch.randn(raw.shape, generator=g).to(DEV)).sum()).backward()
  assert bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(vq.code_book.grad).all())
  # finite inputs whose scores overflow float32: still a finite row that sums to 1
  p = ops.vq_soft_fwd(torch.full((2, 4), 3e19, device=DEV), torch.zeros(3, 4, device=DEV), 0.5)
  assert bool(torch.isfinite(p).all()) and float((p.sum(dim=-1) - 1).abs().max()) <= 1e-6


# ---- guards ------------------------------------------------------------------------------------------------------------------
def test_decode_index_out_of_range_sets_the_status_word():
  c = torch.arange(12, dtype=torch.float32).view(4, 3) + 1
  index = torch.tensor([2, 4, 1, -1, 3], dtype=torch.int32)
  y, status = ops.vq_decode(_dev(index), _dev(c))
  assert int(status.item()) & 1
  want = c[torch.tensor([2, 0, 1, 0, 3])]
  assert torch.equal(y.cpu(), want)
  dy = torch.ones(5, 3)
  dc, status = ops.vq_decode_bwd(_dev(index), _dev(dy), 4)
  assert int(status.item()) & 1
  assert torch.equal(dc.cpu(), torch.tensor([2., 1., 1., 1.]).view(4, 1).expand(4, 3))
  good, status = ops.vq_decode(_dev(torch.tensor([0, 3], dtype=torch.int32)), _dev(c))
  assert int(status.item()) == 0 and torch.equal(good.cpu(), c[[0, 3]])


def test_limits_are_refused_before_any_launch():
  L = jpdse_hip.lib()
  EINVAL = -1
  M, D, Lc = 16, 8, 64
  x = torch.zeros(M, D, device=DEV)
  c = torch.zeros(Lc, D, device=DEV)
  p = torch.full((M, Lc), 7.0, device=DEV)
  dp = torch.zeros(M, Lc, device=DEV)
  out = torch.full((Lc, D), 7.0, device=DEV)
  index = torch.zeros(M, dtype=torch.int32, device=DEV)
  status = torch.zeros(1, dtype=torch.int32, device=DEV)
  ws = torch.zeros(L.jpdse_vq_workspace_size(M, D, Lc), dtype=torch.uint8, device=DEV)
  st = torch.cuda.current_stream().cuda_stream

  def soft(dtype=F32, M=M, D=D, Lc=Lc, sigma=1.0, x=x, c=c, p=p):
    a = jpdse_hip.VqSoftFwdArgs(dtype, M, D, Lc, sigma, x.data_ptr() if x is not None else None,
                                c.data_ptr() if c is not None else None, p.data_ptr() if p is not None else None, st)
    return L.jpdse_vq_soft_fwd(ctypes.byref(a))

  bad = [dict(D=0), dict(D=33), dict(Lc=1), dict(Lc=513), dict(M=0), dict(M=2 ** 22, Lc=512), dict(sigma=0.0), dict(sigma=-1.0),
         dict(sigma=float('inf')), dict(sigma=float('nan')), dict(dtype=2), dict(x=None), dict(c=None), dict(p=None)]
  for kw in bad:
    assert soft(**kw) == EINVAL, kw
    assert jpdse_hip.last_error().startswith('vq_soft_fwd'), kw
  assert L.jpdse_vq_soft_fwd(None) == EINVAL

  def bwd(ws_ptr=ws.data_ptr(), ws_bytes=ws.numel(), dc=out, sigma=1.0, D=D):
    a = jpdse_hip.VqSoftBwdArgs(F32, M, D, Lc, sigma, dp.data_ptr(), p.data_ptr(), x.data_ptr(), c.data_ptr(), None,
                                dc.data_ptr() if dc is not None else None, ws_ptr, ws_bytes, st)
    return L.jpdse_vq_soft_bwd(ctypes.byref(a))

  assert bwd(ws_ptr=None) == EINVAL and bwd(ws_bytes=ws.numel() - 1) == EINVAL and bwd(sigma=0.0) == EINVAL and bwd(D=33) == EINVAL
  a = jpdse_hip.VqDecodeArgs(F32, M, D, Lc, index.data_ptr(), c.data_ptr(), out.data_ptr(), None, st)
  assert L.jpdse_vq_decode(ctypes.byref(a)) == EINVAL                         # no status word
  a = jpdse_hip.VqDecodeBwdArgs(F32, M, D, Lc, index.data_ptr(), x.data_ptr(), out.data_ptr(), status.data_ptr(), None, 0, st)
  assert L.jpdse_vq_decode_bwd(ctypes.byref(a)) == EINVAL                     # no workspace
  a = jpdse_hip.VqHardFwdArgs(F32, M, D, 513, x.data_ptr(), c.data_ptr(), index.data_ptr(), None, st)
  assert L.jpdse_vq_hard_fwd(ctypes.byref(a)) == EINVAL
  a = jpdse_hip.VqArgmaxArgs(M, 1, p.data_ptr(), index.data_ptr(), st)
  assert L.jpdse_vq_argmax(ctypes.byref(a)) == EINVAL
  a = jpdse_hip.VqPmfArgs(M, Lc, p.data_ptr(), out.data_ptr(), None, 0, st)
  assert L.jpdse_vq_pmf(ctypes.byref(a)) == EINVAL
  a = jpdse_hip.VqPmfBwdArgs(0, Lc, out.data_ptr(), p.data_ptr(), st)
  assert L.jpdse_vq_pmf_bwd(ctypes.byref(a)) == EINVAL
  torch.cuda.synchronize()
  # nothing ran: the would-be outputs still hold their fill
  assert bool((p == 7.0).all()) and bool((out == 7.0).all()) and int(status.item()) == 0
  assert soft() == 0 and bwd() == 0
