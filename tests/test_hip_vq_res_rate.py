"""GPU tests of the rate term of the residual vector quantizer (vq_res_rate.hip, vq_residual.hip; ops.vq_res_rate_fwd /
ops.vq_res_bwd(groups, dhist); ctu.quantizers.ResidualS2HVQ.rate) against the float64 restatement
tests/vq_res_rate_ref.py, the kernels it must agree with (ops.vq_res_rows_fwd bit for bit, ops.vq_rate_fwd for one stage,
ops.vq_res_bwd bit for bit without a dhist) and the exact contracts.

Cases (M, L, D, S, G): the table of the issue, then one case on either side of every threshold of the path selection
(vqrr_waves, vq_res_rate.hip: the per-wave tables take S G (L + 1) words -- 3072 / 3073.. words: 4 or 2 waves; 6144: 2 or 1; 12288: one
wave inside 48 KiB or opted in above; 36864: opted in or the general path) and of the grouped backward's staging of dhist (LDS while
the block stays within 64000 bytes).  x is standard normal, the books uniform in [-1, 1), sigma = 1 / D, as
tests/test_hip_vq_residual.py draws them.  The seeds were checked on the CPU: the float64 reference alone leaves at most 1 % of the
rows of every case undecided (the GAP rule); a case beyond that fails.  Sums over all rows are measured against the reference that
follows the device's index on the undecided rows; dx is compared on the decided rows."""
import ctypes

import pytest
import torch

import jpdse_hip
from jpdse_hip import ops, F32, BF16
import hip_util as hu
import vq_residual_ref
import vq_res_rate_ref as ref

pytestmark = pytest.mark.gpu
DEV = hu.DEV
CASES = [(1, 2, 1, 1, 1), (66, 64, 8, 2, 2), (255, 5, 3, 3, 3), (304, 512, 32, 2, 16), (4112, 64, 8, 4, 16), (4100, 64, 8, 2, 20),
         (1040, 16, 4, 8, 130),
         (320, 63, 4, 3, 16), (320, 64, 4, 3, 16),      # 3072 | 3120 words: 4 waves | 2 waves
         (320, 63, 4, 3, 32), (320, 64, 4, 3, 32),      # 6144 | 6240: 2 waves | 1 wave
         (320, 63, 4, 3, 64), (320, 64, 4, 3, 64),      # 12288 | 12480: 1 wave inside 48 KiB | opted in above 64 KiB
         (320, 71, 4, 8, 64), (320, 72, 4, 8, 64),      # 36864 | 37376: opted in | the general path
         (320, 64, 8, 2, 32), (320, 64, 8, 2, 64)]      # the backward with dbooks: dhist staged in LDS (60672 bytes) | read from global
SCALE, DENOM = 0.5, 2.0      # dhist of the order of dy's share of dp: neither term hides the other in the gradients
_cache = {}


def _dev(t, dtype=None):
  t = t.to(DEV)
  return t.to(torch.bfloat16) if dtype == BF16 else t


def _sigma(D):
  return 1.0 / D


def _inputs(case, dtype):
  """Seeded inputs, computed once per (case, dtype) and never modified; the float64 chain alone decides the 1 % cap."""
  key = (case, dtype)
  if key not in _cache:
    M, L, D, S, G = case
    g = torch.Generator().manual_seed(2600 + M + L + 7 * S + G)
    x = hu.quantize_like(torch.randn(M, D, generator=g), dtype)
    books = torch.rand(S, L, D, generator=g) * 2 - 1
    dy = hu.quantize_like(torch.randn(M, D, generator=g), dtype)
    _, decided = ref.chain(x.double(), books.double())
    assert int((~decided).sum()) <= 0.01 * M, '%d of %d rows undecided in float64: beyond the 1 %% cap' % (int((~decided).sum()), M)
    _cache[key] = (x, books, dy, decided)
  return _cache[key]


def _run(case, dtype):
  """The device's forward with everything asked for, and the float64 reference that follows its index: once per (case, dtype)."""
  key = (case, dtype, 'run')
  if key not in _cache:
    M, L, D, S, G = case
    x, books, dy, decided = _inputs(case, dtype)
    xd, bd = _dev(x, dtype), _dev(books)
    got = ops.vq_res_rate_fwd(xd, bd, _sigma(D), G, DENOM, SCALE, want_code=True, want_hist=True)
    follow = got[5].cpu().long()
    assert torch.equal(follow[:, decided], ref.chain(x.double(), books.double())[0][:, decided]), 'an index differs on a decided row'
    rate, rates, hist, _ = ref.rate(x.double(), books.double(), _sigma(D), G, DENOM, follow=follow)
    want = dict(rate=rate, rates=rates, hist=hist, dhist=ref.dhist_of(hist, M // G, DENOM, SCALE), follow=follow)
    _cache[key] = (xd, bd, got, want)
  return _cache[key]


def _close(got, want, dtype, what):
  hu.assert_close(got.double().cpu(), want, hu.RTOL[dtype], what)


@pytest.mark.parametrize('dtype', hu.DTYPES)
@pytest.mark.parametrize('case', CASES, ids=str)
def test_forward_matches_fp64_and_the_exact_contracts(case, dtype):
  M, L, D, S, G = case
  xd, bd, (rate, rates, hist, dhist, y, index), want = _run(case, dtype)
  assert tuple(rate.shape) == (1,) and tuple(rates.shape) == (S,) and tuple(hist.shape) == tuple(dhist.shape) == (S, G, L)
  assert all(t.dtype == torch.float32 for t in (rate, rates, hist, dhist)) and y.dtype == xd.dtype and index.dtype == torch.int32
  # every quantity is a sum over all rows in fp32 partials merged in fp64: the bound of test_hip_vq_rate.py, at F32 whatever x is
  _close(hist / (M // G), want['hist'] / (M // G), F32, 'vq_res_rate_fwd hist / n')
  _close(rates, want['rates'], F32, 'vq_res_rate_fwd rates')
  _close(rate, want['rate'].reshape(1), F32, 'vq_res_rate_fwd rate')
  _close(dhist, want['dhist'], F32, 'vq_res_rate_fwd dhist')
  # exact: the code is the rows kernel's for every stage prefix; dhist is 0 where hist is; rate is the stage-order sum
  for n in range(1, S + 1):
    yn, indexn = ops.vq_res_rows_fwd(xd, bd, n)
    got = ops.vq_res_rate_fwd(xd, bd, _sigma(D), G, DENOM, SCALE, n_stages=n, want_code=True, want_hist=True)
    assert torch.equal(got[4], yn) and torch.equal(got[5], indexn), 'stage prefix %d' % n
    # the sums of a prefix may take another tile or path (both depend on the stage count): close, not bit-equal
    _close(got[2], hist[:n].double().cpu(), F32, 'vq_res_rate_fwd hist of a stage prefix')
  assert not bool(dhist[hist == 0].any()) and bool((hist >= 0).all())
  total = rates[0].clone()
  for s in range(1, S):
    total = total + rates[s]
  assert torch.equal(rate.reshape(()), total)
  # nothing but the outputs asked for changes nothing; a second call gives the same bits
  r2, rs2, none_h, none_d, none_y, none_i = ops.vq_res_rate_fwd(xd, bd, _sigma(D), G, DENOM, SCALE, want_grad=False)
  assert none_h is None and none_d is None and none_y is None and none_i is None
  assert torch.equal(r2, rate) and torch.equal(rs2, rates)
  again = ops.vq_res_rate_fwd(xd, bd, _sigma(D), G, DENOM, SCALE, want_code=True, want_hist=True)
  assert all(torch.equal(a, b) for a, b in zip(again, (rate, rates, hist, dhist, y, index)))


@pytest.mark.parametrize('dtype', hu.DTYPES)
@pytest.mark.parametrize('case', CASES, ids=str)
def test_grouped_backward_matches_fp64_autograd_and_the_plain_call(case, dtype):
  M, L, D, S, G = case
  x, books, dy, decided = _inputs(case, dtype)
  xd, bd, (_, _, _, dhist, _, index), want = _run(case, dtype)
  dyd = _dev(dy, dtype)
  dx, dc = ops.vq_res_bwd(dyd, xd, bd, index, _sigma(D), groups=G, dhist=dhist)
  assert dx.dtype == xd.dtype and dc.dtype == torch.float32 and tuple(dc.shape) == (S, L, D)
  dx64, dc64 = ref.grads(dy.double(), x.double(), books.double(), _sigma(D), G, DENOM, SCALE, follow=want['follow'])
  _close(dx[_dev(decided)], dx64[decided], dtype, 'vq_res_bwd grouped dx')
  _close(dc, dc64, F32, 'vq_res_bwd grouped dbooks')
  only_dx, none = ops.vq_res_bwd(dyd, xd, bd, index, _sigma(D), want_dc=False, groups=G, dhist=dhist)
  assert none is None and torch.equal(only_dx, dx)
  dx2, dc2 = ops.vq_res_bwd(dyd, xd, bd, index, _sigma(D), groups=G, dhist=dhist)
  assert torch.equal(dx2, dx) and torch.equal(dc2, dc)
  # without a dhist, or with zeros, the grouped call gives the plain call's bits
  dx0, dc0 = ops.vq_res_bwd(dyd, xd, bd, index, _sigma(D))
  for dh in (None, torch.zeros_like(dhist)):
    dxg, dcg = ops.vq_res_bwd(dyd, xd, bd, index, _sigma(D), groups=G, dhist=dh)
    assert torch.equal(dxg, dx0) and torch.equal(dcg, dc0)
  assert not torch.equal(dc, dc0)


@pytest.mark.parametrize('dtype', hu.DTYPES)
@pytest.mark.parametrize('case', [(66, 64, 8, 1, 2), (4112, 64, 8, 1, 16), (255, 5, 3, 1, 3), (304, 512, 32, 1, 16)], ids=str)
def test_one_stage_is_the_bottleneck_rate_term(case, dtype):
  M, L, D, S, G = case
  x, books, dy, _ = _inputs(case, dtype)
  xd, bd, dyd = _dev(x, dtype), _dev(books), _dev(dy, dtype)
  rate, rates, hist, dhist, _, index = ops.vq_res_rate_fwd(xd, bd, _sigma(D), G, DENOM, SCALE, want_code=True, want_hist=True)
  rate1, hist1, dhist1 = ops.vq_rate_fwd(xd, bd[0], _sigma(D), G, DENOM, SCALE, want_hist=True)
  _close(rate, rate1.double().cpu(), F32, 'vq_res_rate_fwd rate vs vq_rate_fwd')
  _close(hist[0], hist1.double().cpu(), F32, 'vq_res_rate_fwd hist vs vq_rate_fwd')
  _close(dhist[0], dhist1.double().cpu(), F32, 'vq_res_rate_fwd dhist vs vq_rate_fwd')
  assert torch.equal(rate, rates)
  dx, dc = ops.vq_res_bwd(dyd, xd, bd, index, _sigma(D), groups=G, dhist=dhist)
  dx1, dc1 = ops.vq_quantize_bwd(dyd, xd, bd[0], _sigma(D), groups=G, dhist=dhist[0].contiguous())
  _close(dx, dx1.double().cpu(), dtype, 'vq_res_bwd grouped dx vs vq_quantize_bwd grouped')
  _close(dc[0], dc1.double().cpu(), F32, 'vq_res_bwd grouped dbooks vs vq_quantize_bwd grouped')


# 66 tiles of 256 vectors on 64 blocks (the cap of the partials: 2^22 / (4 * 64 * 256)): the first two blocks walk a second tile,
# the last tile holds 64 vectors.  G = 64 with L = 256 is the general path; M is the multiple of G next to 16384 + 300
TWO_TILES = (16704, 256, 8, 4, 64)


@pytest.mark.parametrize('dtype', hu.DTYPES)
def test_a_block_that_walks_two_tiles(dtype):
  M, L, D, S, G = TWO_TILES
  xd, bd, (_, _, hist, _, y, index), want = _run(TWO_TILES, dtype)
  y0, index0 = ops.vq_res_rows_fwd(xd, bd)
  assert torch.equal(index, index0) and torch.equal(y, y0)
  _close(hist / (M // G), want['hist'] / (M // G), F32, 'vq_res_rate_fwd hist / n, two tiles per block')


def test_refusals_leave_the_outputs_untouched():
  M, L, D, S, G = 64, 16, 4, 2, 4
  g = torch.Generator().manual_seed(1)
  x, books = _dev(torch.randn(M, D, generator=g)), _dev(torch.rand(S, L, D, generator=g) * 2 - 1)
  mark = 12345.0
  outs = dict(rate=torch.full((1,), mark, device=DEV), rates=torch.full((S,), mark, device=DEV),
              hist=torch.full((S, G, L), mark, device=DEV), dhist=torch.full((S, G, L), mark, device=DEV),
              y=torch.full((M, D), mark, device=DEV), index=torch.full((S, M), 777, dtype=torch.int32, device=DEV))
  ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
  base = dict(dtype=F32, M=M, D=D, L=L, S=S, n_stages=S, G=G, sigma=0.25, scale=1.0, denom=1.0, x=x.data_ptr(), books=books.data_ptr(),
              ws=ws.data_ptr(), ws_bytes=ws.numel(), stream=torch.cuda.current_stream().cuda_stream)
  base.update({k: v.data_ptr() for k, v in outs.items()})
  lib = jpdse_hip.lib()
  for over, field in ((dict(n_stages=0), 'n_stages'), (dict(n_stages=3), 'n_stages'), (dict(G=0), 'G = 0'), (dict(G=3), 'G = 3'),
                      (dict(sigma=0.0), 'sigma'), (dict(scale=float('nan')), 'scale'), (dict(denom=0.0), 'denom'),
                      (dict(denom=float('inf')), 'denom'), (dict(rate=None), 'rate'), (dict(rates=None), 'rates'),
                      (dict(y=None), 'y and index'), (dict(ws_bytes=8), 'workspace'), (dict(L=1), 'n_center L'), (dict(D=33), 'D = 33')):
    a = dict(base)
    a.update(over)
    assert lib.jpdse_vq_res_rate_fwd(ctypes.byref(jpdse_hip.VqResRateFwdArgs(**a))) == -1, over
    assert field in jpdse_hip.last_error(), (over, jpdse_hip.last_error())
  dx = torch.full((M, D), mark, device=DEV)
  dc = torch.full((S, L, D), mark, device=DEV)
  bwd = dict(dtype=F32, M=M, D=D, L=L, S=S, n_stages=S, sigma=0.25, dy=x.data_ptr(), x=x.data_ptr(), books=books.data_ptr(),
             index=outs['index'].data_ptr(), dx=dx.data_ptr(), dbooks=dc.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel(),
             stream=base['stream'])
  for over, Gb, field in ((dict(), 0, 'G = 0'), (dict(), 3, 'G = 3'), (dict(n_stages=0), G, 'n_stages'), (dict(sigma=float('nan')), G, 'sigma'),
                          (dict(ws_bytes=8), G, 'workspace')):
    a = dict(bwd)
    a.update(over)
    ga = jpdse_hip.VqResBwdGroupedArgs(jpdse_hip.VqResBwdArgs(**a), Gb, outs['dhist'].data_ptr())
    assert lib.jpdse_vq_res_bwd_grouped(ctypes.byref(ga)) == -1, (over, Gb)
    assert field in jpdse_hip.last_error(), (over, jpdse_hip.last_error())
  torch.cuda.synchronize()
  for k, v in outs.items():
    assert bool((v == (777 if k == 'index' else mark)).all()), k
  assert bool((dx == mark).all()) and bool((dc == mark).all())


@pytest.mark.parametrize('dtype', hu.DTYPES)
@pytest.mark.parametrize('case,stages', [((4112, 64, 8, 4, 16), 2), ((304, 512, 32, 2, 16), 1), ((255, 5, 3, 3, 3), 3)], ids=str)
def test_module_rate_backward_with_a_stage_prefix(case, stages, dtype):
  from ctu.quantizers import ResidualS2HVQ, S2HVQ
  M, L, D, S, G = case
  code_len = G
  x, books, _, decided = _inputs(case, dtype)
  rvq = ResidualS2HVQ(_dev(books).clone(), sigma=_sigma(D)).train()
  xin = _dev(x, dtype).view(M // code_len, code_len * D).clone().requires_grad_(True)
  value = rvq.rate(xin, code_len, groups=G, denom=DENOM, stages=stages)
  assert value.dim() == 0 and value.dtype == torch.float32
  (value * 0.5).backward()
  index = ops.vq_res_rows_fwd(_dev(x, dtype), _dev(books), stages)[1].cpu().long()
  want = ref.rate(x.double(), books.double(), _sigma(D), G, DENOM, stages, follow=index)[0]
  _close(value.reshape(1), want.reshape(1), F32, 'ResidualS2HVQ.rate')
  dx64, dc64 = ref.grads(torch.zeros(M, D, dtype=torch.float64), x.double(), books.double(), _sigma(D), G, DENOM, 0.5, stages,
                         follow=index)
  _close(xin.grad.view(M, D)[_dev(decided)], dx64[decided], dtype, 'ResidualS2HVQ.rate dx')
  gb = rvq.code_books.grad
  _close(gb, dc64, F32, 'ResidualS2HVQ.rate dbooks')
  assert not bool(gb[stages:].any()), 'a book beyond `stages` got a gradient'
  # without gradients: the same value, nothing saved
  with torch.no_grad():
    v2 = rvq.rate(xin, code_len, groups=G, denom=DENOM, stages=stages)
  assert v2.grad_fn is None and torch.equal(v2, value.detach())
  if stages == 1:      # one stage: S2HVQ.rate's value, within the bound
    one = S2HVQ(_dev(books[0]).clone(), sigma=_sigma(D))
    with torch.no_grad():
      _close(value.reshape(1), one.rate(xin, code_len, groups=G, denom=DENOM).double().cpu().reshape(1), F32,
             'ResidualS2HVQ.rate vs S2HVQ.rate')
