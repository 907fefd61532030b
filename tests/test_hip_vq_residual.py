"""GPU tests of the residual vector quantizer (vq_residual.hip; ops.vq_res_fwd / vq_res_decode / vq_res_bwd;
ctu.quantizers.ResidualS2HVQ; ctu.utils.vqstages) against the float64 reference tests/vq_residual_ref.py, the
one-stage kernels it must agree with, the composed form, and the exact contracts (integers, ties, decode, repeatability).

Cases (M, L, D, S): M 1, 63, 65, 1000 -- one vector, one short of and one past a wave, several 256-vector tiles of the forward and
64-vector tiles of the widest backward with a ragged last one; (L, D) (2, 1) the smallest book, (64, 8) a book staged in LDS by
the backward, (512, 32) both limits: the 64 KiB book restaged per stage in more than 64 KiB of LDS, the widest register
footprint; S 1, 2, 4, 8.  x is standard normal, the books uniform in [-1, 1) as the encoder's layer draws them.  sigma = 1 / D:
with scores of the order of D the exponent's float32 rounding stays far below the tolerance (the fixture of 4.13 scales its
inputs for the same reason).  The seeds were checked on the CPU: the float64 reference alone leaves at most 1 % of the rows of
every case undecided (the GAP rule); a case beyond that fails."""
import pytest
import torch

from jpdse_hip import ops, F32, BF16
import hip_util as hu
import vq_util
import vq_residual_ref as ref

pytestmark = pytest.mark.gpu
DEV = hu.DEV
CASES = [(1, 2, 1, 1), (63, 2, 1, 8), (65, 64, 8, 2), (1000, 64, 8, 1), (1000, 64, 8, 4), (63, 512, 32, 2), (65, 512, 32, 4),
         (65, 512, 32, 8), (1000, 512, 32, 2)]
_cache = {}


def _dev(t, dtype=None):
  t = t.to(DEV)
  return t.to(torch.bfloat16) if dtype == BF16 else t


def _sigma(D):
  return 1.0 / D


def _inputs(case, dtype):
  """Seeded inputs and their float64 forward, computed once per (case, dtype) and never modified."""
  key = (case, dtype)
  if key not in _cache:
    M, L, D, S = case
    g = torch.Generator().manual_seed(2300 + M + L + 7 * S)
    x = hu.quantize_like(torch.randn(M, D, generator=g), dtype)
    books = torch.rand(S, L, D, generator=g) * 2 - 1
    dy = hu.quantize_like(torch.randn(M, D, generator=g), dtype)
    y, index, sse, res, decided = ref.forward(x.double(), books.double())
    assert int((~decided).sum()) <= 0.01 * M, '%d of %d rows undecided in float64: beyond the 1 %% cap' % (int((~decided).sum()), M)
    _cache[key] = (x, books, dy, dict(y=y, index=index, sse=sse, residual=res, decided=decided))
  return _cache[key]


def _close(got, want, dtype, what):
  hu.assert_close(got.double().cpu(), want, hu.RTOL[dtype], what)


@pytest.mark.parametrize('dtype', hu.DTYPES)
@pytest.mark.parametrize('case', CASES, ids=str)
def test_forward_matches_fp64_decodes_and_repeats(case, dtype):
  M, L, D, S = case
  x, books, _, want = _inputs(case, dtype)
  xd, bd = _dev(x, dtype), _dev(books)
  y, index, sse, res = ops.vq_res_fwd(xd, bd, want_sse=True, want_residual=True)
  assert y.dtype == xd.dtype and tuple(index.shape) == (S, M) and index.dtype == torch.int32
  assert sse.dtype == torch.float64 and tuple(sse.shape) == (S,) and res.dtype == torch.float32
  got = index.cpu().long()
  assert bool(((got >= 0) & (got < L)).all())
  keep = want['decided']
  assert torch.equal(got[:, keep], want['index'][:, keep]), 'an index differs from float64 on a decided row'
  _close(y[_dev(keep)], want['y'][keep], dtype, 'vq_res_fwd y')
  _close(res[_dev(keep)], want['residual'][keep], F32, 'vq_res_fwd residual')
  # the sums run over ALL rows: the reference follows the device's choice on the undecided ones
  sse_ref = ref.forward(x.double(), books.double(), follow=got)[2]
  _close(sse, sse_ref, F32, 'vq_res_fwd sse')
  # nothing but the outputs asked for changes nothing; a second call gives the same bits
  y2, index2, none, none2 = ops.vq_res_fwd(xd, bd)
  assert none is None and none2 is None and torch.equal(y2, y) and torch.equal(index2, index)
  y3, index3, sse3, res3 = ops.vq_res_fwd(xd, bd, want_sse=True, want_residual=True)
  assert torch.equal(y3, y) and torch.equal(index3, index) and torch.equal(sse3, sse) and torch.equal(res3, res)
  # every stage prefix: the forward, and the decoder bit for bit
  for n in range(1, S + 1):
    yn, indexn, ssen, _ = ops.vq_res_fwd(xd, bd, n_stages=n, want_sse=True)
    assert torch.equal(indexn, index[:n]) and torch.equal(ssen, sse[:n])
    dec, status = ops.vq_res_decode(index, bd, n_stages=n, dtype=xd.dtype)
    assert torch.equal(dec, yn) and int(status.item()) == 0
    dec2, _ = ops.vq_res_decode(index[:n].contiguous(), bd, dtype=xd.dtype)
    assert torch.equal(dec2, yn)
  y0, index0, _, res0 = ops.vq_res_fwd(xd, bd, n_stages=0, want_residual=True)
  assert index0.shape[0] == 0 and not bool(y0.any()) and torch.equal(res0, xd.float())


@pytest.mark.parametrize('dtype', hu.DTYPES)
@pytest.mark.parametrize('case', [c for c in CASES if c[3] == 1] + [(65, 512, 32, 1)], ids=str)
def test_one_stage_is_the_bottleneck_kernel(case, dtype):
  """index and y: bit for bit ops.vq_quantize_fwd(hard).  The backward: within RTOL / ETOL of ops.vq_quantize_bwd -- the two kernels
  run the same sweeps on the shared core (vq_rows.h) but are separate code, so bit equality is not promised and not asserted."""
  M, L, D, S = case
  x, books, dy, _ = _inputs(case, dtype)
  xd, bd, dyd = _dev(x, dtype), _dev(books), _dev(dy, dtype)
  sigma = _sigma(D)
  y, index, _, _ = ops.vq_res_fwd(xd, bd)
  y1, index1, _ = ops.vq_quantize_fwd(xd, bd[0], sigma, hard_forward=True)
  assert torch.equal(index[0], index1) and torch.equal(y, y1)
  dx, dc = ops.vq_res_bwd(dyd, xd, bd, index, sigma)
  dx1, dc1 = ops.vq_quantize_bwd(dyd, xd, bd[0], sigma)
  _close(dx, dx1.double().cpu(), dtype, 'vq_res_bwd dx vs vq_quantize_bwd')
  _close(dc[0], dc1.double().cpu(), F32, 'vq_res_bwd dbooks vs vq_quantize_bwd')


@pytest.mark.parametrize('case', [c for c in CASES if c[3] in (2, 4)], ids=str)
def test_composed_form_is_bit_identical_fp32(case):
  """S rounds of ops.vq_hard_fwd / ops.vq_decode on a torch-subtracted fp32 residual: the same score, tie rule and subtraction."""
  M, L, D, S = case
  x, books, _, _ = _inputs(case, F32)
  xd, bd = _dev(x), _dev(books)
  y, index, _, res = ops.vq_res_fwd(xd, bd, want_residual=True)
  r, ysum = xd, None
  for s in range(S):
    k, _ = ops.vq_hard_fwd(r, bd[s])
    c, _ = ops.vq_decode(k, bd[s])
    assert torch.equal(k, index[s]), 'stage %d' % s
    ysum = c if ysum is None else ysum + c
    r = r - c
  assert torch.equal(ysum, y) and torch.equal(r, res)


@pytest.mark.parametrize('dtype', hu.DTYPES)
@pytest.mark.parametrize('case', [(63, 2, 1, 8), (65, 64, 8, 4), (1000, 512, 32, 2)], ids=str)
def test_integer_inputs_are_exact(case, dtype):
  """Small integers: every score, subtraction and sum is exact (|residual| <= 8 + 4 S, |y| <= 4 S), ties included -- both sides
  take the lowest index."""
  M, L, D, S = case
  g = torch.Generator().manual_seed(77 + M + L + S)
  x = torch.randint(-8, 9, (M, D), generator=g).float()
  books = torch.randint(-4, 5, (S, L, D), generator=g).float()
  y64, index64, sse64, res64, _ = ref.forward(x.double(), books.double())
  y, index, sse, res = ops.vq_res_fwd(_dev(x, dtype), _dev(books), want_sse=True, want_residual=True)
  assert torch.equal(index.cpu().long(), index64)
  assert torch.equal(y.float().cpu().double(), y64) and torch.equal(res.cpu().double(), res64) and torch.equal(sse.cpu(), sse64)


def test_ties_go_to_the_lowest_index_at_every_stage():
  books = torch.full((2, 130, 1), 3.0)
  books[0, [5, 70, 129], 0] = torch.tensor([1.0, -1.0, 1.0])      # stage 1: three nearest to 0 at distance 1 -> 5, r_2 = -1
  books[1, [6, 7, 100], 0] = torch.tensor([-2.0, 0.0, -2.0])      # stage 2: three nearest to -1 at distance 1 -> 6, y = 1 - 2
  x = torch.zeros(3, 1)
  y, index, _, res = ops.vq_res_fwd(_dev(x), _dev(books), want_residual=True)
  assert index.cpu().tolist() == [[5, 5, 5], [6, 6, 6]]
  assert torch.equal(y.cpu(), -torch.ones(3, 1)) and torch.equal(res.cpu(), torch.ones(3, 1))
  books[1, 6, 0] = 3.0                                            # now 7 and 100 tie across two lanes' slots
  assert ops.vq_res_fwd(_dev(x), _dev(books))[1].cpu().tolist() == [[5, 5, 5], [7, 7, 7]]


def test_decode_out_of_range_index_reads_centre_zero_and_sets_status():
  g = torch.Generator().manual_seed(5)
  books = torch.rand(3, 5, 4, generator=g)
  index = torch.tensor([[0, 1, 2, 3], [4, 5, 0, 1], [2, -1, 4, 0]], dtype=torch.int32)
  y, status = ops.vq_res_decode(_dev(index), _dev(books))
  assert int(status.item()) == 1
  fixed = index.clone().long()
  fixed[1, 1] = 0
  fixed[2, 1] = 0
  want = (books[0][fixed[0]] + books[1][fixed[1]]) + books[2][fixed[2]]
  assert torch.equal(y.cpu(), want)
  y2, status2 = ops.vq_res_decode(_dev(index), _dev(books), n_stages=1)       # the first stage alone is clean
  assert int(status2.item()) == 0 and torch.equal(y2.cpu(), books[0][fixed[0]])


def _grad_case(case, dtype, n_stages=None):
  """Device inputs and the float64 oracle of the gradients over the decided rows, dy zeroed on the others for both sides."""
  M, L, D, S = case
  x, books, dy, want = _inputs(case, dtype)
  keep = want['decided']
  dyk = dy * keep.unsqueeze(1).to(dy.dtype)
  dx64, dc64 = ref.grads(dyk.double()[keep], x.double()[keep], books.double(), _sigma(D), n_stages)
  return x, books, dyk, keep, dx64, dc64


@pytest.mark.parametrize('dtype', hu.DTYPES)
@pytest.mark.parametrize('case', CASES, ids=str)
def test_backward_matches_fp64_autograd_and_repeats(case, dtype):
  M, L, D, S = case
  x, books, dyk, keep, dx64, dc64 = _grad_case(case, dtype)
  xd, bd, dyd = _dev(x, dtype), _dev(books), _dev(dyk, dtype)
  index = ops.vq_res_fwd(xd, bd)[1]
  dx, dc = ops.vq_res_bwd(dyd, xd, bd, index, _sigma(D))
  assert dx.dtype == xd.dtype and dc.dtype == torch.float32 and tuple(dc.shape) == (S, L, D)
  _close(dx[_dev(keep)], dx64, dtype, 'vq_res_bwd dx')
  _close(dc, dc64, F32, 'vq_res_bwd dbooks')
  only_dx, none = ops.vq_res_bwd(dyd, xd, bd, index, _sigma(D), want_dc=False)
  none2, only_dc = ops.vq_res_bwd(dyd, xd, bd, index, _sigma(D), want_dx=False)
  assert none is None and none2 is None and torch.equal(only_dx, dx) and torch.equal(only_dc, dc)
  dx2, dc2 = ops.vq_res_bwd(dyd, xd, bd, index, _sigma(D))
  assert torch.equal(dx2, dx) and torch.equal(dc2, dc)


@pytest.mark.parametrize('dtype', hu.DTYPES)
@pytest.mark.parametrize('case,stages', [((1000, 64, 8, 4), 2), ((65, 512, 32, 4), 3)], ids=str)
def test_module_autograd_with_a_stage_prefix(case, stages, dtype):
  from ctu.quantizers import ResidualS2HVQ
  M, L, D, S = case
  code_len = 5 if M % 5 == 0 else 1
  x, books, dyk, keep, dx64, dc64 = _grad_case(case, dtype, stages)
  rvq = ResidualS2HVQ(_dev(books).clone(), sigma=_sigma(D)).train()
  xin = _dev(x, dtype).view(M // code_len, code_len * D).clone().requires_grad_(True)
  y, code = rvq.quantize(xin, code_len, stages=stages)
  assert tuple(code.shape) == (stages, M // code_len, code_len) and code.dtype == torch.int64 and y.dtype == xin.dtype
  y.backward(_dev(dyk, dtype).view_as(y))
  _close(xin.grad.view(M, D)[_dev(keep)], dx64, dtype, 'ResidualS2HVQ.quantize dx')
  g = rvq.code_books.grad
  _close(g, dc64, F32, 'ResidualS2HVQ.quantize dbooks')
  assert not bool(g[stages:].any()), 'a book beyond `stages` got a gradient'
  # eval mode: the same values, nothing saved; encode / decode agree with it bit for bit
  rvq.eval()
  ye, ce = rvq.quantize(xin.detach(), code_len, stages=stages)
  assert ye.grad_fn is None and torch.equal(ye, y.detach()) and torch.equal(ce, code)
  assert torch.equal(rvq.encode(xin.detach(), code_len, stages=stages), code)
  assert torch.equal(rvq.decode(code), ye.float()) if dtype == F32 else True
  full = rvq.encode(xin.detach(), code_len)
  assert torch.equal(rvq.decode(full, stages=stages), rvq.decode(code))


def test_one_stage_module_gives_s2hvq_results():
  from ctu.quantizers import ResidualS2HVQ, S2HVQ
  g = torch.Generator().manual_seed(11)
  x = _dev(torch.randn(40, 24, generator=g))
  book = torch.rand(64, 8, generator=g) * 2 - 1
  one, rvq = S2HVQ(_dev(book).clone(), sigma=0.5).eval(), ResidualS2HVQ(_dev(book).clone().unsqueeze(0), sigma=0.5).eval()
  y1, c1, _ = one.quantize(x, 3)
  y, c = rvq.quantize(x, 3)
  assert torch.equal(y, y1) and torch.equal(c[0], c1) and torch.equal(rvq.encode(x, 3)[0], one.encode(x, 3, train=False, raw=False))
  ys, cs = rvq.quantize(x, 3, hard_forward=False)
  assert torch.equal(ys, one.quantize(x, 3, hard_forward=False)[0]) and torch.equal(cs[0], c1)
  f1, f = one.fit(x, 3, n_iter=3, seed=4), rvq.fit(x, 3, n_iter=3, seed=4)
  assert torch.equal(rvq.code_books.data[0], one.code_book.data) and f[0]['distortion'] == f1['distortion']
  assert f[0]['final'] == float(rvq.distortion(x, 3)[0])


def test_fit_lowers_the_error_stage_by_stage_in_place_and_repeats():
  from ctu.quantizers import ResidualS2HVQ
  g = torch.Generator().manual_seed(3)
  x = _dev(torch.randn(4096, 8, generator=g))
  made = []
  for _ in range(2):
    rvq = ResidualS2HVQ(torch.zeros(3, 16, 8, device=DEV))
    ptr = rvq.code_books.data_ptr()
    rep = rvq.fit(x, 1, n_iter=5, seed=9)
    assert rvq.code_books.data_ptr() == ptr and len(rep) == 3
    made.append((rvq.code_books.data.clone(), rep))
  final = [r['final'] for r in made[0][1]]
  assert final[0] >= final[1] >= final[2] and final[0] <= made[0][1][0]['distortion'][0]
  assert final[0] < float((x.double() ** 2).sum(1).mean()), 'a fitted stage cannot raise the error: every centre is a mean'
  assert torch.equal(made[0][0], made[1][0]) and final == [r['final'] for r in made[1][1]]
  assert all(a['distortion'] == b['distortion'] for a, b in zip(made[0][1], made[1][1]))


@pytest.mark.parametrize('S', [1, 3])
def test_files_round_trip_and_truncate(S, tmp_path):
  from ctu.quantizers import ResidualS2HVQ
  from ctu.utils import vqstages
  g = torch.Generator().manual_seed(40 + S)
  rvq = ResidualS2HVQ(_dev(torch.rand(S, 64, 8, generator=g) * 2 - 1)).eval()
  x = _dev(torch.randn(50, 32, generator=g))
  code = rvq.encode(x, 4)
  path = str(tmp_path / ('code' + vqstages.SUFFIX))
  blob = vqstages.write_stages(path, code, 64, n_streams=8)
  assert open(path, 'rb').read() == blob and vqstages.coded_bits(blob) == 8 * len(blob) == vqstages.coded_bits(path)
  assert torch.equal(vqstages.read_stages(path, DEV), code) and torch.equal(vqstages.read_stages(blob), code)
  assert torch.equal(vqstages.reconstruct_stages(rvq, blob), rvq.decode(code))
  assert torch.equal(vqstages.reconstruct_stages(rvq, blob), rvq.quantize(x, 4)[0])
  for n in range(1, S + 1):
    cut = vqstages.truncate_stages(blob, n)
    assert torch.equal(vqstages.read_stages(cut), code[:n]) and torch.equal(vqstages.read_stages(blob, stages=n), code[:n])
    assert vqstages.coded_bits(blob, stages=n) == 8 * len(cut)
    assert torch.equal(vqstages.reconstruct_stages(rvq, blob, stages=n), rvq.decode(code, stages=n))
