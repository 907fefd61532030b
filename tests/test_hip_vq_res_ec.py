"""GPU tests of the entropy-constrained residual code (csrc/vq_res_ec.hip, ops.vq_res_ec_assign, ResidualS2HVQ.encode_ec / usage;
DESIGN.md 4.25).  The oracles are kernels that were there before: ops.vq_res_rows_fwd without a bias, ops.vq_ec_assign composed
stage by stage with one, ops.vq_res_decode for y, S2HVQ.encode_ec for one stage; never the kernel under test.

Shapes (M, D, L, S, G): the smallest at which each path differs -- one vector, one short of / exactly / one past a tile, several
tiles with G not dividing 256 (a tile starts in the middle of the groups), a padded D, a book in LDS and one read through L2, G
on the shuffle path (1, 4, 16, 64) and on the owner path (3), a bias slice and a table that leave LDS, and more tiles than
blocks (the table cap: 2^22 / 65536 = 64 blocks)."""
import math

import pytest
import torch

from jpdse_hip import ops
from ctu.quantizers import ResidualS2HVQ, S2HVQ
import hip_util as hu
import vq_ec_ref
import vq_res_ec_ref as ref

pytestmark = pytest.mark.gpu
DEV = hu.DEV

#        M          D   L    S  G
CASES = [(1,         4,  8,   1, 1),
         (255,       3,  5,   3, 3),
         (256,       8,  64,  3, 4),
         (257,       8,  64,  1, 1),
         (1023,      16, 200, 3, 3),       # L2 book; r0 != 0 in the tiles after the first
         (4096,      16, 200, 3, 16),
         (4099 * 3,  4,  8,   8, 3),
         (4099 * 16, 8,  64,  8, 16),
         (768,       32, 512, 3, 4),       # L2 book, the bias slice (8 KiB) and the table (24 KiB) in LDS
         (1024,      32, 512, 2, 64),      # the bias slice (128 KiB) and the table (256 KiB) leave LDS
         (769 * 64,  4,  512, 2, 64),      # 193 tiles on 64 blocks: a grid-stride of 3 to 4 tiles per block
         ]
IDS = ['M%d-D%d-L%d-S%d-G%d' % c for c in CASES]
_data_cache = {}


def _data(case):
  """(x fp32 [M, D], books fp32 [S, L, D]) on the device, built once per case and never written."""
  if case not in _data_cache:
    M, D, L, S, G = case
    g = torch.Generator().manual_seed(1000 + M + 7 * D + L)
    x = torch.randn(M, D, generator=g)
    books = torch.stack([torch.randn(L, D, generator=g) * 0.6 ** s for s in range(S)])
    _data_cache[case] = (x.to(DEV), books.to(DEV).contiguous())
  return _data_cache[case]


def _groups(M, G):
  return torch.arange(M, device=DEV) % G


def _bincount(index, G, L):
  n, M = index.shape
  g = _groups(M, G)
  return torch.stack([torch.bincount(g * L + index[s].long(), minlength=G * L).view(G, L) for s in range(n)])


def _group_sum(v, G):
  return torch.zeros(G, dtype=torch.float64, device=DEV).index_add_(0, _groups(v.shape[0], G), v.double())


def _composed(x32, books, bias, G):
  """(index [S, M], hist [S, G, L], sse [S, G]) stage by stage from ops.vq_ec_assign and the torch subtraction that DESIGN.md
  4.23 shows to be bit-exact.  Stage s depends on nothing after it: the first n rows are the oracle of the n-stage call."""
  r = x32.clone()
  index, hist, sse = [], [], []
  for s in range(books.shape[0]):
    k, h, e = ops.vq_ec_assign(r, books[s].contiguous(), None if bias is None else bias[s].contiguous(), G)
    r = r - books[s][k.long()]
    index.append(k), hist.append(h), sse.append(e)
  return torch.stack(index), torch.stack(hist), torch.stack(sse)


# ---- 1: no bias ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_no_bias_is_the_rows_forward_with_exact_counts(case):
  M, D, L, S, G = case
  x, books = _data(case)
  for n in range(1, S + 1):
    y0, i0 = ops.vq_res_rows_fwd(x, books, n)
    y, index, hist, sse = ops.vq_res_ec_assign(x, books, None, G, n)
    assert index.dtype == torch.int32 and tuple(index.shape) == (n, M) and torch.equal(index, i0)
    assert y.dtype == x.dtype and torch.equal(y, y0)
    assert hist.dtype == torch.int32 and tuple(hist.shape) == (n, G, L) and torch.equal(hist.long(), _bincount(i0, G, L))
    assert sse.dtype == torch.float64 and tuple(sse.shape) == (n, G)
    r = x.clone()
    tol = (D + 2) * math.ldexp(1.0, -23)            # the fp32 rounding of a D-term score against the exact sum of squares
    for s in range(n):
      r = r - books[s][i0[s].long()]
      want = _group_sum((r.double() ** 2).sum(1), G)
      err = ((sse[s] - want).abs() / want.clamp(min=1e-300)).max().item()
      print('n', n, 'stage', s, 'sse rel err', err, 'bound', tol)
      assert err <= tol


# ---- 2: with a bias, fp32 -----------------------------------------------------------------------------------------------------------
def _bias_tables(case):
  """Two tables [S, G, L]: the code lengths of the plain code's histograms at lambda 0.5 (+inf on every empty bin), and a random
  finite one with one row of +inf alone."""
  M, D, L, S, G = case
  x, books = _data(case)
  _, _, hist, _ = ops.vq_res_ec_assign(x, books, None, G, S, want_y=False)
  lengths, _ = ops.vq_ec_lengths(hist.view(S * G, L), 0.5)
  g = torch.Generator().manual_seed(77 + M)
  rnd = (torch.rand(S, G, L, generator=g) * 0.5).to(DEV)
  rnd[S - 1, G - 1, :] = float('inf')
  return lengths.view(S, G, L).contiguous(), rnd.contiguous()


@pytest.mark.parametrize('which', ['lengths', 'random'])
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_bias_is_the_composed_ec_assign(case, which):
  M, D, L, S, G = case
  x, books = _data(case)
  bias = _bias_tables(case)[0 if which == 'lengths' else 1]
  if which == 'lengths' and M // G < L:
    assert bool(torch.isinf(bias).any())             # fewer vectors than bins: some bin of the plain code is empty
  i0, h0, e0 = _composed(x, books, bias, G)
  tol = M * math.ldexp(1.0, -52)                     # another order of an fp64 sum of M non-negative terms
  for n in range(1, S + 1):
    y, index, hist, sse = ops.vq_res_ec_assign(x, books, bias[:n].contiguous(), G, n)
    assert torch.equal(index, i0[:n]) and torch.equal(hist, h0[:n])
    err = ((sse - e0[:n]).abs() / e0[:n].clamp(min=1e-300)).max().item()
    print('n', n, 'sse rel err', err, 'bound', tol)
    assert err <= tol
    assert torch.equal(y, ops.vq_res_decode(index, books, n)[0])
  if which == 'random':                              # the row of +inf alone: index 0 for every vector of that group
    last = index[S - 1][_groups(M, G) == G - 1]
    assert int(last.abs().max()) == 0 and int(hist[S - 1, G - 1, 0]) == M // G


# ---- 3: bf16 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [CASES[1], CASES[2], CASES[4], CASES[8]], ids=[IDS[1], IDS[2], IDS[4], IDS[8]])
def test_bf16_input_is_widened_once_and_y_rounded_once(case):
  M, D, L, S, G = case
  x, books = _data(case)
  bias = _bias_tables(case)[0]
  xb = x.to(torch.bfloat16)
  buf = torch.empty(M * D + 1, dtype=torch.bfloat16, device=DEV)
  view = buf[1:].view(M, D)                          # two bytes off every 16-byte boundary
  view.copy_(xb)
  assert view.is_contiguous() and view.data_ptr() % 16 == 2
  for b in (None, bias):
    y32, i32, h32, e32 = ops.vq_res_ec_assign(xb.float(), books, b, G)
    for xin in (xb, view):
      y, index, hist, sse = ops.vq_res_ec_assign(xin, books, b, G)
      assert y.dtype == torch.bfloat16 and torch.equal(index, i32) and torch.equal(hist, h32) and torch.equal(sse, e32)
      assert torch.equal(y, y32.to(torch.bfloat16))


# ---- 4: an exact tie ----------------------------------------------------------------------------------------------------------------
def test_two_identical_centres_give_the_lower_index():
  g = torch.Generator().manual_seed(5)
  M, D, L, G = 600, 8, 64, 4
  books = torch.randn(2, L, D, generator=g)
  books[0, 41] = books[0, 9]                         # twins in both stages; the data sits on them
  books[1, 63] = books[1, 0]
  x = (books[0, 9] + books[1, 0]).view(1, D) + 0.01 * torch.randn(M, D, generator=g)
  x, books = x.to(DEV), books.to(DEV).contiguous()
  bias = torch.zeros(2, G, L, device=DEV)
  bias[:, :, 20:30] = float('inf')
  for b in (None, bias):
    _, index, hist, _ = ops.vq_res_ec_assign(x, books, b, G)
    assert int((index[0] == 9).sum()) > M // 2 and int((index[1] == 0).sum()) > M // 2
    assert int(hist[0, :, 41].sum()) == 0 and int(hist[1, :, 63].sum()) == 0
  assert torch.equal(ops.vq_res_ec_assign(x, books, None, G)[1], ops.vq_res_rows_fwd(x, books)[1])


# ---- 5, 6: determinism; the optional outputs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [CASES[4], CASES[7], CASES[9]], ids=[IDS[4], IDS[7], IDS[9]])
def test_two_calls_give_identical_bytes_and_optional_outputs_change_nothing(case):
  M, D, L, S, G = case
  x, books = _data(case)
  for b in (None, _bias_tables(case)[0]):
    a = ops.vq_res_ec_assign(x, books, b, G)
    c = ops.vq_res_ec_assign(x, books, b, G)
    assert all(torch.equal(u.view(torch.uint8), v.view(torch.uint8)) for u, v in zip(a, c))
    y, index, hist, sse = ops.vq_res_ec_assign(x, books, b, G, want_y=False)
    assert y is None and torch.equal(index, a[1]) and torch.equal(hist, a[2]) and torch.equal(sse, a[3])
    y, index, hist, sse = ops.vq_res_ec_assign(x, books, b, G, want_stats=False)
    assert hist is None and sse is None and torch.equal(index, a[1]) and torch.equal(y, a[0])
    y, index, hist, sse = ops.vq_res_ec_assign(x, books, b, G, want_y=False, want_stats=False)
    assert y is None and hist is None and sse is None and torch.equal(index, a[1])


# ---- 7: ResidualS2HVQ.encode_ec and usage -------------------------------------------------------------------------------------------
N_ROWS, CODE_LEN, QD, QL, QS, QG = 300, 8, 8, 32, 3, 4


def _quantizer(S=QS, dtype=torch.float32):
  g = torch.Generator().manual_seed(11)
  books = torch.stack([torch.randn(QL, QD, generator=g) * 0.6 ** s for s in range(S)])
  x = torch.randn(N_ROWS, CODE_LEN * QD, generator=g).to(DEV).to(dtype)
  return ResidualS2HVQ(books).to(DEV).eval(), x


def test_encode_ec_without_a_constraint_is_the_plain_code():
  vq, x = _quantizer()
  plain = vq.encode(x, CODE_LEN)
  for lam, n_iter in ((0.0, 2), (0, 0), (0.8, 0)):
    code, report = vq.encode_ec(x, CODE_LEN, lam, groups=QG, n_iter=n_iter)
    assert code.dtype == torch.int64 and tuple(code.shape) == (QS, N_ROWS, CODE_LEN) and torch.equal(code, plain)
    assert all(len(report[k]) == n_iter + 1 for k in ('distortion', 'bits', 'cost'))
    assert all(len(row) == QS for row in report['distortion'] + report['bits'])
  usage = vq.usage(x, CODE_LEN, groups=QG)
  assert usage.dtype == torch.int64 and torch.equal(usage, _bincount(plain.view(QS, -1), QG, QL))
  assert torch.equal(vq.usage(x, CODE_LEN, groups=QG, stages=2), usage[:2])


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_one_stage_is_s2hvqs_encode_ec(dtype):
  vq, x = _quantizer(S=1, dtype=dtype)
  one = S2HVQ(vq.code_books.detach()[0].clone()).to(DEV).eval()
  M = N_ROWS * CODE_LEN
  for lam, n_iter in ((0.5, 2), (2.0, 3)):
    code, report = vq.encode_ec(x, CODE_LEN, lam, groups=QG, n_iter=n_iter)
    code1, report1 = one.encode_ec(x, CODE_LEN, lam, groups=QG, n_iter=n_iter)
    assert torch.equal(code[0], code1)
    tol = M * math.ldexp(1.0, -52)
    for t in range(n_iter + 1):
      assert abs(report['distortion'][t][0] - report1['distortion'][t]) <= tol * report1['distortion'][t]
      assert abs(report['bits'][t][0] - report1['bits'][t]) <= tol * report1['bits'][t]
      assert abs(report['cost'][t] - report1['cost'][t]) <= 2 * tol * report1['cost'][t]


def test_encode_ec_prefix_property_report_and_stage_one_guarantee():
  vq, x = _quantizer()
  lam, n_iter = 0.6, 2
  code, report = vq.encode_ec(x, CODE_LEN, lam, groups=QG, n_iter=n_iter)
  assert not torch.equal(code, vq.encode(x, CODE_LEN))
  for n in range(1, QS + 1):                          # the first n stages are the n-stage encoder's
    code_n, report_n = vq.encode_ec(x, CODE_LEN, lam, groups=QG, n_iter=n_iter, stages=n)
    assert torch.equal(code_n, code[:n])
    assert [row[:n] for row in report['distortion']] == report_n['distortion']
    assert [row[:n] for row in report['bits']] == report_n['bits']
  # the last round's bits are the entropy of the returned code, counted on the host
  want = ref.entropy_bits(_bincount(code.view(QS, -1), QG, QL).cpu()).tolist()
  assert report['bits'][-1] == pytest.approx(want, rel=1e-12)
  assert all(report['cost'][t] == report['distortion'][t][-1] + lam * math.fsum(report['bits'][t]) or
             report['cost'][t] == report['distortion'][t][-1] + lam * sum(report['bits'][t]) for t in range(n_iter + 1))
  # against the CPU restatement: the same code
  index_ref, report_ref, _ = ref.encode_ec(x.cpu().view(-1, QD), vq.code_books.detach().cpu(), lam, QG, n_iter)
  assert torch.equal(code.view(QS, -1).cpu(), index_ref)
  assert report['bits'][-1] == pytest.approx(report_ref['bits'][-1], rel=1e-12)
  # stage 1 is ECVQ: J_1 = d_1 + lam * bits_1 does not rise over the rounds, and d_1 is smallest in round 0 (the
  # nearest centres), so bits_1 of any round <= bits_1 of round 0 + the fp32 slack of J_1 (vq_ec_ref.slack, as 4.22's test) / lam
  j1 = [report['distortion'][t][0] + lam * report['bits'][t][0] for t in range(n_iter + 1)]
  print('stage-1 cost', j1, 'stage-1 bits', [report['bits'][t][0] for t in range(n_iter + 1)])
  assert all(j1[t + 1] <= j1[t] + vq_ec_ref.slack(QD, j1[t]) for t in range(n_iter))
  assert all(report['bits'][t][0] <= report['bits'][0][0] + vq_ec_ref.slack(QD, j1[0]) / lam for t in range(1, n_iter + 1))
  assert all(report['distortion'][t][0] >= report['distortion'][0][0] * (1 - (QD + 2) * math.ldexp(1.0, -23))
             for t in range(1, n_iter + 1))
