"""GPU tests of the entropy-constrained assignment (vq_ec.hip: jpdse_vq_ec_assign, jpdse_vq_ec_lengths; ops.vq_ec_assign /
vq_ec_lengths; S2HVQ.encode_ec) against the float64 restatement tests/vq_ec_ref.py.

Shapes (M, D, L, G): (2, 1, 2, 1) the smallest; (66, 3, 10, 2) odd D, L no power of two, a partial wave; (80, 8, 64, 16) the
bottleneck's shape, tables in LDS; (64, 32, 257, 1) five slots per lane, a book of 32 KiB; (1040, 32, 512, 16) the largest book,
several tiles and blocks, tables and bias through L2.  Both dtypes; a bf16 x is rounded first and the reference sees the rounded
values.  Tolerances are derived (the fp32 rounding of D terms and one add), never measured."""
import math

import pytest
import torch

from jpdse_hip import ops, BF16
from ctu.quantizers import S2HVQ
import hip_util as hu
import vq_ec_ref as ref

pytestmark = pytest.mark.gpu
DEV = hu.DEV
SHAPES = [(2, 1, 2, 1), (66, 3, 10, 2), (80, 8, 64, 16), (64, 32, 257, 1), (1040, 32, 512, 16)]
EPS = math.ldexp(1.0, -24)
INF = float('inf')


def _x(t, dtype):
  """(device tensor in dtype, the float64 values it holds)."""
  d = t.to(DEV)
  d = d.to(torch.bfloat16) if dtype == BF16 else d.float()
  return d.contiguous(), d.cpu().to(torch.float64)


def _dev(t):
  return t.to(DEV).float().contiguous()


def _float_case(M, D, L, G, seed):
  g = torch.Generator().manual_seed(seed)
  return torch.randn(M, D, generator=g), torch.randn(L, D, generator=g), 4.0 * torch.rand(G, L, generator=g)


def _integer_case(M, D, L, G, seed):
  """Integer x and centres with |v| <= 8, a bias of multiples of 0.25 in [0, 16]; vectors drawn by rejection until the minimum
  cost of each is unique.  Every cost is an exact float32."""
  g = torch.Generator().manual_seed(seed)
  c = torch.randint(-8, 9, (L, D), generator=g).float()
  while torch.unique(c, dim=0).shape[0] != L:
    c = torch.randint(-8, 9, (L, D), generator=g).float()
  bias = torch.randint(0, 65, (G, L), generator=g).float() * 0.25
  x = torch.zeros(M, D)
  todo = torch.arange(M)
  for _ in range(400):
    x[todo] = torch.randint(-8, 9, (todo.numel(), D), generator=g).float()
    two = torch.topk(ref.cost(x, c, bias, G), 2, dim=-1, largest=False).values
    todo = torch.nonzero(two[:, 0] == two[:, 1])[:, 0]
    if todo.numel() == 0:
      return x, c, bias
  raise AssertionError('no %d vectors with a unique minimum cost for D %d, L %d' % (M, D, L))


@pytest.mark.parametrize('dtype', hu.DTYPES)
@pytest.mark.parametrize('shape', SHAPES)
def test_zero_bias_is_the_hard_assignment(shape, dtype):
  M, D, L, G = shape
  x, c, _ = _float_case(M, D, L, G, 11)
  xd, _ = _x(x, dtype)
  cd = _dev(c)
  want, _ = ops.vq_hard_fwd(xd, cd)
  for bias in (None, torch.zeros(G, L, device=DEV)):
    index, hist, _ = ops.vq_ec_assign(xd, cd, bias, G)
    assert torch.equal(index, want)
    assert torch.equal(hist.cpu().to(torch.int64), ref.hist_of(want.cpu(), G, L))
    only, none_h, none_s = ops.vq_ec_assign(xd, cd, bias, G, want_hist=False, want_sse=False)
    assert none_h is None and none_s is None and torch.equal(only, want)


@pytest.mark.parametrize('dtype', hu.DTYPES)
@pytest.mark.parametrize('shape', SHAPES)
def test_integer_inputs_are_exact(shape, dtype):
  M, D, L, G = shape
  x, c, bias = _integer_case(M, D, L, G, 5)
  xd, x64 = _x(x, dtype)
  assert torch.equal(x64, x.to(torch.float64))
  index, hist, sse = ops.vq_ec_assign(xd, _dev(c), _dev(bias), G)
  want, want_hist, want_sse = ref.assign(x64, c, bias, G)
  assert torch.equal(index.cpu().to(torch.int64), want)
  assert torch.equal(hist.cpu().to(torch.int64), want_hist)
  assert torch.equal(sse.cpu(), want_sse)


def test_ties_go_to_the_lowest_index():
  """Equal costs from different (d, bias) pairs.  D = 1, x = 0: d[k] = c[k]^2.  L = 130: lane 5 owns 5, 69; lane 6 owns 6, 70;
  lane 1 owns 1, 65, 129."""
  L = 130
  c = torch.full((L, 1), 3.0)                      # d = 9
  bias = torch.zeros(1, L)
  x = torch.zeros(3, 1)
  c[[5, 69, 70, 129], 0] = torch.tensor([1.0, 2.0, 0.0, -2.0])
  bias[0, [5, 69, 70, 129]] = torch.tensor([4.0, 1.0, 5.0, 1.0])      # four costs of 5: (1, 4), (4, 1), (0, 5), (4, 1)

  def run():
    return ops.vq_ec_assign(_dev(x), _dev(c), _dev(bias), 1)[0].cpu().tolist()

  assert run() == [5, 5, 5]
  bias[0, 5] = 4.5                                 # inside a lane's slots went; now across lanes: 69 (lane 5) and 70 (lane 6)
  assert run() == [69, 69, 69]
  bias[0, 69] = 1.5                                # slot 1 of lane 6 against slot 2 of lane 1
  assert run() == [70, 70, 70]
  bias[0, 70] = 5.5
  assert run() == [129, 129, 129]
  bias[0, 5], bias[0, 69] = 4.0, 1.0               # slots 0 and 1 of lane 5 again, and 129 of lane 1: 5 wins
  assert run() == [5, 5, 5]
  # two groups, the same vectors: group 1 carries a row that lifts the four to the 9 of every plain centre: index 0 wins
  two = torch.cat([bias, torch.zeros(1, L)])
  two[1, [5, 69, 70, 129]] = torch.tensor([8.0, 5.0, 9.0, 5.0])
  assert ops.vq_ec_assign(_dev(torch.zeros(4, 1)), _dev(c), _dev(two), 2)[0].cpu().tolist() == [5, 0, 5, 0]


@pytest.mark.parametrize('shape', [(66, 3, 10, 2), (80, 8, 64, 16), (1040, 32, 512, 16)])
def test_an_infinite_bias_is_never_chosen(shape):
  M, D, L, G = shape
  x, c, bias = _float_case(M, D, L, G, 7)
  xd, x64 = _x(x, hu.DTYPES[0])
  plain = ref.argmin_lowest(ref.cost(x64, c, None, G))
  bias = torch.zeros(G, L)
  grp = torch.arange(M) % G
  head = torch.arange(min(M, 2 * G))               # the plain winners of the first vectors are forbidden in their groups
  bias[grp[head], plain[head]] = INF
  index, hist, sse = ops.vq_ec_assign(xd, _dev(c), _dev(bias), G)
  index = index.cpu().to(torch.int64)
  assert bool(torch.isfinite(bias[grp, index]).all())
  assert bool((hist.cpu()[torch.isinf(bias)] == 0).all())
  # one finite entry per group wins for every vector
  one = torch.full((G, L), INF)
  keep = (torch.arange(G) * 7 + 3) % L
  one[torch.arange(G), keep] = 2.5
  index, hist, sse = ops.vq_ec_assign(xd, _dev(c), _dev(one), G)
  assert torch.equal(index.cpu().to(torch.int64), keep[grp])
  assert bool(torch.isfinite(sse).all())
  # a row of +inf alone: index 0, and the distortion of centre 0 (no NaN)
  index, hist, sse = ops.vq_ec_assign(xd, _dev(c), torch.full((G, L), INF, device=DEV), G)
  assert bool((index == 0).all()) and bool(torch.isfinite(sse).all())
  want = ref.sse_of(x64, c, torch.zeros(M, dtype=torch.int64), G)
  assert bool(((sse.cpu() - want).abs() <= (D + 2) * EPS * want).all())


@pytest.mark.parametrize('dtype', hu.DTYPES)
@pytest.mark.parametrize('shape', SHAPES)
def test_float_inputs_within_the_rounding_of_the_score_loop(shape, dtype):
  M, D, L, G = shape
  x, c, bias = _float_case(M, D, L, G, 3)
  xd, x64 = _x(x, dtype)
  cd, bd = _dev(c), _dev(bias)
  index, hist, sse = ops.vq_ec_assign(xd, cd, bd, G)
  index = index.cpu().to(torch.int64)
  J = ref.cost(x64, c, bias, G)
  chosen = J.gather(1, index[:, None])[:, 0]
  bound = ref.slack(D, chosen)
  two = torch.topk(J, 2, dim=-1, largest=False)
  excess = chosen - two.values[:, 0]
  print('max (J[chosen] - min J) / bound = %.3g' % float((excess / bound).max()))
  assert bool((excess <= bound).all())             # every vector
  clear = (two.values[:, 1] - two.values[:, 0]) > 2 * bound
  assert bool((index[clear] == two.indices[:, 0][clear]).all())
  assert torch.equal(hist.cpu().to(torch.int64), ref.hist_of(index, G, L))
  want = ref.sse_of(x64, c, index, G)
  err = ((sse.cpu() - want).abs() / want).max()
  print('sse: max relative error %.3g, bound %.3g' % (float(err), (D + 2) * EPS))
  assert float(err) <= (D + 2) * EPS
  # determinism: a second call on the same buffers
  again = ops.vq_ec_assign(xd, cd, bd, G)
  assert torch.equal(again[0].cpu().to(torch.int64), index) and torch.equal(again[1], hist) and torch.equal(again[2], sse)


@pytest.mark.parametrize('lam', [0.0, 0.75, 1e6])
@pytest.mark.parametrize('G,L', [(1, 2), (2, 10), (16, 64), (3, 257), (16, 512)])
def test_lengths(G, L, lam):
  g = torch.Generator().manual_seed(G * L)
  hist = torch.randint(0, 50, (G, L), generator=g, dtype=torch.int32)
  hist[torch.rand(G, L, generator=g) < 0.3] = 0
  hist[:, 0] += 1                                  # no empty row
  if L > 2:
    hist[G - 1, 1:] = 0                            # one centre holds a whole group: length 0
  bias, bits = ops.vq_ec_lengths(hist.to(DEV), lam)
  want, want_bits = ref.lengths(hist, lam)
  bias, bits = bias.cpu().to(torch.float64), bits.cpu()
  empty = hist == 0
  if lam == 0:
    assert bool((bias == 0).all())
  else:
    assert bool((bias[empty] == INF).all()) and bool(torch.isfinite(bias[~empty]).all())
    assert bool(((bias[~empty] - want[~empty]).abs() <= 1e-6 * want[~empty]).all())
  assert bool(((bits - want_bits).abs() <= 1e-12 * want_bits).all())
  again = ops.vq_ec_lengths(hist.to(DEV), lam)
  assert torch.equal(again[0].cpu().to(torch.float64), bias) and torch.equal(again[1].cpu(), bits)


@pytest.mark.parametrize('dtype', hu.DTYPES)
@pytest.mark.parametrize('case', [(66, 3, 10, 2), (80, 8, 64, 16), (1040, 32, 512, 16)])
def test_encode_ec(case, dtype):
  M, D, L, G = case
  x, c, _ = _float_case(M, D, L, G, 19)
  half = torch.arange(M) < (3 * M) // 4            # uneven usage: most of every group sits next to one centre of its own
  fav = ((torch.arange(M) % G) * 5 + 1) % L
  x = torch.where(half[:, None], c[fav] + 0.05 * x, x)
  xd, x64 = _x(x, dtype)
  vq = S2HVQ(c.clone().to(DEV), sigma=10.0).eval()
  plain = vq.encode(xd, 1, train=False, raw=False)
  for lam, n_iter in ((0.0, 2), (0.7, 0)):
    code, report = vq.encode_ec(xd, 1, lam, groups=G, n_iter=n_iter)
    assert code.dtype == torch.int64 and tuple(code.shape) == (M, 1) and torch.equal(code, plain)
    assert all(len(report[k]) == n_iter + 1 for k in ('distortion', 'bits', 'cost'))
  lam, n_iter = 0.7, 3
  code, report = vq.encode_ec(xd, 1, lam, groups=G, n_iter=n_iter)
  index = code.cpu().view(-1)
  d_last = float(ref.sse_of(x64, c, index, G).sum())
  b_last = float(ref.lengths(ref.hist_of(index, G, L), lam)[1].sum())
  cost_last = d_last + lam * b_last
  slack = ref.slack(D, cost_last)
  print('cost', report['cost'], 'recomputed last', cost_last, 'slack', slack)
  assert abs(report['cost'][-1] - cost_last) <= slack
  assert all(report['cost'][t + 1] <= report['cost'][t] + ref.slack(D, report['cost'][t]) for t in range(n_iter))
  assert all(report['cost'][t] == report['distortion'][t] + lam * report['bits'][t] for t in range(n_iter + 1))
  # a huge multiplier: every group's code is its most frequent plain centre.  (With two centres tied for the most frequent the
  # distortion would decide between them in round 1: the fixture has a single one per group.)
  code, _ = vq.encode_ec(xd, 1, 1e6, groups=G, n_iter=2)
  hist = ref.hist_of(plain.cpu().view(-1), G, L)
  top = ref.argmin_lowest(-hist.to(torch.float64))
  assert bool(((hist == hist.max(dim=-1, keepdim=True).values).sum(dim=-1) == 1).all()), 'fixture: two most frequent centres'
  assert torch.equal(code.cpu().view(-1), top[torch.arange(M) % G])
