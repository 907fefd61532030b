"""GPU tests of the code-book fit (vq_fit.hip: jpdse_vq_lloyd_accum, jpdse_vq_lloyd_update; ops.vq_lloyd_state / vq_lloyd_accum /
vq_lloyd_update; S2HVQ.fit) against the float64 restatement tests/vq_fit_ref.py.

Cases (M, D, L): (1, 1, 2) the smallest; (66, 8, 64) a partial wave; (255, 3, 5) odd D, L no power of two; (304, 32, 512) the
largest book (read from its transposed copy in the workspace, eight slots per lane, two centres per gather thread); (4112, 8,
64) several tiles and blocks; and the streamed pair (700, 4, 16) then (330, 4, 16).  Inputs are seeded and scaled by
(sigma D)^-1/2 as tests/test_hip_vq_rate.py scales them, two centres of a book of five or more are moved far outside the data so
that dead centres exist, and the fixture asserts on the CPU that the float64 reference alone is unambiguous: the nearest centre
of every vector and the farthest member of every centre are each clear of the runner-up by more than 1e-5 relative."""
import pytest
import torch

from jpdse_hip import ops, F32, BF16
from ctu.quantizers import S2HVQ
import hip_util as hu
import vq_util
import vq_fit_ref as ref

pytestmark = pytest.mark.gpu
DEV = hu.DEV
TOL = hu.RTOL[F32]
SIGMA = 10.0
CASES = [(1, 1, 2), (66, 8, 64), (255, 3, 5), (304, 32, 512), (4112, 8, 64)]
STREAM = ((700, 4, 16), (330, 4, 16))
KEYS = ('counts', 'sums', 'sse', 'far_dist', 'far_vec')
_cache = {}


def _dev(t, dtype=None):
  t = t.to(DEV)
  return t.to(torch.bfloat16) if dtype == BF16 else t


def _decided(x64, c64, index, dist):
  two = torch.topk(vq_util.scores(x64, c64), 2, dim=-1, largest=False).values
  assert bool(((two[:, 1] - two[:, 0]) > 1e-5 * two[:, 0]).all()), 'fixture: a vector between two centres'
  for k in range(c64.shape[0]):
    dk = dist[index == k]
    if dk.numel() >= 2:
      top = torch.topk(dk, 2).values
      assert float(top[0] - top[1]) > 1e-5 * float(top[0]), 'fixture: two farthest members of centre %d' % k


def _make(M, D, L, dtype, extra=0):
  """x (fp32 values the device dtype holds exactly; M + extra rows) and the book, with its dead centres."""
  g = torch.Generator().manual_seed(4210 + M + L)
  scale = (SIGMA * D) ** -0.5
  x = hu.quantize_like((torch.rand(M + extra, D, generator=g) * 2 - 1) * scale, dtype)
  c = (torch.rand(L, D, generator=g) * 2 - 1) * scale
  if L >= 5:
    c[1] += 50.0
    c[L - 2] -= 50.0
  return x, c


def _inputs(case, dtype):
  """(x, c, the reference's assignment and state), computed once per (case, dtype) and never modified."""
  key = (case, dtype)
  if key not in _cache:
    M, D, L = case
    x, c = _make(M, D, L, dtype)
    x64, c64 = x.double(), c.double()
    index, dist = ref.assign(x64, c64)
    _decided(x64, c64, index, dist)
    _cache[key] = (x, c, index, ref.accumulate(x64, index, dist, L))
  return _cache[key]


def _check_state(state, x, index, want, what):
  """Check 1 of the issue: the device state against the reference's for the assignment `index` of x."""
  L, D = want['sums'].shape
  got = {k: state[k].cpu() for k in KEYS}
  assert torch.equal(got['counts'], want['counts']), what
  bound = torch.zeros(L, D, dtype=torch.float64)
  bound.index_add_(0, index, x.double().abs())
  bound = bound * want['counts'].double().view(L, 1) * 2.0 ** -23
  err = (got['sums'] - want['sums']).abs()
  assert bool((err <= bound).all()), '%s: sums off by %.3e beyond the fp32 bound' % (what, float((err - bound).max()))
  hu.assert_close(got['sse'], want['sse'], TOL, what + ' sse')
  assert torch.equal(got['far_vec'], want['far_vec'].float()), what + ': far_vec bits'
  dead = want['counts'] == 0
  assert torch.equal(got['far_dist'] == -1.0, dead), what
  live = ~dead
  if bool(live.any()):
    hu.assert_close(got['far_dist'][live], want['far_dist'][live], TOL, what + ' far_dist')


@pytest.mark.parametrize('dtype', hu.DTYPES)
@pytest.mark.parametrize('case', CASES, ids=str)
def test_accumulate_matches_fp64_and_repeats_bit_identically(case, dtype):
  M, D, L = case
  x, c, index, want = _inputs(case, dtype)
  xd, cd = _dev(x, dtype), _dev(c)
  state = ops.vq_lloyd_accum(xd, cd, ops.vq_lloyd_state(L, D, DEV), True)
  hard, _ = ops.vq_hard_fwd(xd, cd)
  assert torch.equal(state['counts'].cpu(), torch.bincount(hard.cpu().long(), minlength=L))
  assert torch.equal(hard.cpu().long(), index)
  _check_state(state, x, index, want, 'vq_lloyd_accum %s' % (case,))
  assert int(state['counts'].sum()) == M
  # determinism: a second call on the same inputs, into a state that held other numbers
  again = ops.vq_lloyd_state(L, D, DEV)
  for k in KEYS:
    again[k].fill_(3)
  ops.vq_lloyd_accum(xd, cd, again, True)
  for k in KEYS:
    assert torch.equal(state[k], again[k]), k


@pytest.mark.parametrize('dtype', hu.DTYPES)
def test_streamed_batches_are_the_concatenation(dtype):
  (M1, D, L), (M2, _, _) = STREAM
  key = ('stream', dtype)
  if key not in _cache:
    x, c = _make(M1, D, L, dtype, extra=M2)
    index, dist = ref.assign(x.double(), c.double())
    _decided(x.double(), c.double(), index, dist)
    _cache[key] = (x, c, index, ref.accumulate(x.double(), index, dist, L))
  x, c, index, want = _cache[key]
  cd = _dev(c)
  x1, x2 = _dev(x[:M1].contiguous(), dtype), _dev(x[M1:].contiguous(), dtype)
  state = ops.vq_lloyd_state(L, D, DEV)
  ops.vq_lloyd_accum(x1, cd, state, True)
  ops.vq_lloyd_accum(x2, cd, state, False)
  _check_state(state, x, index, want, 'streamed')
  whole = ops.vq_lloyd_accum(_dev(x, dtype), cd, ops.vq_lloyd_state(L, D, DEV), True)
  assert torch.equal(whole['counts'], state['counts']) and torch.equal(whole['far_vec'], state['far_vec'])
  assert torch.equal(whole['far_dist'], state['far_dist'])
  # an earlier call keeps an equal distance: the same batch twice leaves the farthest members of the first pass
  twice = ops.vq_lloyd_state(L, D, DEV)
  ops.vq_lloyd_accum(x1, cd, twice, True)
  first_far = twice['far_vec'].clone()
  ops.vq_lloyd_accum(x1, cd, twice, False)
  assert torch.equal(twice['far_vec'], first_far)
  once = ops.vq_lloyd_accum(x1, cd, ops.vq_lloyd_state(L, D, DEV), True)
  assert torch.equal(twice['counts'], 2 * once['counts'])


def _ref_state_of(state):
  st = {k: state[k].cpu() for k in KEYS}
  return dict(counts=st['counts'], sums=st['sums'], sse=st['sse'], far_dist=st['far_dist'].double(), far_vec=st['far_vec'].double())


def _check_update(c, state, reseed, what):
  """ops.vq_lloyd_update on a copy of c against the rule applied to the device's own state."""
  st = _ref_state_of(state)
  book = c.clone()
  report = ops.vq_lloyd_update(book, state, reseed=reseed)
  want, want_report, took = ref.update(c.cpu().double(), st, reseed)
  got = book.cpu()
  live = st['counts'] > 0
  mean = (st['sums'] / st['counts'].double().clamp_min(1).view(-1, 1)).float()
  assert torch.equal(got[live], mean[live]), what + ': the means, bit for bit'
  for k in torch.nonzero(~live).view(-1).tolist():
    src = st['far_vec'][took[k]].float() if k in took else c[k].cpu()
    assert torch.equal(got[k], src), '%s: dead centre %d' % (what, k)
  assert torch.equal(got, want.float()), what
  assert tuple(report.cpu().tolist()) == want_report, what
  return want_report


@pytest.mark.parametrize('dtype', hu.DTYPES)
@pytest.mark.parametrize('case', CASES, ids=str)
def test_update_from_the_device_state(case, dtype):
  M, D, L = case
  x, c, _, _ = _inputs(case, dtype)
  cd = _dev(c)
  state = ops.vq_lloyd_accum(_dev(x, dtype), cd, ops.vq_lloyd_state(L, D, DEV), True)
  dead, reseeded = _check_update(cd, state, True, 'update %s' % (case,))
  assert dead >= (2 if L >= 5 else 1)
  assert _check_update(cd, state, False, 'update without reseed %s' % (case,)) == (dead, 0)
  assert torch.equal(cd.cpu(), c)                          # the checks worked on copies


def _hand_state(counts, sse, far_dist, D=3):
  L = len(counts)
  g = torch.Generator().manual_seed(L)
  st = ops.vq_lloyd_state(L, D, DEV)
  st['counts'].copy_(torch.tensor(counts))
  st['sums'].copy_(torch.randn(L, D, generator=g, dtype=torch.float64))
  st['sse'].copy_(torch.tensor(sse, dtype=torch.float64))
  st['far_dist'].copy_(torch.tensor(far_dist))
  st['far_vec'].copy_(torch.randn(L, D, generator=g))
  return st, torch.randn(L, D, generator=g).to(DEV)


def test_update_rule_on_hand_built_states():
  # two dead centres, three donors with a tie in sse (the lower k first); 2 has one member, 6 a zero farthest distance
  st, c = _hand_state([4, 0, 1, 3, 0, 2, 5], [1.0, 0.0, 9.0, 2.5, 0.0, 2.5, 7.0], [0.5, -1.0, 3.0, 1.0, -1.0, 0.7, 0.0])
  assert _check_update(c, st, True, 'tie') == (2, 2)
  book = c.clone()
  ops.vq_lloyd_update(book, st)
  assert torch.equal(book[1], st['far_vec'][3]) and torch.equal(book[4], st['far_vec'][5])
  assert _check_update(c, st, False, 'tie, no reseed') == (2, 0)
  # more dead centres than donors: the surplus stays
  st, c = _hand_state([0, 0, 6, 0, 2], [0.0, 0.0, 1.0, 0.0, 4.0], [-1.0, -1.0, 0.0, -1.0, 0.25])
  assert _check_update(c, st, True, 'surplus') == (3, 1)
  book = c.clone()
  ops.vq_lloyd_update(book, st)
  assert torch.equal(book[0], st['far_vec'][4]) and torch.equal(book[1], c[1]) and torch.equal(book[3], c[3])
  # the largest book, every other centre dead, donors in descending order of k
  L = 512
  counts = [0 if k % 2 else 3 for k in range(L)]
  st, c = _hand_state(counts, [float(k) for k in range(L)], [-1.0 if k % 2 else 1.0 for k in range(L)], D=32)
  assert _check_update(c, st, True, '512') == (256, 256)
  book = c.clone()
  ops.vq_lloyd_update(book, st)
  assert torch.equal(book[1], st['far_vec'][510]) and torch.equal(book[511], st['far_vec'][0])


# ---- S2HVQ.fit -----------------------------------------------------------------------------------------------------------------
FIT_L, FIT_D, PER = 16, 2, 40


def _clustered(dtype):
  """FIT_L lattice points one unit apart plus uniform noise of +-0.05, PER vectors each, shuffled; the lattice itself."""
  g = torch.Generator().manual_seed(77)
  lattice = torch.stack([torch.tensor([float(i % 4), float(i // 4)]) for i in range(FIT_L)])
  x = lattice.repeat_interleave(PER, dim=0) + (torch.rand(FIT_L * PER, FIT_D, generator=g) * 2 - 1) * 0.05
  x = hu.quantize_like(x[torch.randperm(FIT_L * PER, generator=g)], dtype)
  start = lattice + (torch.rand(FIT_L, FIT_D, generator=g) * 2 - 1) * 0.1
  return x, lattice, start


@pytest.mark.parametrize('dtype', hu.DTYPES)
def test_fit_on_clustered_data(dtype):
  x, lattice, start = _clustered(dtype)
  n_iter = 3
  vq = S2HVQ(start.clone().to(DEV), sigma=SIGMA)
  sentinel = torch.full((FIT_L, FIT_D), 0.25, device=DEV)
  vq._code_book.grad = sentinel
  ptr = vq._code_book.data_ptr()
  half = FIT_L * PER // 2
  out = vq.fit(_dev(x[half:].contiguous(), dtype), 1, n_iter=0, init='current')
  assert len(out['distortion']) == 1 and out['dead'] == [] and out['reseeded'] == []
  assert torch.equal(vq._code_book.detach().cpu(), start)
  x64 = x.double()
  want_book, want_dist, want_dead, want_res, want_counts = ref.lloyd([x64], start.double(), n_iter)
  out = vq.fit(_dev(x, dtype), 1, n_iter=n_iter, init='current')
  assert vq._code_book.data_ptr() == ptr and vq._code_book.requires_grad
  assert vq._code_book.grad is sentinel and bool((sentinel == 0.25).all())
  hu.assert_close(vq._code_book.detach().cpu(), want_book, TOL, 'fitted book')
  assert len(out['distortion']) == n_iter + 1 and all(isinstance(v, float) for v in out['distortion'])
  hu.assert_close(torch.tensor(out['distortion']), torch.tensor(want_dist), TOL, 'distortion')
  for a, b in zip(out['distortion'], out['distortion'][1:]):
    assert b <= a * (1 + TOL), out['distortion']
  assert out['dead'] == want_dead == [0] * n_iter and out['reseeded'] == want_res
  assert out['counts'].dtype == torch.int64 and torch.equal(out['counts'].cpu(), want_counts)
  assert torch.equal(out['counts'].cpu(), torch.full((FIT_L,), PER))
  # a list of batches is the same fit as their concatenation, up to the order of the fp64 merge
  vq2 = S2HVQ(start.clone().to(DEV), sigma=SIGMA)
  out2 = vq2.fit([_dev(x[:half].contiguous(), dtype), _dev(x[half:].contiguous(), dtype)], 1, n_iter=n_iter, init='current')
  hu.assert_close(vq2._code_book.detach().cpu(), want_book, TOL, 'fitted book, two batches')
  assert torch.equal(out2['counts'], out['counts'])
  # code_len > 1: rows of 4 vectors are the same vectors
  vq3 = S2HVQ(start.clone().to(DEV), sigma=SIGMA)
  vq3.fit(_dev(x.reshape(-1, 4 * FIT_D).contiguous(), dtype), 4, n_iter=n_iter, init='current')
  assert torch.equal(vq3._code_book.detach(), vq._code_book.detach())


@pytest.mark.parametrize('dtype', hu.DTYPES)
def test_fit_init_sample_and_reseeding(dtype):
  x, lattice, start = _clustered(dtype)
  xd = _dev(x, dtype)
  M = x.shape[0]
  vq = S2HVQ(torch.zeros(FIT_L, FIT_D, device=DEV), sigma=SIGMA)
  ptr = vq._code_book.data_ptr()
  vq.fit(xd, 1, n_iter=0, init='sample', seed=5)
  book = vq._code_book.detach().cpu()
  pick = torch.randperm(M, generator=torch.Generator().manual_seed(5))[:FIT_L]
  assert len(set(pick.tolist())) == FIT_L and torch.equal(book, x[pick])       # rows of x, bit for bit, from distinct vectors
  for row in book:
    assert bool((x == row).all(dim=1).any())
  assert vq._code_book.data_ptr() == ptr
  vq.fit(xd, 1, n_iter=0, init='sample', seed=5)
  assert torch.equal(vq._code_book.detach().cpu(), book)
  vq.fit(xd, 1, n_iter=0, init='sample', seed=6)
  assert not torch.equal(vq._code_book.detach().cpu(), book)
  with pytest.raises(ValueError, match='sample'):
    vq.fit(xd[:FIT_L - 1].contiguous(), 1)
  # one centre far outside the data: dead at the first pass, reseeded by the update, in use afterwards
  far = lattice.clone()
  far[5] = torch.tensor([100.0, -100.0])
  vq = S2HVQ(far.to(DEV), sigma=SIGMA)
  out = vq.fit(xd, 1, n_iter=1, init='current')
  assert out['dead'] == [1] and out['reseeded'] == [1]
  assert int((out['counts'] == 0).sum()) == 0 and int(out['counts'].sum()) == M
  assert out['distortion'][1] < out['distortion'][0]
  # without reseeding the centre stays dead, and stays where it was
  vq = S2HVQ(far.to(DEV), sigma=SIGMA)
  out = vq.fit(xd, 1, n_iter=2, init='current', reseed=False)
  assert out['dead'] == [1, 1] and out['reseeded'] == [0, 0] and int(out['counts'][5]) == 0
  assert torch.equal(vq._code_book.detach()[5].cpu(), far[5])
