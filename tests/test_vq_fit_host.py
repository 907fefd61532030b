"""Host tests of the code-book fit: the exported symbols and the workspace query, the refusals of the ops
wrappers, of S2HVQ.fit and of the model's fit_vq_code_book / get_vq_usage on a bare model (the one tests/test_codec_refusals.py
builds), and the properties of the float64 reference tests/vq_fit_ref.py that the GPU tests lean on.  No GPU."""
import importlib.util
import os

import pytest
import torch

import jpdse_hip
from jpdse_hip import ops
from ctu.quantizers import S2HVQ
import vq_fit_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('jpdse_vq_lloyd_workspace_size', 'jpdse_vq_lloyd_accum', 'jpdse_vq_lloyd_update')


def _load(name):
  spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'scripts', name + '.py'))
  module = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(module)
  return module


def test_symbols_are_exported_and_in_the_table():
  L = jpdse_hip.lib()
  for name in NAMES:
    assert hasattr(L, name) and name in jpdse_hip.SIGNATURES, name
  assert L.jpdse_version() == 2


def test_workspace_size_is_positive_and_grows_with_m():
  L = jpdse_hip.lib()
  for D, n_center in ((1, 2), (8, 64), (3, 5), (32, 512), (4, 16), (16, 200)):
    last = 0
    for M in (1, 2, 63, 64, 255, 256, 257, 4112, 70000, 262144, 1048576, 3000000):
      if M * n_center >= 2 ** 31:
        continue
      size = L.jpdse_vq_lloyd_workspace_size(M, D, n_center)
      assert size > 0 and size >= last, (M, D, n_center, size, last)
      last = size
  # outside the limits: 0, as the other workspace queries
  assert L.jpdse_vq_lloyd_workspace_size(16, 33, 8) == 0
  assert L.jpdse_vq_lloyd_workspace_size(16, 4, 513) == 0
  assert L.jpdse_vq_lloyd_workspace_size(16, 4, 1) == 0
  assert L.jpdse_vq_lloyd_workspace_size(0, 4, 8) == 0
  assert L.jpdse_vq_lloyd_workspace_size(2 ** 30, 4, 8) == 0


def test_null_arguments_are_refused_before_any_launch():
  L = jpdse_hip.lib()
  assert L.jpdse_vq_lloyd_accum(None) == -1 and 'vq_lloyd_accum' in jpdse_hip.last_error()
  assert L.jpdse_vq_lloyd_update(None) == -1 and 'vq_lloyd_update' in jpdse_hip.last_error()
  args = jpdse_hip.VqLloydAccumArgs(jpdse_hip.F32, 16, 4, 8, 1)           # every pointer NULL
  assert L.jpdse_vq_lloyd_accum(args) == -1 and 'null pointer' in jpdse_hip.last_error()
  args = jpdse_hip.VqLloydAccumArgs(7, 16, 4, 8, 1)
  assert L.jpdse_vq_lloyd_accum(args) == -1 and 'dtype' in jpdse_hip.last_error()
  args = jpdse_hip.VqLloydUpdateArgs(4, 600, 1)
  assert L.jpdse_vq_lloyd_update(args) == -1 and 'n_center' in jpdse_hip.last_error()


def test_ops_wrappers_refuse_bad_arguments_without_a_device():
  state = ops.vq_lloyd_state(8, 4, 'cpu')
  assert [state[k].dtype for k in ('counts', 'sums', 'sse', 'far_dist', 'far_vec')] == \
      [torch.int64, torch.float64, torch.float64, torch.float32, torch.float32]
  assert state['sums'].shape == (8, 4) and state['far_vec'].shape == (8, 4) and state['counts'].shape == (8,)
  x, c = torch.zeros(16, 4), torch.zeros(8, 4)
  with pytest.raises(AssertionError):
    ops.vq_lloyd_state(1, 4, 'cpu')
  with pytest.raises(AssertionError):
    ops.vq_lloyd_state(8, 33, 'cpu')
  with pytest.raises(AssertionError):
    ops.vq_lloyd_accum(x.double(), c, state, True)                         # dtype of x
  with pytest.raises(AssertionError):
    ops.vq_lloyd_accum(x, c.double(), state, True)                         # dtype of the book
  with pytest.raises(AssertionError):
    ops.vq_lloyd_accum(torch.zeros(16, 5), c, state, True)                 # D of x
  with pytest.raises(AssertionError):
    ops.vq_lloyd_accum(x, c, ops.vq_lloyd_state(9, 4, 'cpu'), True)        # a state of another shape
  with pytest.raises(AssertionError):
    ops.vq_lloyd_accum(x, c, dict(state, sums=state['sums'].float()), True)
  with pytest.raises(AssertionError):
    ops.vq_lloyd_accum(x, c, {k: v for k, v in state.items() if k != 'sse'}, True)
  with pytest.raises(AssertionError):
    ops.vq_lloyd_update(c.double(), state)
  with pytest.raises(AssertionError):
    ops.vq_lloyd_update(torch.zeros(8, 5), state)
  with pytest.raises(AssertionError):
    ops.vq_lloyd_update(c.view(-1), state)


def test_s2hvq_fit_refuses_bad_arguments_without_a_device():
  vq = S2HVQ(torch.zeros(8, 4))
  x = torch.zeros(6, 8)                        # 12 vectors of 4
  for bad in (-1, 1.5, True, None):
    with pytest.raises(ValueError, match='n_iter'):
      vq.fit(x, 2, n_iter=bad)
  with pytest.raises(ValueError, match='init'):
    vq.fit(x, 2, init='kmeans++')
  with pytest.raises(ValueError, match='non-empty'):
    vq.fit([], 2)
  with pytest.raises(ValueError, match='sample'):
    vq.fit(torch.zeros(3, 8), 2, init='sample')            # 6 vectors, 8 centres
  with pytest.raises(ValueError, match='sample'):
    vq.fit([torch.zeros(3, 8), x], 2)                      # the first tensor is the one sampled
  with pytest.raises(NotImplementedError, match='float64'):
    vq.fit(x.double(), 2)
  with pytest.raises(ValueError, match='code_len'):
    vq.fit(torch.zeros(6, 9), 2)
  with pytest.raises(ValueError):
    vq.fit(torch.zeros(6, 2, 4), 2)
  with pytest.raises(ValueError):
    vq.fit([x, 'text'], 2)
  with pytest.raises(jpdse_hip.JpdseError, match='no CPU fallback'):      # every host check passed: the device is next
    vq.fit(x, 2, n_iter=0, init='current')
  assert vq._code_book.grad is None and torch.equal(vq._code_book.detach(), torch.zeros(8, 4))


@pytest.mark.parametrize('quantizer', [None, 'binarizer'])
def test_model_calls_need_the_vector_quantizer(quantizer):
  mk = _load('make_codec_refusals')
  m = mk.bare_model(quantizer)
  for call in (lambda: m.fit_vq_code_book([mk.x_dict()]), lambda: m.get_vq_usage(mk.x_dict())):
    with pytest.raises(ValueError, match='--encoder_quantizer s2hvq'):
      call()


def test_model_refusals_come_before_device_work():
  mk = _load('make_codec_refusals')
  m = mk.bare_model('s2hvq')
  with pytest.raises(ValueError, match='non-empty list'):
    m.fit_vq_code_book([])
  with pytest.raises(ValueError, match='non-empty list'):
    m.fit_vq_code_book(mk.x_dict())
  with pytest.raises(ValueError, match='n_iter'):
    m.fit_vq_code_book([mk.x_dict()], n_iter=-1)
  with pytest.raises(ValueError, match='init'):
    m.fit_vq_code_book([mk.x_dict()], init='random')
  m.zero_vis = True
  with pytest.raises(ValueError, match='--zero_vis'):
    m.fit_vq_code_book([mk.x_dict()])
  m.zero_vis = False
  # past the refusals the calls reach the device hooks, which a bare model answers with this assertion
  with pytest.raises(AssertionError, match='device work before the refusal'):
    m.fit_vq_code_book([mk.x_dict()])
  with pytest.raises(AssertionError, match='device work before the refusal'):
    m.get_vq_usage(mk.x_dict())


# ---- the reference's own properties --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reseed', [True, False])
def test_reference_distortion_never_increases(reseed):
  g = torch.Generator().manual_seed(421)
  x1 = torch.randn(300, 3, generator=g, dtype=torch.float64)
  x2 = torch.randn(150, 3, generator=g, dtype=torch.float64) + 2.0
  c = torch.randn(12, 3, generator=g, dtype=torch.float64)
  c[10:] += 50.0                                # two centres far outside the data: dead at the first pass
  book, dist, dead, reseeded, counts = ref.lloyd([x1, x2], c, 8, reseed=reseed, round32=False)
  assert len(dist) == 9 and len(dead) == 8 and len(reseeded) == 8
  for a, b in zip(dist, dist[1:]):
    assert b <= a * (1 + 1e-12), dist
  assert int(counts.sum()) == 450
  assert dead[0] == 2
  if reseed:
    assert reseeded[0] == 2 and int((counts == 0).sum()) == 0
  else:
    assert reseeded == [0] * 8 and torch.equal(book[10:], c[10:])


def _hand_state(counts, sse, far_dist):
  L, D = len(counts), 2
  return dict(counts=torch.tensor(counts), sums=torch.arange(L * D, dtype=torch.float64).view(L, D),
              sse=torch.tensor(sse, dtype=torch.float64), far_dist=torch.tensor(far_dist, dtype=torch.float64),
              far_vec=100.0 + torch.arange(L * D, dtype=torch.float64).view(L, D), far_m=torch.zeros(L, dtype=torch.int64))


def test_reference_reseed_rule_on_a_hand_built_state():
  # centres 1 and 4 are dead; donors: 0, 3, 5 (2 has one member, 6 a zero farthest distance); 3 and 5 tie in sse, above 0
  st = _hand_state([4, 0, 1, 3, 0, 2, 5], [1.0, 0.0, 9.0, 2.5, 0.0, 2.5, 7.0], [0.5, -1.0, 3.0, 1.0, -1.0, 0.7, 0.0])
  assert ref.donors(st) == [3, 5, 0]
  c = torch.full((7, 2), -1.0, dtype=torch.float64)
  out, report, took = ref.update(c, st)
  assert report == (2, 2) and took == {1: 3, 4: 5}
  assert torch.equal(out[1], st['far_vec'][3]) and torch.equal(out[4], st['far_vec'][5])
  for k in (0, 2, 3, 5, 6):                     # the donors keep their means
    assert torch.equal(out[k], st['sums'][k] / float(st['counts'][k]))
  out, report, took = ref.update(c, st, reseed=False)
  assert report == (2, 0) and took == {} and torch.equal(out[1], c[1]) and torch.equal(out[4], c[4])


def test_reference_more_dead_centres_than_donors():
  st = _hand_state([0, 0, 6, 0, 2], [0.0, 0.0, 1.0, 0.0, 4.0], [-1.0, -1.0, 0.0, -1.0, 0.25])
  assert ref.donors(st) == [4]
  c = torch.full((5, 2), -3.0, dtype=torch.float64)
  out, report, took = ref.update(c, st)
  assert report == (3, 1) and took == {0: 4}
  assert torch.equal(out[0], st['far_vec'][4]) and torch.equal(out[1], c[1]) and torch.equal(out[3], c[3])


def test_reference_accumulate_streams():
  g = torch.Generator().manual_seed(5)
  x = torch.randn(90, 2, generator=g, dtype=torch.float64)
  c = torch.randn(6, 2, generator=g, dtype=torch.float64)
  index, dist = ref.assign(x, c)
  whole = ref.accumulate(x, index, dist, 6)
  part = ref.accumulate(x[:50], index[:50], dist[:50], 6)
  part = ref.accumulate(x[50:], index[50:], dist[50:], 6, part, m_offset=50)
  assert torch.equal(whole['counts'], part['counts']) and torch.equal(whole['far_vec'], part['far_vec'])
  assert torch.equal(whole['far_m'], part['far_m'])
  assert torch.allclose(whole['sums'], part['sums'], rtol=1e-13, atol=1e-13)
  assert torch.equal(whole['counts'], torch.bincount(index, minlength=6))
