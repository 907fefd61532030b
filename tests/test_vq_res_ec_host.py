"""Host-only checks of the entropy-constrained residual code: the two entry points of the library with every
refusal they make before a launch, the checks the new model and trainer calls run before device work, and the CPU restatement
(vq_res_ec_ref.py) against a case worked by hand.  Nothing here launches a kernel."""
import ctypes
import importlib.util
import math
import os

import pytest
import torch

import jpdse_hip
from jpdse_hip import F32
import vq_res_ec_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
  spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'scripts', name + '.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


MAKER = _load('make_model_option_refusals')


# ---- the library ----------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_points():
  lib = jpdse_hip.lib()
  for name in ('jpdse_vq_res_ec_assign', 'jpdse_vq_res_ec_workspace_size'):
    assert name in jpdse_hip.SIGNATURES and callable(getattr(lib, name))
  assert lib.jpdse_version() == 2


def test_workspace_size_is_the_stated_function_and_zero_outside_the_limits():
  size = jpdse_hip.lib().jpdse_vq_res_ec_workspace_size
  # blocks = min(tiles, 2^22 / (n G L), 1024); bytes = blocks * n * G * (8 + 4 L)
  assert size(1000, 8, 64, 4, 3) == 4 * 3 * 4 * (8 + 4 * 64)                       # 4 tiles
  assert size(1 << 20, 8, 64, 16, 4) == 1024 * 4 * 16 * (8 + 4 * 64)               # the block cap
  assert size(1 << 20, 32, 512, 16, 8) == 64 * 8 * 16 * (8 + 4 * 512)              # the table cap: 2^22 / 65536
  for bad in ((0, 8, 64, 1, 1), (10, 33, 64, 1, 1), (10, 8, 1, 1, 1), (10, 8, 64, 0, 1), (10, 8, 64, 3, 1), (10, 8, 64, 1, 0),
              (10, 8, 64, 1, 9), (4096, 8, 512, 64, 3), (1 << 20, 8, 512, 256, 1)):
    assert size(*bad) == 0, bad


def test_assign_refuses_on_the_host():
  lib = jpdse_hip.lib()
  P = 0x1000                                                  # never dereferenced: every call below is refused first

  def args(**kw):
    v = dict(dtype=F32, M=12, D=8, L=64, S=4, n_stages=4, G=2, x=P, books=P, bias=None, y=P, index=P, hist=None, sse=None, ws=None,
             ws_bytes=0, stream=None)
    v.update(kw)
    return jpdse_hip.VqResEcAssignArgs(**v)

  need = lib.jpdse_vq_res_ec_workspace_size(12, 8, 64, 2, 4)
  assert need > 0
  cases = ((args(n_stages=0), 'n_stages = 0'), (args(n_stages=5), 'n_stages = 5'), (args(S=9, n_stages=9), 'S = 9 stages'),
           (args(D=33), 'center_size D = 33'), (args(L=1), 'n_center L = 1'), (args(M=0), 'M = 0'), (args(dtype=7), 'bad dtype'),
           (args(G=0), 'G = 0 groups'), (args(G=5), 'G = 5 does not divide M = 12'),
           (args(M=4096, L=512, G=256), 'G * L = 131072'),
           (args(M=4096, L=512, G=64, n_stages=3), 'n_stages * G * L = 98304'),
           (args(x=None), 'null pointer'), (args(books=None), 'null pointer'), (args(index=None), 'null pointer'),
           (args(hist=P), 'hist and sse come together'), (args(sse=P), 'hist and sse come together'),
           (args(hist=P, sse=P), 'workspace too small'), (args(hist=P, sse=P, ws=P, ws_bytes=need - 1), 'workspace too small'),
           (args(hist=P, sse=P, ws=P + 4, ws_bytes=need), 'workspace not 8-byte aligned'))
  for a, field in cases:
    assert lib.jpdse_vq_res_ec_assign(ctypes.byref(a)) == -1, field
    assert field in jpdse_hip.last_error() and 'vq_res_ec_assign' in jpdse_hip.last_error(), (field, jpdse_hip.last_error())
  assert lib.jpdse_vq_res_ec_assign(None) == -1 and 'null argument struct' in jpdse_hip.last_error()


# ---- the quantizer module: refused before the device ------------------------------------------------------------------------------
def test_quantizer_arguments_are_checked_before_device_work():
  from ctu.quantizers import ResidualS2HVQ
  vq = ResidualS2HVQ(torch.zeros(3, 8, 4))
  x = torch.zeros(6, 8)
  with MAKER.hidden_device():
    for lam in (-1.0, float('inf'), float('nan'), 'x'):
      with pytest.raises(ValueError, match='lam must be a finite number >= 0'):
        vq.encode_ec(x, 2, lam)
    for n_iter in (-1, 1.0, True):
      with pytest.raises(ValueError, match='n_iter must be an int >= 0'):
        vq.encode_ec(x, 2, 0.5, n_iter=n_iter)
    for stages in (0, 4, True, 1.0):
      with pytest.raises(ValueError, match='stages must be an int in 1 .. 3'):
        vq.encode_ec(x, 2, 0.5, stages=stages)
      with pytest.raises(ValueError, match='stages must be an int in 1 .. 3'):
        vq.usage(x, 2, stages=stages)
    for groups in (0, 5):
      with pytest.raises(ValueError, match='groups must divide n \\* code_len'):
        vq.encode_ec(x, 2, 0.5, groups=groups)
      with pytest.raises(ValueError, match='groups must divide n \\* code_len'):
        vq.usage(x, 2, groups=groups)
    big = ResidualS2HVQ(torch.zeros(3, 512, 4))
    with pytest.raises(NotImplementedError, match='stages \\* groups \\* n_center = 98304'):
      big.encode_ec(torch.zeros(64, 4), 1, 0.5, groups=64)
    with pytest.raises(jpdse_hip.JpdseError, match='no CPU fallback'):      # a good call gets as far as the device check
      vq.encode_ec(x, 2, 0.5)


# ---- the model and the trainer ----------------------------------------------------------------------------------------------------
HOST = None


def _stages_host():
  """The fakes of test_vq_stages_host.py (a bare model over a fake three-stage encoder), loaded as a module."""
  global HOST
  if HOST is None:
    spec = importlib.util.spec_from_file_location('vq_stages_host_fakes', os.path.join(ROOT, 'tests', 'test_vq_stages_host.py'))
    HOST = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(HOST)
  return HOST


EC_CALLS = ['get_stage_code_ec', 'get_coded_stages_ec', 'get_stage_ec_report']
INSTEAD = {'get_stage_code_ec': 'get_vq_code(rate_lambda=)', 'get_coded_stages_ec': 'get_coded_ec',
           'get_stage_ec_report': 'get_vq_ec_report', 'get_stage_usage': 'get_vq_usage', 'get_stage_rates': 'get_vq_rate'}


@pytest.mark.parametrize('call', EC_CALLS)
def test_ec_calls_check_their_arguments_before_device_work(call):
  h = _stages_host()
  m = h._bare_model(h._codec())
  for target in (m, h._bare_trainer(m)):
    with MAKER.hidden_device():
      for lam in (-0.5, float('inf'), float('nan'), None):
        with pytest.raises(ValueError, match='lam must be a finite number >= 0'):
          getattr(target, call)(h.X_DICT, lam)
      for n_iter in (-1, 2.0, True):
        with pytest.raises(ValueError, match='n_iter must be an int >= 0'):
          getattr(target, call)(h.X_DICT, 0.5, n_iter=n_iter)
      for stages in (0, 4, True, 1.0, 'all'):
        with pytest.raises(ValueError, match=r'%s: stages must be an int in 1 .. 3 \(vq_stages\)' % call):
          getattr(target, call)(h.X_DICT, 0.5, stages=stages)
      for good in (dict(), dict(stages=1), dict(stages=3, n_iter=0)):          # a good call gets as far as the device
        with pytest.raises(AssertionError, match='device work'):
          getattr(target, call)(h.X_DICT, 0.5, **good)
        with pytest.raises(AssertionError, match='device work'):
          getattr(target, call)(h.X_DICT, 0.0, **good)


def test_usage_and_rates_reach_the_device_on_a_stage_model_only():
  h = _stages_host()
  m = h._bare_model(h._codec())
  for target in (m, h._bare_trainer(m)):
    for call in ('get_stage_usage', 'get_stage_rates'):
      with MAKER.hidden_device(), pytest.raises(AssertionError, match='device work'):
        getattr(target, call)(h.X_DICT)


@pytest.mark.parametrize('call', sorted(INSTEAD))
def test_a_one_stage_model_is_refused_by_name(call):
  from ctu.models.codec import VQIndexCodec
  h = _stages_host()
  m = h._bare_model(VQIndexCodec(h._FakeEncoder(), F32))
  args = (h.X_DICT, 0.5) if call in EC_CALLS else (h.X_DICT,)
  for target in (m, h._bare_trainer(m)):
    with MAKER.hidden_device(), pytest.raises(ValueError) as err:
      getattr(target, call)(*args)
    text = str(err.value)
    assert text.startswith(call + ': ') and 'vq_stages = 1' in text and text.endswith('use ' + INSTEAD[call]), text


def test_stage_curve_checks_the_rate_arguments_first():
  h = _stages_host()
  tr = h._bare_trainer(h._bare_model(h._codec()))
  with MAKER.hidden_device():
    with pytest.raises(ValueError, match='lam must be a finite number >= 0'):
      tr.get_stage_curve(h.X_DICT, rate_lambda=-1)
    with pytest.raises(ValueError, match='n_iter must be an int >= 0'):
      tr.get_stage_curve(h.X_DICT, rate_lambda=0.5, n_iter=-2)
    for kw in (dict(), dict(rate_lambda=0.5)):
      with pytest.raises(AssertionError, match='device work'):
        tr.get_stage_curve(h.X_DICT, **kw)


def test_the_pinned_one_stage_calls_still_refuse_a_stage_model():
  h = _stages_host()
  m = h._bare_model(h._codec())
  for call, kw in h.CALLS:
    with MAKER.hidden_device(), pytest.raises(ValueError, match='vq_stages = 3'):
      getattr(m, call)(h.X_DICT, **kw)


# ---- the reference module against a case worked by hand ---------------------------------------------------------------------------
def test_reference_on_a_hand_worked_two_stage_two_centre_case():
  """D = 1, two stages of two centres, G = 2 (vector m in group m % 2).
  books: C_1 = {0, 4}, C_2 = {-1, 1}.  x = [0.5, 3.0, 1.9, 2.1].
  No bias.   stage 1: d = [(0.25, 12.25), (9, 1), (3.61, 4.41), (4.41, 3.61)] -> k = [0, 1, 0, 1], r_2 = [0.5, -1, 1.9, -1.9]
             stage 2: d = [(2.25, 0.25), (0, 4), (8.41, 0.81), (0.81, 8.41)] -> k = [1, 0, 1, 0], y = [1, 3, 1, 3]
  With bias[0] = [[0, 0], [2, 0]] (group 1 pays 2 for centre 0 of stage 1) and bias[1] = [[+inf, +inf], [0, +inf]]:
             stage 1: group 1 holds x = 3.0 and 2.1: costs (11, 1), (6.41, 3.61) -> unchanged, k = [0, 1, 0, 1]
             stage 2: group 0 (vectors 0, 2) sees +inf alone -> index 0; group 1 -> centre 0: k = [0, 0, 0, 0]
             sse of stage 2 WITHOUT the bias: group 0: 2.25 + 8.41, group 1: 0 + 0.81."""
  books = torch.tensor([[[0.0], [4.0]], [[-1.0], [1.0]]])
  x = torch.tensor([[0.5], [3.0], [1.9], [2.1]])
  y, index, hist, sse = ref.assign(x, books, None, groups=2)
  assert index.tolist() == [[0, 1, 0, 1], [1, 0, 1, 0]]
  assert y.view(-1).tolist() == [1.0, 3.0, 1.0, 3.0]
  assert hist.tolist() == [[[2, 0], [0, 2]], [[0, 2], [2, 0]]]
  f = lambda v: float(torch.tensor(v, dtype=torch.float32))
  r2 = [f(0.5), f(3.0) - f(4.0), f(1.9), f(2.1) - f(4.0)]
  sq = lambda a, b: f(f(a - b) ** 2)             # one component: the fp32 difference, then its square rounded once
  assert sse[0].tolist() == [sq(f(0.5), 0) + sq(f(1.9), 0), sq(f(3.0), 4) + sq(f(2.1), 4)]
  assert sse[1].tolist() == [sq(r2[0], 1) + sq(r2[2], 1), sq(r2[1], -1) + sq(r2[3], -1)]
  assert sse.sum(1).tolist() == pytest.approx([0.25 + 1 + 3.61 + 3.61, 0.25 + 0 + 0.81 + 0.81], rel=1e-6)
  inf = float('inf')
  bias = torch.tensor([[[0.0, 0.0], [2.0, 0.0]], [[inf, inf], [0.0, inf]]])
  y, index, hist, sse = ref.assign(x, books, bias, groups=2)
  assert index.tolist() == [[0, 1, 0, 1], [0, 0, 0, 0]]
  assert y.view(-1).tolist() == [-1.0, 3.0, -1.0, 3.0]
  assert hist[1].tolist() == [[2, 0], [2, 0]]
  assert sse[1].tolist() == [sq(r2[0], -1) + sq(r2[2], -1), sq(r2[1], -1) + sq(r2[3], -1)]
  # a tie keeps the lower index; a stage prefix is the shorter code
  tie = torch.tensor([[[1.0], [1.0]], [[0.0], [0.0]]])
  assert ref.assign(x, tie)[1].tolist() == [[0] * 4, [0] * 4]
  assert ref.assign(x, books, bias[:1], groups=2, n_stages=1)[1].tolist() == index[:1].tolist()


def test_reference_lengths_and_rounds():
  hist = torch.tensor([[[3, 1, 0, 0]], [[2, 2, 0, 0]]])
  bias, bits = ref.lengths(hist, 0.5)
  assert bits.view(-1).tolist() == pytest.approx([3 * math.log2(4 / 3) + 2.0, 4.0], rel=1e-15)
  assert bias[0, 0].tolist() == [float(torch.tensor(0.5 * math.log2(4 / 3), dtype=torch.float32)), 1.0, float('inf'), float('inf')]
  assert ref.lengths(hist, 0.0)[0].abs().sum() == 0 and ref.entropy_bits(hist).tolist() == bits.sum(-1).tolist()
  g = torch.Generator().manual_seed(0)
  x, books = torch.randn(200, 3, generator=g), torch.randn(2, 6, 3, generator=g) * torch.tensor([1.0, 0.4]).view(2, 1, 1)
  plain = ref.assign(x, books, None, 2)[1]
  for lam, n_iter in ((0.0, 2), (0.7, 0)):
    index, report, _ = ref.encode_ec(x, books, lam, 2, n_iter)
    assert torch.equal(index, plain) and len(report['cost']) == n_iter + 1
  index, report, hist = ref.encode_ec(x, books, 0.7, 2, 2)
  assert report['bits'][2][0] <= report['bits'][0][0] and not torch.equal(index, plain)      # stage 1: ECVQ's guarantee
  assert report['bits'][2] == ref.entropy_bits(hist).tolist()
  assert torch.equal(ref.encode_ec(x, books, 0.7, 2, 2, n_stages=1)[0], index[:1])            # the prefix property
