"""CPU-only checks of the entropy-constrained assignment: both libraries export the entry points, the size
query refuses every shape outside the limits, the Python refusals come without a GPU and without touching the library, and the
float64 restatement the GPU tests compare against (tests/vq_ec_ref.py) has the property the iteration is built on: its cost never
increases."""
import ctypes

import pytest
import torch

import jpdse_hip
import vq_ec_ref as ref
from test_quantizers_host import hidden_gpu  # noqa: F401  (the fixture)

EC_SYMBOLS = ('jpdse_vq_ec_workspace_size', 'jpdse_vq_ec_assign', 'jpdse_vq_ec_lengths')


def test_both_libraries_export_the_entry_points():
  for path in (jpdse_hip.LIB_PATH, jpdse_hip.DEV_LIB_PATH):
    handle = ctypes.CDLL(path)
    for name in EC_SYMBOLS:
      assert hasattr(handle, name), (path, name)
      assert name in jpdse_hip.SIGNATURES
  assert jpdse_hip.lib().jpdse_version() == 2


def test_workspace_size_is_zero_outside_the_limits():
  size = jpdse_hip.lib().jpdse_vq_ec_workspace_size
  assert size(80, 8, 64, 16) > 0 and size(2, 1, 2, 1) > 0 and size(1040, 32, 512, 16) > 0
  assert size(128, 32, 512, 128) > 0                       # G * L == 65536
  for bad in ((0, 8, 64, 1), (80, 0, 64, 1), (80, 33, 64, 1), (80, 8, 1, 1), (80, 8, 513, 1), (1 << 25, 8, 64, 1),
              (80, 8, 64, 0), (80, 8, 64, -1), (80, 8, 64, 3), (258, 8, 512, 129), (129 * 4, 8, 512, 129)):
    assert size(*bad) == 0, bad
  # host only: a refused launch reports before any device work
  args = jpdse_hip.VqEcAssignArgs(jpdse_hip.F32, 80, 8, 64, 3, None, None, None, None, None, None, None, 0, None)
  assert jpdse_hip.lib().jpdse_vq_ec_assign(ctypes.byref(args)) != 0
  assert b'does not divide' in jpdse_hip.lib().jpdse_last_error()
  largs = jpdse_hip.VqEcLengthsArgs(1, 64, -1.0, None, None, None, None)
  assert jpdse_hip.lib().jpdse_vq_ec_lengths(ctypes.byref(largs)) != 0
  assert b'lambda' in jpdse_hip.lib().jpdse_last_error()


def test_encode_ec_refusals_need_no_device(hidden_gpu):  # noqa: F811
  from ctu.quantizers import S2HVQ
  vq = S2HVQ(torch.zeros(8, 4))
  x = torch.zeros(6, 8)
  for lam in (-1.0, float('nan'), float('inf'), -float('inf'), 'much'):
    with pytest.raises(ValueError, match='lam must be a finite number >= 0'):
      vq.encode_ec(x, 2, lam)
  for n_iter in (-1, 1.5, True, None):
    with pytest.raises(ValueError, match='n_iter must be an int >= 0'):
      vq.encode_ec(x, 2, 1.0, n_iter=n_iter)
  with pytest.raises(ValueError, match='groups must divide'):
    vq.encode_ec(x, 2, 1.0, groups=5)
  with pytest.raises(ValueError, match='code_len must divide'):
    vq.encode_ec(torch.zeros(6, 9), 2, 1.0)


def test_model_call_refusals_need_no_device(hidden_gpu):  # noqa: F811
  from ctu.models.codec import BinaryCodec, VQIndexCodec
  from ctu.models.coded_calls import CodedCalls

  class Bare(CodedCalls):
    def __init__(self, codec):
      self.codec = codec

  binary, vq = Bare(BinaryCodec(None, None)), Bare(VQIndexCodec(None, None))
  for call in ('get_coded_ec', 'get_coded_rate_ec'):
    with pytest.raises(ValueError, match='--encoder_quantizer s2hvq'):
      getattr(binary, call)({}, rate_lambda=1.0)
  with pytest.raises(ValueError, match='needs --encoder_quantizer s2hvq'):      # its existing refusal, first
    binary.get_vq_code({}, rate_lambda=1.0)
  for call in ('get_vq_code', 'get_coded_ec', 'get_coded_rate_ec', 'get_vq_ec_report'):
    for lam in (-0.5, float('nan'), float('inf')):
      with pytest.raises(ValueError, match='lam must be a finite number >= 0'):
        getattr(vq, call)({}, rate_lambda=lam)
    with pytest.raises(ValueError, match='n_iter must be an int >= 0'):
      getattr(vq, call)({}, rate_lambda=1.0, n_iter=-2)


@pytest.mark.parametrize('shape', [(66, 3, 10, 2), (256, 4, 16, 4), (300, 8, 64, 1)])
@pytest.mark.parametrize('lam', [0.0, 0.3, 2.0, 50.0])
def test_the_restatement_never_increases_its_cost(shape, lam):
  M, D, L, G = shape
  g = torch.Generator().manual_seed(M + L)
  x, c = torch.randn(M, D, generator=g, dtype=torch.float64), torch.randn(L, D, generator=g, dtype=torch.float64)
  index, report = ref.encode_ec(x, c, lam, G, 4)
  cost = report['cost']
  assert all(cost[t + 1] <= cost[t] * (1 + 1e-12) for t in range(4)), cost
  plain = ref.argmin_lowest(ref.scores(x, c))
  if lam == 0:
    assert torch.equal(index, plain)
  else:
    assert report['bits'][-1] <= report['bits'][0] and report['distortion'][-1] >= report['distortion'][0] * (1 - 1e-12)
  # lengths: an empty bin is +inf, a full one 0, and the bits are the entropy of the histogram
  bias, bits = ref.lengths(torch.tensor([[4, 0, 4], [8, 0, 0]]), 2.0)
  assert bias.tolist() == [[2.0, ref.INF, 2.0], [0.0, ref.INF, ref.INF]] and bits.tolist() == [8.0, 0.0]
