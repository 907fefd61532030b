"""CPU-only checks of ctu.quantizers: the torch restatement the GPU tests compare against (tests/vq_util.py)
is pinned to the REAL reference through tests/golden/s2hvq.npz (scripts/make_golden_s2hvq.py); the module imports and refuses
what it must refuse without a GPU and without touching the library; the shipped library exports the new entry points."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

import jpdse_hip
import vq_util

VQ_SYMBOLS = ('jpdse_vq_workspace_size', 'jpdse_vq_soft_fwd', 'jpdse_vq_hard_fwd', 'jpdse_vq_soft_bwd', 'jpdse_vq_decode',
              'jpdse_vq_decode_bwd', 'jpdse_vq_argmax', 'jpdse_vq_pmf', 'jpdse_vq_pmf_bwd')
REL = 1e-6       # max|a - b| <= REL * max|b|: the same float32 torch operations in another grouping


def golden_configs(golden_dir):
  z = np.load(os.path.join(golden_dir, 's2hvq.npz'))
  n = len({k.split('_')[0] for k in z.files})
  return [{k[len('c%d_' % i):]: z[k] for k in z.files if k.startswith('c%d_' % i)} for i in range(n)]


def _close(a, b, what):
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  assert a.shape == b.shape, (what, a.shape, b.shape)
  err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
  assert err <= REL, '%s: max|a-b| / max|b| = %.3e > %.0e' % (what, err, REL)


@pytest.fixture
def hidden_gpu(monkeypatch):
  """No GPU, and any touch of the library is an error (the pattern of test_still_refused_combinations_...)."""
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  touched = lambda: (_ for _ in ()).throw(AssertionError('library touched'))
  import jpdse_hip.ops  # noqa: F401
  monkeypatch.setattr(jpdse_hip, 'lib', touched)
  monkeypatch.setattr(jpdse_hip.ops, 'lib', touched)           # ops binds `lib` at import time


def test_helper_reproduces_the_reference_golden(golden_dir):
  configs = golden_configs(golden_dir)
  assert len(configs) >= 3
  for i, gold in enumerate(configs):
    n, d, code_len, L = (int(v) for v in gold['cfg'][:4])
    sigma = float(gold['cfg'][4])
    x, c = torch.from_numpy(gold['x']), torch.from_numpy(gold['code_book'])
    r, q = torch.from_numpy(gold['r']), torch.from_numpy(gold['q'])
    xg, cg = x.clone().requires_grad_(True), c.clone().requires_grad_(True)
    soft = vq_util.encode(xg, cg, code_len, sigma)
    _close(soft.detach(), gold['soft'], 'config %d soft code_raw' % i)
    vq_util.golden_loss(xg, cg, code_len, sigma, r, q).backward()
    _close(xg.grad, gold['gx'], 'config %d dx' % i)
    _close(cg.grad, gold['gc'], 'config %d dC' % i)
    # the stated backward formulas give the same gradients as autograd through the forward
    dx, dc = vq_util.soft_bwd(r.view(-1, L), soft.detach().view(-1, L), x.view(-1, d // code_len), c, sigma)
    index = vq_util.argmax_lowest(soft.detach().view(-1, L))
    _close(dx.view(n, d), gold['gx'], 'config %d dx by formula' % i)
    _close(dc + vq_util.decode_bwd(index, q.view(-1, d // code_len), L), gold['gc'], 'config %d dC by formula' % i)
    with torch.no_grad():
      hard = vq_util.encode(x, c, code_len, sigma, train=False)
      assert np.array_equal(hard.numpy(), gold['hard']), i
      assert np.array_equal(vq_util.encode(x, c, code_len, sigma, train=False, raw=False).numpy(), gold['hard_code']), i
      assert np.array_equal(vq_util.encode(x, c, code_len, sigma, raw=False).numpy(), gold['soft_code']), i
      assert np.array_equal(vq_util.decode_raw(hard, c).numpy(), gold['decode_hard']), i
      assert np.array_equal(vq_util.decode_raw(soft.detach(), c).numpy(), gold['decode']), i
      pm = vq_util.pmf(soft.detach())
      _close(pm, gold['pmf'], 'config %d pmf' % i)
      assert np.array_equal(vq_util.pmf(hard).numpy(), gold['pmf_hard']), i
      _close(torch.stack([vq_util.cross_entropy(pm, pm), vq_util.cross_entropy(vq_util.pmf(hard), pm)]), gold['xent'],
             'config %d cross entropy' % i)
    xg2 = x.clone().requires_grad_(True)
    (vq_util.pmf(vq_util.encode(xg2, c, code_len, sigma)) * torch.arange(L, dtype=torch.float32)).sum().backward()
    _close(xg2.grad, gold['gpmf_x'], 'config %d d pmf / dx' % i)


def test_import_works_without_a_gpu_and_without_the_library(hidden_gpu):
  for name in [m for m in sys.modules if m == 'ctu.quantizers' or m.startswith('ctu.quantizers.')]:
    del sys.modules[name]
  mod = importlib.import_module('ctu.quantizers')
  from ctu.quantizers import S2HVQ, S2HVQV2  # noqa: F401
  assert mod.S2HVQ is S2HVQ
  vq = S2HVQ(torch.randn(10, 5), sigma=1)
  assert list(vq.state_dict().keys()) == ['_code_book']           # the reference's parameter name
  assert vq.center_size == 5 and vq.sigma == 1 and vq.code_book is vq._code_book
  vq.sigma = 3.5
  assert vq.sigma == 3.5
  with pytest.raises(AssertionError):
    vq.sigma = 0
  with pytest.raises(AssertionError):
    S2HVQ(torch.randn(10, 5), sigma=-1.)
  # n_center numbers in plain torch: no device needed
  p = torch.tensor([0.5, 0.25, 0.25, 0.0])
  assert abs(float(S2HVQ.get_cross_entropy(p, p)) - 1.5) < 1e-6
  with pytest.raises(AssertionError):
    S2HVQ.get_cross_entropy(p * 2, p)


def test_encode_value_errors_come_before_any_library_call(hidden_gpu):
  from ctu.quantizers import S2HVQ
  vq = S2HVQ(torch.randn(10, 5), sigma=1)
  x = torch.randn(100, 15)
  with pytest.raises(ValueError, match='greater than or equal to code_len, got 15 and 20'):
    vq.encode(x=x, code_len=20)
  with pytest.raises(ValueError, match='code_len must divide x.size\\(1\\), got 7 and 15'):
    vq.encode(x=x, code_len=7)
  with pytest.raises(ValueError, match='Illegal code_len.*got 15, 5, and 5'):
    vq.encode(x=x, code_len=5)
  with pytest.raises(ValueError):
    vq.decode(torch.randn(4, 3, 9))
  # a legal call on a CPU tensor: the error require_gpu() raises, still without the library
  with pytest.raises(jpdse_hip.JpdseError, match='no CPU fallback'):
    vq.encode(x=x, code_len=3)
  with pytest.raises(jpdse_hip.JpdseError, match='no CPU fallback'):
    vq.decode(torch.randn(4, 3, 10))
  with pytest.raises(jpdse_hip.JpdseError, match='no CPU fallback'):
    S2HVQ.get_pmf(torch.rand(4, 3, 10))


def test_unsupported_variants_raise_not_implemented(hidden_gpu):
  from ctu.quantizers import S2HVQ, S2HVQV2
  with pytest.raises(NotImplementedError, match='Linear'):
    S2HVQV2(code_book=torch.randn(10, 5), sigma=1.)
  with pytest.raises(NotImplementedError, match='center_size 33'):
    S2HVQ(torch.randn(10, 33))
  with pytest.raises(NotImplementedError, match='n_center 513'):
    S2HVQ(torch.randn(513, 4))
  with pytest.raises(NotImplementedError, match='n_center 1'):
    S2HVQ(torch.randn(1, 4))
  with pytest.raises(NotImplementedError, match='float32'):
    S2HVQ(torch.randn(10, 4, dtype=torch.float64))
  vq = S2HVQ(torch.randn(512, 1))
  with pytest.raises(NotImplementedError, match='float32 and bfloat16'):
    vq.encode(torch.randn(4, 3, dtype=torch.float64), code_len=3)
  huge = torch.empty(1).expand(2 ** 22, 1)                       # no storage: 2^22 vectors x 512 centres = 2^31
  with pytest.raises(NotImplementedError, match='2\\^31'):
    vq.encode(huge, code_len=1)
  with pytest.raises(NotImplementedError, match='2\\^31'):
    S2HVQ.get_pmf(torch.empty(1).expand(2 ** 22, 1, 512))


def test_library_exports_the_vq_entry_points():
  L = jpdse_hip.lib()
  dev = ctypes.CDLL(jpdse_hip.DEV_LIB_PATH)
  for name in VQ_SYMBOLS:
    assert name in jpdse_hip.SIGNATURES, name
    assert hasattr(L, name) and hasattr(dev, name), name
  # host-only query: the limits and a size that grows with the code book
  assert L.jpdse_vq_workspace_size(1025, 32, 512) >= 3 * 512 * 32 * 4
  assert L.jpdse_vq_workspace_size(1025, 8, 64) >= 3 * 64 * 8 * 4
  for M, D, Lc in ((0, 8, 64), (16, 0, 64), (16, 33, 64), (16, 8, 1), (16, 8, 513), (2 ** 22, 8, 512)):
    assert L.jpdse_vq_workspace_size(M, D, Lc) == 0, (M, D, Lc)
