"""CPU-only checks of the per-class distortion (jpdse_eval_metrics_sem): the new C-ABI entries are declared,
exported and refuse bad arguments before any launch, the integer yardstick of the GPU test (tests/class_metrics_ref.py) is
pinned to a hand-computed example, the host half (ops.eval_metrics_per_class) is checked on hand-made tables, and the three
ablation flags are no longer refused.  No device kernel is launched here."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import jpdse_hip
from jpdse_hip import F32, BF16

import class_metrics_ref as cref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('jpdse_eval_metrics_sem_workspace_size', 'jpdse_eval_metrics_sem')


def test_new_symbols_are_declared_and_exported():
  header = open(os.path.join(ROOT, 'include', 'jpdse.h')).read()
  declared = set(re.findall(r'\b(jpdse_[a-zA-Z0-9_]+)\s*\(', header))
  L = jpdse_hip.lib()
  dev = ctypes.CDLL(jpdse_hip.DEV_LIB_PATH)
  for name in NEW_SYMBOLS:
    assert name in declared, name + ' missing from include/jpdse.h'
    assert name in jpdse_hip.SIGNATURES
    assert hasattr(L, name) and hasattr(dev, name)
  assert L.jpdse_version() == 2


def test_workspace_size_is_zero_for_unsupported_shapes_and_class_counts():
  L = jpdse_hip.lib()
  size, plain = L.jpdse_eval_metrics_sem_workspace_size, L.jpdse_eval_metrics_workspace_size
  for shape in ((1, 175, 400, 3), (1, 400, 175, 3), (1, 256, 256, 4), (0, 256, 256, 3)):
    assert size(*shape, 35) == 0, shape
  for n_classes in (0, -1, 257):
    assert size(1, 256, 256, 3, n_classes) == 0, n_classes
  # the plain workspace plus one partial row of (n_classes + 1) x 3 64-bit counters per block and image
  for shape in ((1, 176, 176, 3), (4, 512, 1024, 3)):
    assert plain(*shape) < size(*shape, 1) < size(*shape, 35) < size(*shape, 256)
    blocks = min(-(-shape[1] * shape[2] // 1024), 1024)
    extra = size(*shape, 35) - plain(*shape)
    assert shape[0] * blocks * 36 * 3 * 8 <= extra < shape[0] * blocks * 36 * 3 * 8 + 256


def test_bad_arguments_are_refused_before_any_launch():
  L = jpdse_hip.lib()
  dummy = (ctypes.c_double * 16)()
  p = ctypes.cast(dummy, ctypes.c_void_p)
  m = (ctypes.c_double * 3)(0.5, 0.5, 0.5)

  def call(df=F32, dr=F32, n=1, h=256, w=256, c=3, label=p, n_classes=35, cls=p, fake=p, out=p, nbytes=1 << 30):
    v = lambda q: q.value if q is not None else None
    a = jpdse_hip.EvalMetricsSemArgs(df, dr, n, h, w, c, v(fake), v(p), v(label), n_classes, m, m, v(out), v(cls), v(p), nbytes,
                                     None)
    return L.jpdse_eval_metrics_sem(ctypes.byref(a))
  for n_classes in (0, -3, 257):
    assert call(n_classes=n_classes) == -1 and 'n_classes' in jpdse_hip.last_error()
  assert call(label=None) == -1 and 'null' in jpdse_hip.last_error()
  assert call(cls=None) == -1 and 'null' in jpdse_hip.last_error()
  assert call(fake=None) == -1 and 'null' in jpdse_hip.last_error()
  assert call(out=None) == -1 and 'null' in jpdse_hip.last_error()
  # the shape limits of jpdse_eval_metrics
  assert call(df=BF16, h=175, w=512) == -1 and '176' in jpdse_hip.last_error()
  assert call(h=512, w=175) == -1 and '176' in jpdse_hip.last_error()
  assert call(c=1) == -1 and 'channels' in jpdse_hip.last_error()
  assert call(dr=BF16) == -1 and 'real' in jpdse_hip.last_error()
  assert call(df=2) == -1 and 'fake' in jpdse_hip.last_error()
  # the plain call's workspace is one class-partial area short
  plain = L.jpdse_eval_metrics_workspace_size(1, 256, 256, 3)
  assert call(nbytes=plain) == -2 and 'workspace' in jpdse_hip.last_error()
  assert L.jpdse_eval_metrics_sem(None) == -1 and 'null' in jpdse_hip.last_error()
  with pytest.raises(jpdse_hip.JpdseError):
    jpdse_hip.check(call(n_classes=300), 'eval_metrics_sem')


# ---- the yardstick -----------------------------------------------------------------------------------------------------------
def test_yardstick_on_a_hand_computed_2x2_example():
  """One 2x2 image, n_classes 3.  Pixels (row-major): labels 0, 2, 0, 7 (7 is a stray).  Per pixel and channel q(fake) -
  q(real):  p0 (1, -2, 0)  p1 (0, 0, 0)  p2 (-3, 4, 5)  p3 (10, 0, -1)."""
  qr = np.full((1, 3, 2, 2), 100, dtype=np.uint8)
  d = np.array([[1, 0, -3, 10], [-2, 0, 4, 0], [0, 0, 5, -1]]).reshape(1, 3, 2, 2)
  qf = (qr.astype(np.int64) + d).astype(np.uint8)
  label = np.array([0.0, 2.0, 0.0, 7.0]).reshape(1, 1, 2, 2)
  tab = cref.table(qf, qr, label, 3)
  assert tab.dtype == np.int64 and tab.shape == (1, 4, 3)
  assert tab[0].tolist() == [[3 + 12, 5 + 50, 2],      # class 0: p0 (|d| 3, d^2 5) and p2 (|d| 12, d^2 50)
                             [0, 0, 0],                # class 1: absent
                             [0, 0, 1],                # class 2: p1, exact
                             [11, 101, 1]]             # strays: p3
  r = cref.per_class(tab)
  assert r['pixels'].tolist() == [2, 0, 1] and r['unlabelled'] == 1
  assert r['l1'].tolist() == [15 / 6, 0.0, 0.0] and r['mse'].tolist() == [55 / 6, 0.0, 0.0]
  assert r['psnr'][0] == 10.0 * math.log10(255.0 ** 2 / (55 / 6)) and math.isnan(r['psnr'][1]) and r['psnr'][2] == math.inf
  assert r['per_image']['l1'].shape == (1, 3)


def test_yardstick_class_index_sends_every_stray_to_the_extra_row():
  lab = np.array([-1.0, 0.0, 3.5, 34.0, 35.0, 255.0, np.nan, -0.0, 1e9])
  assert cref.class_index(lab, 35).tolist() == [35, 0, 35, 34, 35, 35, 35, 0, 35]


# ---- the host half -----------------------------------------------------------------------------------------------------------
def test_per_class_dict_is_pixel_weighted_and_marks_absent_and_exact_classes():
  from jpdse_hip import ops
  # two images, three classes + the extra row; class 0 has very different areas in the two images, class 1 is exact,
  # class 2 is absent from both
  cls = torch.tensor([[[30, 300, 10], [0, 0, 5], [0, 0, 0], [7, 49, 1]],
                      [[9000, 90000, 1000], [0, 0, 0], [0, 0, 0], [0, 0, 0]]], dtype=torch.int64)
  r = ops.eval_metrics_per_class(cls)
  assert set(r) == {'pixels', 'l1', 'mse', 'psnr', 'unlabelled', 'per_image', 'raw'}
  assert r['pixels'].dtype == torch.int64 and r['pixels'].tolist() == [1010, 5, 0]
  for k in ('l1', 'mse', 'psnr'):
    assert r[k].dtype == torch.float64 and tuple(r[k].shape) == (3,) and r[k].device.type == 'cpu'
    assert r['per_image'][k].dtype == torch.float64 and tuple(r['per_image'][k].shape) == (2, 3)
  assert r['per_image']['pixels'].dtype == torch.int64 and r['per_image']['pixels'].tolist() == [[10, 5, 0], [1000, 0, 0]]
  assert r['unlabelled'] == 1 and isinstance(r['unlabelled'], int)
  # pixel-weighted: (30 + 9000) / (3 * 1010), not the mean of 1.0 and 3.0
  assert r['l1'].tolist() == [9030 / 3030, 0.0, 0.0] and r['l1'][0].item() != 2.0
  assert r['mse'].tolist() == [90300 / 3030, 0.0, 0.0]
  assert r['per_image']['l1'].tolist() == [[1.0, 0.0, 0.0], [3.0, 0.0, 0.0]]
  assert r['per_image']['mse'].tolist() == [[10.0, 0.0, 0.0], [30.0, 0.0, 0.0]]
  assert r['psnr'][0].item() == pytest.approx(10.0 * math.log10(255.0 ** 2 / (90300 / 3030)), rel=1e-14)
  assert r['psnr'][1].item() == math.inf and math.isnan(r['psnr'][2].item())
  p = r['per_image']['psnr']
  assert p[0, 1].item() == math.inf and math.isnan(p[1, 1].item()) and math.isnan(p[0, 2].item())
  # and it is the yardstick's dict
  want = cref.per_class(cls.numpy())
  for k in ('pixels', 'l1', 'mse'):
    assert np.array_equal(r[k].numpy(), want[k]) and np.array_equal(r['per_image'][k].numpy(), want['per_image'][k])
  assert np.allclose(r['psnr'].numpy(), want['psnr'], rtol=1e-14, atol=0, equal_nan=True)   # log10 of two libms: a few ulp


def test_public_calls_take_per_class_and_the_default_is_unchanged():
  from jpdse_hip import ops
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  from ctu.trainers.pix2pixHD_trainer import Pix2PixHDTrainer
  for cls in (Pix2PixHDModel, Pix2PixHDTrainer):
    par = inspect.signature(cls.get_eval_metrics).parameters
    assert list(par) == ['self', 'x_dict', 'per_class'] and par['per_class'].default is False
  par = inspect.signature(ops.eval_metrics).parameters
  assert list(par) == ['fake', 'real32', 'mean', 'std', 'label', 'n_classes']
  assert par['label'].default is None and par['n_classes'].default is None


@pytest.mark.parametrize('flag', ['zero_sem', 'zero_ins', 'zero_vis'])
def test_zero_flags_left_the_refused_list(flag, monkeypatch):
  """Pix2PixHDModel.__init__ names every refused flag in one NotImplementedError before any network exists: beside a flag that
  is still refused, the ablation flag is no longer named.  Checked with the GPU hidden and the library out of reach."""
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  from oracle.ctu_cpu import model as omodel
  import jpdse_hip.ops  # noqa: F401
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  touched = lambda: (_ for _ in ()).throw(AssertionError('library touched'))
  monkeypatch.setattr(jpdse_hip, 'lib', touched)
  monkeypatch.setattr(jpdse_hip.ops, 'lib', touched)
  opt = omodel.default_opt(gpu_ids=[0], ngf=8, ndf=8, n_blocks_global=1, sem_masking=True, **{flag: True})
  with pytest.raises(NotImplementedError) as e:
    Pix2PixHDModel(opt)
  assert '--sem_masking' in str(e.value) and '--' + flag not in str(e.value)
