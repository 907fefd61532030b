"""CPU-only checks of the evaluation metrics (jpdse_eval_metrics): the float64 MS-SSIM yardstick the GPU test
compares the kernel with (tests/msssim_ref.py) is pinned to closed forms, the new C-ABI entries are declared, exported and
refuse unsupported shapes before any launch, and the host half (ops.eval_metrics_finish: PSNR, the MS-SSIM product and its
clamp) is checked on hand-made read-backs.  No device kernel is launched here."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import jpdse_hip
from jpdse_hip import F32, BF16

import msssim_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('jpdse_eval_metrics_workspace_size', 'jpdse_eval_metrics')


def _noise(h, w, seed):
  return np.random.RandomState(seed).randint(0, 256, size=(3, h, w)).astype(np.uint8)


def test_yardstick_window_is_the_normalised_11x11_gaussian():
  w = ref.window()
  assert w.shape == (11, 11) and abs(w.sum() - 1.0) < 1e-15
  assert np.array_equal(w, w.T) and np.array_equal(w, w[::-1, ::-1])
  assert abs(w[5, 5] / w[5, 6] - math.exp(1.0 / (2 * 1.5 ** 2))) < 1e-12
  assert (ref.C1, ref.C2) == ((0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2)
  assert abs(sum(ref.WEIGHTS) - 1.0) < 1e-3 and len(ref.WEIGHTS) == 5


def test_yardstick_identical_images_give_exactly_one():
  x = _noise(176, 200, 1)
  r = ref.ms_ssim(x, x.copy())
  assert r['ms_ssim'] == 1.0
  assert np.all(r['cs'] == 1.0) and np.all(r['ssim'] == 1.0)


@pytest.mark.parametrize('a,b', [(100, 140), (3, 250), (255, 254)])
def test_yardstick_constant_images_match_the_closed_form(a, b):
  x = np.full((3, 180, 176), a, dtype=np.uint8)
  y = np.full((3, 180, 176), b, dtype=np.uint8)
  r = ref.ms_ssim(x, y)
  want = (2.0 * a * b + ref.C1) / (a * a + b * b + ref.C1)
  np.testing.assert_allclose(r['cs'], 1.0, rtol=0, atol=1e-9)       # variances are rounding noise against C2 = 58.5
  np.testing.assert_allclose(r['ssim'], want, rtol=1e-9, atol=0)
  assert abs(r['ms_ssim'] - want ** ref.WEIGHTS[4]) <= 1e-9


def test_yardstick_refuses_a_175_pixel_side():
  ok = _noise(176, 176, 2)
  ref.ms_ssim(ok, ok)
  for h, w in ((175, 300), (300, 175)):
    z = _noise(h, w, 3)
    with pytest.raises(ValueError):
      ref.ms_ssim(z, z)


def test_yardstick_negative_scale_mean_gives_zero_not_nan():
  x = (np.random.RandomState(4).randint(0, 2, size=(3, 176, 176)) * 255).astype(np.uint8)
  y = 255 - x                                    # anti-correlated: s_xy = -s_x^2, so cs < 0 wherever s_x^2 > C2 / 2
  r = ref.ms_ssim(x, y)
  assert r['cs'][0] < 0
  assert r['ms_ssim'] == 0.0 and not math.isnan(r['ms_ssim'])


def test_yardstick_scales_follow_the_2x2_mean_with_odd_edges_dropped():
  a = np.arange(3 * 5 * 7, dtype=np.float64).reshape(3, 5, 7)
  d = ref.downsample(a)
  assert d.shape == (3, 2, 3)
  assert d[1, 1, 2] == a[1, 2:4, 4:6].mean()
  # a direct evaluation of one position of one scale-1 map, written out from the definition
  x, y = _noise(176, 176, 5).astype(np.float64), _noise(176, 176, 6).astype(np.float64)
  cs, ss = ref.scale_maps(x, y)
  assert cs.shape == (3, 166, 166)
  w = ref.window()
  px, py = x[2, 40:51, 7:18], y[2, 40:51, 7:18]
  mx, my = (w * px).sum(), (w * py).sum()
  sxx, syy, sxy = (w * px * px).sum() - mx * mx, (w * py * py).sum() - my * my, (w * px * py).sum() - mx * my
  want_cs = (2 * sxy + ref.C2) / (sxx + syy + ref.C2)
  assert abs(cs[2, 40, 7] - want_cs) < 1e-12
  assert abs(ss[2, 40, 7] - want_cs * (2 * mx * my + ref.C1) / (mx * mx + my * my + ref.C1)) < 1e-12


def test_yardstick_quantiser_truncates_like_tensor2im():
  x = np.array([-1.2, -1.0, -0.999, 0.0, 0.0039, 0.999, 1.0, 1.7]).reshape(1, 1, 8).repeat(3, axis=0)
  q = ref.quantise(x, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
  assert q.dtype == np.uint8 and q[0, 0].tolist() == [0, 0, 0, 127, 127, 254, 255, 255]


def test_golden_pairs_have_positive_scale_means():
  z = np.load(os.path.join(ROOT, 'tests', 'golden', 'eval_metrics_pairs.npz'))
  assert sorted(z.files) == ['jpeg_q10', 'jpeg_q40', 'jpeg_q85', 'original']
  orig = z['original']
  assert orig.dtype == np.uint8 and orig.shape == (176, 208, 3)
  last = 0.0
  for q in (10, 40, 85):
    r = ref.ms_ssim(orig, z['jpeg_q%d' % q])
    assert min(r['cs'].min(), r['ssim'].min()) > 0
    assert last < r['ms_ssim'] < 1.0           # a better JPEG is closer to the original
    last = r['ms_ssim']


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
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


def test_unsupported_shapes_are_refused_before_any_launch():
  L = jpdse_hip.lib()
  size = L.jpdse_eval_metrics_workspace_size
  assert size(1, 176, 176, 3) > 0 and size(4, 512, 1024, 3) > size(1, 512, 1024, 3)
  assert size(1, 175, 400, 3) == 0 and size(1, 400, 175, 3) == 0 and size(1, 256, 256, 4) == 0 and size(0, 256, 256, 3) == 0
  # two planes of every scale, both images, must fit: >= 2 * 3 * 4 bytes * H * W * (1 + 1/4 + ...)
  assert size(1, 512, 1024, 3) >= 2 * 3 * 4 * 512 * 1024 * 1.33
  dummy = (ctypes.c_double * 16)()
  p = ctypes.cast(dummy, ctypes.c_void_p)
  m = (ctypes.c_double * 3)(0.5, 0.5, 0.5)

  def call(df, dr, n, h, w, c, nbytes=1 << 30):
    return L.jpdse_eval_metrics(df, dr, n, h, w, c, p, p, m, m, p, p, nbytes, None)
  assert call(BF16, F32, 1, 175, 512, 3) == -1 and '176' in jpdse_hip.last_error()
  assert call(F32, F32, 1, 512, 175, 3) == -1 and '176' in jpdse_hip.last_error()
  assert call(F32, F32, 1, 256, 256, 1) == -1 and 'channels' in jpdse_hip.last_error()
  assert call(F32, BF16, 1, 256, 256, 3) == -1 and 'real' in jpdse_hip.last_error()
  # a side whose tile count would exceed the launch grid is refused here too, not by a failed launch after the first kernel
  assert size(1, 16 * 65536 + 10, 176, 3) == 0 and size(1, 16 * 65535 + 10, 176, 3) > 0
  assert call(F32, F32, 1, 16 * 65536 + 10, 176, 3) == -1 and 'tile grid' in jpdse_hip.last_error()
  assert call(F32, F32, 1, 256, 256, 3, nbytes=1024) == -2 and 'workspace' in jpdse_hip.last_error()
  with pytest.raises(jpdse_hip.JpdseError):
    jpdse_hip.check(call(BF16, F32, 2, 100, 100, 3), 'eval_metrics')


# ---- the host half -------------------------------------------------------------------------------------------------------
def _raw(rows):
  return torch.tensor(rows, dtype=torch.float64)


def test_finish_forms_psnr_and_the_product_in_float64():
  from jpdse_hip import ops
  count = 3.0 * 176 * 176
  cs = [0.9, 0.95, 0.97, 0.99, 0.999]
  ss = [0.89, 0.94, 0.96, 0.98, 0.997]
  raw = _raw([[5.0 * count, 40.0 * count, count, 0.0] + cs + ss,
              [0.0, 0.0, count, 0.0] + [1.0] * 10])
  r = ops.eval_metrics_finish(raw)
  per = r['per_image']
  assert set(per) == {'l1', 'mse', 'psnr', 'ms_ssim'}
  assert all(v.dtype == torch.float64 and tuple(v.shape) == (2,) and v.device.type == 'cpu' for v in per.values())
  assert per['l1'].tolist() == [5.0, 0.0] and per['mse'].tolist() == [40.0, 0.0]
  assert per['psnr'][0].item() == 10.0 * math.log10(255.0 ** 2 / 40.0) and per['psnr'][1].item() == math.inf
  want = math.prod(t ** w for t, w in zip(cs[:4] + [ss[4]], ref.WEIGHTS))
  assert abs(per['ms_ssim'][0].item() - want) < 1e-15 and per['ms_ssim'][1].item() == 1.0
  assert abs(per['ms_ssim'][0].item() - ref.combine(cs, ss)) < 1e-15
  assert r['l1'] == 2.5 and r['mse'] == 20.0 and r['psnr'] == math.inf
  assert r['ms_ssim'] == (per['ms_ssim'][0].item() + 1.0) / 2
  assert all(isinstance(r[k], float) for k in ('l1', 'mse', 'psnr', 'ms_ssim'))


def test_finish_clamps_a_non_positive_scale_mean_to_zero():
  from jpdse_hip import ops
  count = 3.0 * 200 * 300
  for bad in (0, 1, 2, 3):
    cs = [0.9] * 5
    cs[bad] = -0.2
    r = ops.eval_metrics_finish(_raw([[1.0, 1.0, count, 0.0] + cs + [0.8] * 5]))
    assert r['ms_ssim'] == 0.0 and r['per_image']['ms_ssim'][0].item() == 0.0
  r = ops.eval_metrics_finish(_raw([[1.0, 1.0, count, 0.0] + [0.9] * 5 + [0.8, 0.8, 0.8, 0.8, 0.0]]))
  assert r['ms_ssim'] == 0.0
  # cs_5 and ssim_1..4 do not enter the product
  r = ops.eval_metrics_finish(_raw([[1.0, 1.0, count, 0.0] + [0.9, 0.9, 0.9, 0.9, -1.0] + [-1.0, -1.0, -1.0, -1.0, 0.8]]))
  assert r['ms_ssim'] > 0 and not math.isnan(r['ms_ssim'])


def test_finish_rounds_l1_and_mse_like_quant_loss():
  """jpdse_quant_loss returns float32(total * (1.0 / count)) over the whole batch: the batch figures must be those bits."""
  from jpdse_hip import ops
  count = 3.0 * 177 * 203
  sums = [(1234567.0, 98765432.0), (7654321.0, 12345678.0), (13.0, 17.0)]
  r = ops.eval_metrics_finish(_raw([[a, b, count, 0.0] + [1.0] * 10 for a, b in sums]))
  inv = 1.0 / (3 * count)
  assert r['l1'] == float(np.float32(sum(a for a, _ in sums) * inv))
  assert r['mse'] == float(np.float32(sum(b for _, b in sums) * inv))


def test_trainer_and_model_expose_get_eval_metrics():
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  from ctu.trainers.pix2pixHD_trainer import Pix2PixHDTrainer
  assert callable(getattr(Pix2PixHDModel, 'get_eval_metrics')) and callable(getattr(Pix2PixHDTrainer, 'get_eval_metrics'))
