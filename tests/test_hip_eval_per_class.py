"""GPU tests of the per-class distortion (jpdse_eval_metrics_sem through ops.eval_metrics(..., label, n_classes), and the
public get_eval_metrics(x, per_class=True)).

Everything the kernel adds is an integer, so the yardstick (tests/class_metrics_ref.py: np.bincount over the images numpy
quantises with tensor2im's arithmetic) is met EXACTLY: no tolerance on anything the device wrote (only the host's log10 is compared to a few ulp).  Shapes: N = 2 at 176x176 (the
smallest the MS-SSIM half accepts: 31 blocks of 1024 pixels, the last one ragged) and 177x203 (odd width, rows that straddle
waves and blocks), both storage dtypes of the reconstruction; one 1024x512 image for the counters that pass 2^32."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import class_metrics_ref as cref  # noqa: E402
import hip_util as hu  # noqa: E402
import msssim_ref as ref  # noqa: E402
from hip_util import DEV  # noqa: E402
from jpdse_hip import F32, BF16, ops  # noqa: E402
from ctu.utils import synthetic  # noqa: E402
from oracle.ctu_cpu import model as omodel  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MEAN, STD = (0.5, 0.5, 0.5), (1.0, 1.0, 1.0)
SHAPES = [(176, 176), (177, 203)]
DTYPES = [F32, BF16]


def _mirror_tile(a, H, W):
  """[h, w, ...] -> [H, W, ...], mirror-tiled (no seams) or cropped."""
  h, w = a.shape[:2]
  pad = ((0, max(H - h, 0)), (0, max(W - w, 0))) + ((0, 0),) * (a.ndim - 2)
  return np.ascontiguousarray(np.pad(a, pad, mode='symmetric')[:H, :W])


_IMAGES = {}


def _images(H, W):
  """(fake, real) fp32 normalised NCHW [2, 3, H, W], made once per shape and never modified: image 0 is a Cityscapes crop
  against its JPEG decode at quality 10, image 1 the synthetic pair."""
  if (H, W) not in _IMAGES:
    z = np.load(os.path.join(GOLDEN, 'eval_metrics_pairs.npz'))
    norm = lambda u8: (torch.from_numpy(np.transpose(_mirror_tile(u8, H, W), (2, 0, 1)).astype(np.float32)) + 0.5) / 255.0 - 0.5
    xd = synthetic.synthetic_batch(1, H, W, seed=77)
    fake = torch.stack([norm(z['jpeg_q10']), xd['compressed_img'][0]]).contiguous()
    real = torch.stack([norm(z['original']), xd['image'][0]]).contiguous()
    _IMAGES[(H, W)] = (fake, real)
  return _IMAGES[(H, W)]


def _labels(kind, H, W):
  """(label fp32 [2, 1, H, W], n_classes)."""
  rng = np.random.RandomState(len(kind) * 1000 + H + W)
  if kind == 'cityscapes crop':
    lab = np.load(os.path.join(GOLDEN, 'preprocess_cityscapes_crop.npz'))['label']       # [64, 128] uint8, ids 4..27
    a = _mirror_tile(lab, H, W)
    both, n = np.stack([a, a[::-1, ::-1]]), 35
  elif kind == 'random 35':
    both, n = rng.randint(0, 35, size=(2, H, W)), 35
  elif kind == 'one class':
    both, n = np.stack([np.zeros((H, W), dtype=np.int64), rng.randint(0, 2, size=(H, W))]), 1    # image 1: half strays
  elif kind == '256 classes':
    both, n = rng.choice([0, 7, 128, 255], size=(2, H, W), p=[0.4, 0.3, 0.2, 0.1]), 256
  else:
    raise KeyError(kind)
  return torch.from_numpy(np.ascontiguousarray(both).astype(np.float32))[:, None].contiguous(), n


def _call(fake, real, label, n_classes, dtype):
  """ops.eval_metrics with the label map + the yardstick's table for the images the device saw."""
  fa, ra = hu.to_act(fake, dtype), hu.to_act(real, F32)
  lab = label.to(DEV).contiguous()
  got = ops.eval_metrics(fa, ra, MEAN, STD, lab, n_classes)
  qf = ref.quantise(hu.quantize_like(fake, dtype).numpy(), MEAN, STD)
  qr = ref.quantise(real.numpy(), MEAN, STD)
  want = cref.table(qf, qr, label.numpy(), n_classes)
  return got, want, (fa, ra, lab)


def _conserved(got, H, W):
  cls = got['per_class']['raw']
  assert cls.dtype == torch.int64 and cls.device.type == 'cpu'
  tot = cls.sum(dim=1)
  assert tot[:, 0].tolist() == got['raw'][:, 0].tolist(), 'the |d| rows do not add up to out[0]'
  assert tot[:, 1].tolist() == got['raw'][:, 1].tolist(), 'the d^2 rows do not add up to out[1]'
  assert tot[:, 2].tolist() == [H * W] * cls.shape[0], 'pixels dropped or counted twice'


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('shape', SHAPES, ids=['176x176', '177x203'])
@pytest.mark.parametrize('kind', ['cityscapes crop', 'random 35', 'one class', '256 classes'])
def test_class_table_equals_the_numpy_integers(kind, shape, dtype):
  H, W = shape
  fake, real = _images(H, W)
  label, n = _labels(kind, H, W)
  got, want, acts = _call(fake, real, label, n, dtype)
  cls = got['per_class']['raw']
  assert tuple(cls.shape) == (2, n + 1, 3)
  assert np.array_equal(cls.numpy(), want)
  if kind == '256 classes':
    assert (want[:, :, 2] == 0).sum() >= 2 * 252          # most classes absent
  if kind == 'one class':
    assert want[0, 1, 2] == 0 and want[1, 1, 2] > H * W // 4
  # conservation, and `out` is what the plain call writes for the same buffers, bit for bit
  _conserved(got, H, W)
  plain = ops.eval_metrics(acts[0], acts[1], MEAN, STD)
  assert torch.equal(plain['raw'], got['raw'])
  for k in ('l1', 'mse', 'psnr', 'ms_ssim'):
    assert plain[k] == got[k] and torch.equal(plain['per_image'][k], got['per_image'][k])
  assert 'per_class' not in plain
  # determinism: a second call on the same buffers
  again = ops.eval_metrics(acts[0], acts[1], MEAN, STD, acts[2], n)
  assert torch.equal(again['per_class']['raw'], cls) and torch.equal(again['raw'], got['raw'])


def test_one_class_over_a_whole_large_image_passes_2_to_32():
  """1 x 1024 x 512, every pixel of class 7, fake quantises to 0 and real to 255 everywhere: all 64 lanes of every wave meet
  in one class, and the squared sum 65025 * 3 * 524288 = 1.02e11 needs more than 32 bits (a block alone sums 2.0e8 of it)."""
  H, W = 1024, 512
  fake = torch.full((1, 3, H, W), -0.5)
  real = torch.full((1, 3, H, W), 0.5)
  label = torch.full((1, 1, H, W), 7.0)
  for dtype in DTYPES:
    got, want, _ = _call(fake, real, label, 35, dtype)
    cls = got['per_class']['raw']
    assert cls[0, 7].tolist() == [255 * 3 * H * W, 65025 * 3 * H * W, H * W]
    assert 65025 * 3 * H * W > 2 ** 32
    assert np.array_equal(cls.numpy(), want) and int(cls.sum()) == int(cls[0, 7].sum())
    _conserved(got, H, W)
    r = got['per_class']
    assert r['l1'][7].item() == 255.0 and r['mse'][7].item() == 65025.0 and r['psnr'][7].item() == 0.0
    assert r['pixels'].sum().item() == H * W and r['unlabelled'] == 0


@pytest.mark.parametrize('shape', SHAPES, ids=['176x176', '177x203'])
def test_stray_labels_land_in_the_extra_row_once(shape):
  H, W = shape
  fake, real = _images(H, W)
  n = 35
  label, _ = _labels('random 35', H, W)
  label = label.clone()
  strays = [(-1.0, (0, 0, 0)), (float(n), (0, H - 1, W - 1)), (255.0, (0, 5, 64)), (3.5, (1, 100, 63)),
            (-0.5, (1, H - 1, 0)), (1e9, (1, 0, W - 1)), (float('nan'), (1, 88, 129))]
  for v, (i, y, x) in strays:
    label[i, 0, y, x] = v
  got, want, _ = _call(fake, real, label, n, F32)
  cls = got['per_class']['raw'].numpy()
  assert np.array_equal(cls, want)
  assert cls[0, n, 2] == 3 and cls[1, n, 2] == 4 and got['per_class']['unlabelled'] == 7
  # they appear in no class: the classes hold exactly the other pixels
  assert cls[:, :n, 2].sum(axis=1).tolist() == [H * W - 3, H * W - 4]
  _conserved(got, H, W)


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_images_do_not_mix(dtype):
  """The same class ids in both images: a 2-image call equals two 1-image calls, image for image."""
  H, W = 177, 203
  fake, real = _images(H, W)
  label, n = _labels('cityscapes crop', H, W)
  got, _, (fa, ra, lab) = _call(fake, real, label, n, dtype)
  for i in range(2):
    one = ops.eval_metrics(fa.batch_slice(i, i + 1), ra.batch_slice(i, i + 1), MEAN, STD, lab[i:i + 1].contiguous(), n)
    assert torch.equal(one['per_class']['raw'][0], got['per_class']['raw'][i])
    assert torch.equal(one['raw'][0], got['raw'][i])
  shared = (got['per_class']['raw'][0, :n, 2] > 0) & (got['per_class']['raw'][1, :n, 2] > 0)
  assert shared.sum().item() >= 5


def test_host_dict_absent_exact_and_pixel_weighted_classes():
  """Class 0: a small area of image 0 and most of image 1, with different errors (the mean of per-image means would differ
  from the pixel-weighted figure); class 1: reconstructed exactly; class 2: absent; class 3: the rest of image 0."""
  H, W = 176, 176
  fake, real = _images(H, W)
  fake, real = fake.clone(), real.clone()
  lab = np.zeros((2, H, W), dtype=np.float32)
  lab[0, :, :] = 3
  lab[0, :16, :40] = 0
  lab[0, 100:, 90:] = 1
  lab[1, 170:, :] = 1
  label = torch.from_numpy(lab)[:, None].contiguous()
  exact = (label == 1).expand(-1, 3, -1, -1)
  fake[exact] = real[exact]
  got, want, _ = _call(fake, real, label, 4, F32)
  assert np.array_equal(got['per_class']['raw'].numpy(), want)
  r, w = got['per_class'], cref.per_class(want)
  assert r['pixels'].tolist() == w['pixels'].tolist() == [16 * 40 + 170 * W, 76 * 86 + 6 * W, 0, H * W - 16 * 40 - 76 * 86]
  for k in ('l1', 'mse'):
    assert np.array_equal(r[k].numpy(), w[k]) and np.array_equal(r['per_image'][k].numpy(), w['per_image'][k])
    assert r[k][1].item() == 0.0 and r[k][2].item() == 0.0 and r[k][0].item() > 0.0
  assert np.allclose(r['psnr'].numpy(), w['psnr'], rtol=1e-14, atol=0, equal_nan=True)   # log10 of two libms: a few ulp
  assert r['psnr'][1].item() == float('inf') and np.isnan(r['psnr'][2].item()) and np.isfinite(r['psnr'][0].item())
  assert np.isnan(r['per_image']['psnr'][1, 3].item()) and r['per_image']['l1'][1, 3].item() == 0.0
  # pixel-weighted over the batch, not the mean of the two per-image figures
  per = r['per_image']['l1'][:, 0]
  tab = got['per_class']['raw']
  assert r['l1'][0].item() == (tab[0, 0, 0] + tab[1, 0, 0]).item() / (3.0 * (tab[0, 0, 2] + tab[1, 0, 2]).item())
  assert abs(r['l1'][0].item() - per.mean().item()) > 1e-3 * r['l1'][0].item()


def test_get_eval_metrics_per_class_on_the_trainer():
  from ctu.trainers import get_trainer
  opt = omodel.default_opt(gpu_ids=[0], print_losses=False, ngf=8, ndf=8, n_blocks_global=1)
  torch.manual_seed(4321)
  tr = get_trainer(opt)(opt, 'train')
  xd = synthetic.synthetic_batch(2, 176, 192, seed=9)
  plain = tr.get_eval_metrics(xd)
  m = tr.get_eval_metrics(xd, per_class=True)
  assert 'per_class' not in plain and set(m) == set(plain) | {'per_class'}
  assert torch.equal(m['raw'], plain['raw'])
  for k in ('l1', 'mse', 'psnr', 'ms_ssim'):
    assert m[k] == plain[k] and torch.equal(m['per_image'][k], plain['per_image'][k])
  # the yardstick on get_img's output
  img = tr.get_img(xd)
  qf = ref.quantise(img.cpu().numpy(), opt.normalize_mean, opt.normalize_std)
  qr = ref.quantise(xd['image'].numpy(), opt.normalize_mean, opt.normalize_std)
  n = tr.model.n_onehot
  assert n == 35
  want = cref.table(qf, qr, xd['label'].numpy(), n)
  r, w = m['per_class'], cref.per_class(want)
  assert np.array_equal(r['raw'].numpy(), want)
  assert r['unlabelled'] == 0 and r['pixels'].sum().item() == 2 * 176 * 192
  for k in ('pixels', 'l1', 'mse'):
    assert tuple(r[k].shape) == (n,) and tuple(r['per_image'][k].shape) == (2, n)
    assert np.array_equal(r[k].numpy(), w[k]) and np.array_equal(r['per_image'][k].numpy(), w['per_image'][k])
  assert np.allclose(r['psnr'].numpy(), w['psnr'], rtol=1e-14, atol=0, equal_nan=True)   # log10 of two libms: a few ulp
  _conserved(m, 176, 192)
