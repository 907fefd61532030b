"""GPU tests of the evaluation metrics (jpdse_eval_metrics through ops.eval_metrics, and the public get_eval_metrics).

Yardstick: tests/msssim_ref.py, float64, direct 2-D correlation (no code shared with the kernel).  Tolerance of the
per-scale means cs_j / ssim_j and of ms_ssim: the error of a plain fp32 torch-CPU evaluation of the same definition
(uncentred moments, F.conv2d) against the yardstick on the SAME pair, times a margin of 2 for summation order -- the
"as close to fp64 as torch-fp32, within 2x" rule of the gradient checks -- asserted pair by pair.  Both errors go to the
parity report per shape and pair.
The L1 / squared-error sums are integers and must be exact.

Image pairs (every pair of a tolerance comparison has all five yardstick means > 0, asserted; the clamp is tested by its own
constructed pair): a Cityscapes crop against its JPEG decodes at three qualities (tests/golden/eval_metrics_pairs.npz,
mirror-tiled to the test shape), the synthetic batch's image against its decoded-frame stand-in, identical images, and two
constant images.

Measured figures: DESIGN.md 4.5.  Every run prints both errors per pair and records them in the parity report."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hip_util as hu  # noqa: E402
import msssim_ref as ref  # noqa: E402
from hip_util import DEV  # noqa: E402
from jpdse_hip import F32, BF16, ops  # noqa: E402
from ctu.utils import synthetic  # noqa: E402
from oracle.ctu_cpu import model as omodel  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'eval_metrics_pairs.npz')
MEAN, STD = (0.5, 0.5, 0.5), (1.0, 1.0, 1.0)          # the project's normalisation (ctu.utils.synthetic.default_opt)
MARGIN = 2.0


# ---- image pairs -----------------------------------------------------------------------------------------------------------
def _tile(img_hwc, H, W):
  """[h, w, 3] uint8 -> [3, H, W]: mirror-tiled (no seams) or cropped to the test shape."""
  h, w = img_hwc.shape[:2]
  a = np.pad(img_hwc, ((0, max(H - h, 0)), (0, max(W - w, 0)), (0, 0)), mode='symmetric')[:H, :W]
  return np.ascontiguousarray(np.transpose(a, (2, 0, 1)))


def _normalised(u8):
  """uint8 [..., H, W] -> fp32 normalised values whose quantisation is u8 again (mid-bin, so bf16 rounding may move it)."""
  return ((torch.from_numpy(u8.astype(np.float32)) + 0.5) / 255.0 - 0.5).to(torch.float32)


def _pairs(H, W, kinds):
  """(fake, real) fp32 normalised NCHW tensors [len(kinds), 3, H, W]."""
  z = np.load(GOLDEN)
  fake, real = [], []
  for k in kinds:
    if k.startswith('jpeg_q'):
      f, r = _normalised(_tile(z[k], H, W)), _normalised(_tile(z['original'], H, W))
    elif k == 'synthetic':
      xd = synthetic.synthetic_batch(1, H, W, seed=77)
      f, r = xd['compressed_img'][0], xd['image'][0]
    elif k == 'identical':
      r = hu.bf16_round(_normalised(_tile(z['original'], H, W)))      # the same image under either storage dtype of fake
      f = r.clone()
    elif k == 'constants':
      f = _normalised(np.full((3, H, W), 100, dtype=np.uint8))
      r = _normalised(np.full((3, H, W), 140, dtype=np.uint8))
    elif k == 'anticorrelated':
      b = (np.random.RandomState(4).randint(0, 2, size=(3, H, W)) * 255).astype(np.uint8)
      f, r = _normalised(255 - b), _normalised(b)
    else:
      raise KeyError(k)
    fake.append(f)
    real.append(r)
  return torch.stack(fake).contiguous(), torch.stack(real).contiguous()


def _run(fake, real, dtype):
  """ops.eval_metrics on the pair + the quantised uint8 images the device saw (fake rounded to `dtype` first)."""
  fa = hu.to_act(fake, dtype)
  ra = hu.to_act(real, F32)
  got = ops.eval_metrics(fa, ra, MEAN, STD)
  qf = ref.quantise(hu.quantize_like(fake, dtype).numpy(), MEAN, STD)
  qr = ref.quantise(real.numpy(), MEAN, STD)
  return got, qf, qr, (fa, ra)


# ---- the fp32 torch-CPU evaluation that sets the tolerance --------------------------------------------------------------------
def torch_fp32_ms_ssim(qx, qy):
  """The definition evaluated the plain way in fp32: uncentred E[x^2] - mu^2, F.conv2d with the 2-D window, fp32 means."""
  w = torch.from_numpy(ref.window()).to(torch.float32)[None, None].repeat(3, 1, 1, 1)
  x = torch.from_numpy(qx.astype(np.float32))[None]
  y = torch.from_numpy(qy.astype(np.float32))[None]
  c1, c2 = torch.tensor(ref.C1, dtype=torch.float32), torch.tensor(ref.C2, dtype=torch.float32)
  cs, ss = [], []
  for j in range(5):
    if j:
      x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
    mx, my = F.conv2d(x, w, groups=3), F.conv2d(y, w, groups=3)
    sxx = F.conv2d(x * x, w, groups=3) - mx * mx
    syy = F.conv2d(y * y, w, groups=3) - my * my
    sxy = F.conv2d(x * y, w, groups=3) - mx * my
    m_cs = (2 * sxy + c2) / (sxx + syy + c2)
    m_ss = m_cs * (2 * mx * my + c1) / (mx * mx + my * my + c1)
    cs.append(m_cs.mean().item())
    ss.append(m_ss.mean().item())
  return dict(cs=np.array(cs), ssim=np.array(ss), ms_ssim=ref.combine(cs, ss))


def _err(r, want):
  return max(float(np.abs(np.asarray(r['cs']) - want['cs']).max()), float(np.abs(np.asarray(r['ssim']) - want['ssim']).max()),
             abs(r['ms_ssim'] - want['ms_ssim']))


SMALL = ('jpeg_q10', 'jpeg_q40', 'jpeg_q85', 'synthetic', 'identical', 'constants')
CASES = [
    # name, H, W, pairs of the batch, images checked against the yardstick
    ('176x176', 176, 176, SMALL, range(6)),
    ('177x203', 177, 203, SMALL, range(6)),                      # odd sizes: ragged tiles, odd rows / columns dropped
    ('512x256', 256, 512, SMALL, range(6)),
    ('1024x512 batch 4', 512, 1024, ('jpeg_q10', 'jpeg_q40', 'jpeg_q85', 'synthetic'), (0, 3)),
    ('2048x1024', 1024, 2048, ('jpeg_q40',), (0,)),
]


@pytest.mark.parametrize('dtype', [F32, BF16])
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_kernel_against_the_fp64_yardstick(case, dtype):
  name, H, W, kinds, checked = case
  fake, real = _pairs(H, W, kinds)
  got, qf, qr, acts = _run(fake, real, dtype)
  raw = got['raw']
  assert tuple(raw.shape) == (len(kinds), 14) and raw.dtype == torch.float64
  # integer sums: exact, every image of the batch
  d = qf.astype(np.int64) - qr.astype(np.int64)
  for i in range(len(kinds)):
    assert raw[i, 0].item() == float(np.abs(d[i]).sum()), (name, kinds[i], 'L1 sum')
    assert raw[i, 1].item() == float((d[i] * d[i]).sum()), (name, kinds[i], 'squared-error sum')
    assert raw[i, 2].item() == 3.0 * H * W and raw[i, 3].item() == 0.0
  count = 3.0 * H * W * len(kinds)
  assert got['l1'] == float(np.float32(float(np.abs(d).sum()) * (1.0 / count)))
  assert got['mse'] == float(np.float32(float((d * d).sum()) * (1.0 / count)))
  # per-scale means and ms_ssim
  for i in checked:
    want = ref.ms_ssim(qf[i], qr[i])
    assert min(want['cs'].min(), want['ssim'].min()) > 0, (name, kinds[i], 'pair unfit for a tolerance comparison')
    mine = dict(cs=raw[i, 4:9].numpy(), ssim=raw[i, 9:14].numpy(), ms_ssim=got['per_image']['ms_ssim'][i].item())
    plain = torch_fp32_ms_ssim(qf[i], qr[i])
    ek, et = _err(mine, want), _err(plain, want)
    print('%-18s %-10s %s: kernel %.3e, torch fp32 %.3e (ms_ssim %.9f, yardstick %.9f)'
          % (name, kinds[i], 'bf16' if dtype == BF16 else 'fp32', ek, et, mine['ms_ssim'], want['ms_ssim']))
    # the bound holds pair by pair: each pair against the torch-fp32 error on that very pair
    hu.record('eval_metrics cs_j / ssim_j / ms_ssim vs fp64 yardstick [max abs]: %s, %s' % (name, kinds[i]), ek, MARGIN * et,
              'torch fp32 (uncentred) error %.3e' % et)
    assert ek <= MARGIN * et, '%s %s: kernel error %.3e > %g x torch-fp32 error %.3e' % (name, kinds[i], ek, MARGIN, et)
    if kinds[i] == 'identical':
      assert mine['ms_ssim'] == 1.0 and np.all(mine['cs'] == 1.0) and np.all(mine['ssim'] == 1.0)
      assert raw[i, 0].item() == 0.0 and math.isinf(got['per_image']['psnr'][i].item())
    if kinds[i] == 'constants':
      a, b = float(qf[i].flat[0]), float(qr[i].flat[0])
      assert np.all(qf[i] == a) and np.all(qr[i] == b) and a != b
      closed = (2 * a * b + ref.C1) / (a * a + b * b + ref.C1)
      assert np.all(mine['cs'] == 1.0)                              # centred tiles: variances are exactly 0
      # fp64 throughout: a handful of roundings per position, then < 64 additions on any path of the fixed-order sum
      # (4 per thread, 6 + 2 per block, <= 32 + 8 in the final kernel): worst case 64 x 1.1e-16 = 7e-15 relative
      np.testing.assert_allclose(mine['ssim'], closed, rtol=1e-13)
      assert abs(mine['ms_ssim'] - closed ** ref.WEIGHTS[4]) <= 1e-13
  # determinism: a second call on the same buffers, bit for bit
  again = ops.eval_metrics(acts[0], acts[1], MEAN, STD)
  assert torch.equal(again['raw'], raw)


def test_negative_scale_mean_is_clamped_to_zero():
  fake, real = _pairs(176, 200, ('anticorrelated', 'jpeg_q40'))
  got, qf, qr, _ = _run(fake, real, F32)
  want = ref.ms_ssim(qf[0], qr[0])
  assert want['cs'][0] < 0 and want['ms_ssim'] == 0.0
  assert got['raw'][0, 4].item() < 0
  assert abs(got['raw'][0, 4].item() - want['cs'][0]) < 1e-4
  per = got['per_image']['ms_ssim']
  assert per[0].item() == 0.0 and per[1].item() > 0.9
  assert not math.isnan(got['ms_ssim']) and got['ms_ssim'] == per.mean().item()


def test_small_images_and_other_channel_counts_raise():
  import jpdse_hip
  for h, w, c in ((175, 256, 3), (256, 175, 3), (256, 256, 4)):
    a = ops.Act.empty(1, h, w, c, F32, DEV)
    a.t.zero_()
    with pytest.raises(jpdse_hip.JpdseError):
      ops.eval_metrics(a, a, (0.5,) * c, (1.0,) * c)


# ---- the public call --------------------------------------------------------------------------------------------------------
CODEC = dict(no_feat_encoding=False, no_encoder_binarization=False, feat_num=3, nef=8, n_downsample_E=4,
             encoder_binarizer_out_channels=32)


@pytest.mark.parametrize('mode', ['global fp32', 'global bf16', 'learned codec'])
def test_get_eval_metrics_is_one_forward_of_get_img(mode):
  from ctu.trainers import get_trainer
  import jpdse_hip
  kw = dict(ngf=8, ndf=8, n_blocks_global=1)
  if mode == 'learned codec':
    kw.update(CODEC)
  opt = omodel.default_opt(gpu_ids=[0], print_losses=False, compute_dtype='bf16' if mode.endswith('bf16') else 'fp32', **kw)
  torch.manual_seed(4321)
  tr = get_trainer(opt)(opt, 'train')
  xd = synthetic.synthetic_batch(2, 176, 192, seed=9)
  assert (tr.model.netE is not None) == (mode == 'learned codec')

  # one generator forward per call, and the same conv launches as one get_img (ResnetBlock convs: 128 -> 128, 3x3)
  calls = [0]
  fwd = tr.model.netG.fwd

  def counting(x):
    calls[0] += 1
    return fwd(x)
  tr.model.netG.fwd = counting
  L = jpdse_hip.lib()

  def conv_launches(fn):
    ms, fl, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
    jpdse_hip.check(L.jpdse_prof_select(1, 128, 9 * 128, 64), 'prof_select')
    try:
      out = fn()
      torch.cuda.synchronize()
      jpdse_hip.check(L.jpdse_prof_collect(ctypes.byref(ms), ctypes.byref(fl),
                                           ctypes.byref(n)), 'prof_collect')
    finally:
      L.jpdse_prof_select(0, 0, 0, 0)
    return out, n.value
  img, n_img = conv_launches(lambda: tr.get_img(xd))
  assert calls[0] == 1
  m, n_met = conv_launches(lambda: tr.get_eval_metrics(xd))
  assert calls[0] == 2, 'get_eval_metrics must run the generator once'
  assert n_met == n_img
  tr.model.netG.fwd = fwd

  # equals ops.eval_metrics on get_img's output and the input image
  fake = ops.nchw_to_nhwc(img.contiguous(), F32)
  real = ops.nchw_to_nhwc(xd['image'].to(DEV, torch.float32).contiguous(), F32)
  want = ops.eval_metrics(fake, real, opt.normalize_mean, opt.normalize_std)
  assert torch.equal(m['raw'], want['raw'])
  for k in ('l1', 'mse', 'psnr', 'ms_ssim'):
    assert isinstance(m[k], float) and m[k] == want[k], k
    v = m['per_image'][k]
    assert v.dtype == torch.float64 and v.device.type == 'cpu' and tuple(v.shape) == (2,)
    assert torch.equal(v, want['per_image'][k])
  # PSNR: the float64 formula on the per-image MSE, averaged
  psnr = [10.0 * math.log10(255.0 ** 2 / v) for v in m['per_image']['mse'].tolist()]
  assert m['per_image']['psnr'].tolist() == psnr and m['psnr'] == float(torch.tensor(psnr, dtype=torch.float64).mean())
  assert 0.0 <= m['ms_ssim'] <= 1.0 and m['ms_ssim'] == m['per_image']['ms_ssim'].mean().item()
  # l1 / mse: the bits get_eval_loss returns under either flag
  saved = opt.distortion_loss_fn
  try:
    for flag in ('l1', 'mse'):
      opt.distortion_loss_fn = flag
      assert tr.model.opt.distortion_loss_fn == flag
      assert tr.get_eval_loss(xd) == m[flag], flag
  finally:
    opt.distortion_loss_fn = saved
  # and the quantised images behind them are the ones numpy makes from get_img
  qf = ref.quantise(img.cpu().numpy(), opt.normalize_mean, opt.normalize_std)
  qr = ref.quantise(xd['image'].numpy(), opt.normalize_mean, opt.normalize_std)
  d = qf.astype(np.int64) - qr.astype(np.int64)
  assert m['raw'][:, 0].tolist() == [float(np.abs(d[i]).sum()) for i in range(2)]
  assert m['raw'][:, 1].tolist() == [float((d[i] * d[i]).sum()) for i in range(2)]
