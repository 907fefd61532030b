"""Generate tests/golden/eval_metrics_pairs.npz: one natural crop and its JPEG decodes at three qualities, the image pairs
the MS-SSIM tests of jpdse_eval_metrics run on.  Needs the reference tree: the crop is cut from one image of its bundled
Cityscapes fixture, found through oracle._refbridge.REFERENCE_ROOT.  Data only: four uint8 arrays [176, 208, 3].

  original            the crop (rows 300.., columns 400.. of the first leftImg8bit frame in sorted order)
  jpeg_q10/_q40/_q85  Pillow's JPEG round trip of it (quality 10 / 40 / 85, default 4:2:0 subsampling)

The script also prints the float64 yardstick (tests/msssim_ref.py) of every pair: the test's tolerance comparison needs all
five per-scale means > 0, which is checked here, on the CPU, when the pairs are chosen (the test asserts it again per shape).

Run:  python scripts/make_golden_eval_metrics.py
"""
import glob
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
  if p not in sys.path:
    sys.path.insert(0, p)

from oracle import _refbridge  # noqa: E402
import msssim_ref  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'eval_metrics_pairs.npz')
CROP_H, CROP_W, ROW0, COL0 = 176, 208, 300, 400
QUALITIES = (10, 40, 85)


def main():
  frames = sorted(glob.glob(os.path.join(_refbridge.REFERENCE_ROOT, 'datasets', '*', 'leftImg8bit', '*', '*', '*.png')))
  if not frames:
    raise SystemExit('no leftImg8bit frame under the reference tree')
  img = np.asarray(Image.open(frames[0]).convert('RGB'))
  crop = np.ascontiguousarray(img[ROW0:ROW0 + CROP_H, COL0:COL0 + CROP_W])
  assert crop.shape == (CROP_H, CROP_W, 3), crop.shape
  out = {'original': crop}
  for q in QUALITIES:
    buf = io.BytesIO()
    Image.fromarray(crop).save(buf, format='JPEG', quality=q)
    out['jpeg_q%d' % q] = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert('RGB'))
  np.savez_compressed(OUT, **out)
  print('wrote %s (%d bytes) from %s' % (OUT, os.path.getsize(OUT), os.path.basename(frames[0])))
  for q in QUALITIES:
    r = msssim_ref.ms_ssim(crop, out['jpeg_q%d' % q])
    assert min(r['cs'].min(), r['ssim'].min()) > 0
    print('q%-3d ms_ssim %.6f  cs %s  ssim %s' % (q, r['ms_ssim'], np.round(r['cs'], 5), np.round(r['ssim'], 5)))


if __name__ == '__main__':
  main()
