"""Writes tests/golden/semantics_cityscapes.npz: ONE real label / instance map pair, the data the coder of DESIGN.md 4.9 is
checked and measured on.  Reads one Cityscapes gtFine pair (`*_gtFine_labelIds.png`, `*_gtFine_instanceIds.png`) with PIL and
brings it to the loader's size by nearest neighbour, as the dataset does for label and instance maps (scale to the load
width, Image.NEAREST, no normalisation).  The file holds two integer arrays and nothing else:

  label     uint8 [H, W]   class ids
  instance  int32 [H, W]   Cityscapes instance ids (class id, or class id * 1000 + k for the things classes)

The recorded file was made from the pair gtFine/val/frankfurt/frankfurt_000000_005898 (the stem oracle/make_golden.py also
uses) at the default width of 1024: 1024 x 512, 20 classes, 28 instance ids.

  python scripts/make_golden_semantics.py --label PATH_labelIds.png --instance PATH_instanceIds.png [--width 1024]
"""
import argparse
import os

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(path, width):
  img = Image.open(path)
  w, h = img.size
  return np.array(img.resize((width, int(round(width * h / w))), Image.NEAREST))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--label', required=True)
  ap.add_argument('--instance', required=True)
  ap.add_argument('--width', type=int, default=1024)
  ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'semantics_cityscapes.npz'))
  args = ap.parse_args()
  label, inst = load(args.label, args.width), load(args.instance, args.width)
  if label.shape != inst.shape or label.ndim != 2:
    raise SystemExit('label %s and instance %s maps do not match' % (label.shape, inst.shape))
  if label.max() > 255 or inst.min() < 0 or inst.max() >= 1 << 31:
    raise SystemExit('values outside the planes of the format')
  np.savez_compressed(args.out, label=label.astype(np.uint8), instance=inst.astype(np.int32))
  print('%s: %d x %d, %d classes, %d instance ids, %d bytes' % (args.out, label.shape[1], label.shape[0],
                                                             len(np.unique(label)), len(np.unique(inst)),
                                                             os.path.getsize(args.out)))


if __name__ == '__main__':
  main()
