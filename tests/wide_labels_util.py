"""What tests/test_wide_labels_host.py and tests/test_hip_wide_labels.py share: the ADE20K-width configuration (150 labels
+ don't-care + instance edge: 152 semantic lanes, 155 input channels) and the batch / weights of
tests/golden/wide_labels_ngf8.npz (scripts/make_golden_wide_labels.py, recorded from the reference)."""
import os

import numpy as np
import torch

from oracle.ctu_cpu import model as omodel, nets

NUM_LABELS = 150
N_ONEHOT, LABEL_NC, INPUT_NC = 151, 152, 155
WIDE = dict(num_labels=NUM_LABELS, contain_dontcare_label=True)
NET = dict(ngf=8, ndf=8, n_blocks_global=1, **WIDE)


def load_gold(golden_dir):
  z = np.load(os.path.join(golden_dir, 'wide_labels_ngf8.npz'))
  return {k: z[k] for k in z.files}


def batch(gold):
  """The recorded inputs as an x_dict (fresh tensors on every call)."""
  image = torch.from_numpy(gold['image'].copy())
  return {'label': torch.from_numpy(gold['label'].astype(np.float32)), 'instance': torch.from_numpy(gold['instance'].astype(np.int64)),
          'image': image, 'compressed_img': image.clone(), 'path': ['wide_%d' % i for i in range(image.shape[0])]}


def weights(seed, **net):
  """The seeded weights of the fixture (or of another generator configuration at the same input width)."""
  opt = omodel.default_opt(**dict(NET, **net))
  torch.manual_seed(seed)
  sd_G = nets.init_generator(omodel.gen_cfg(opt), INPUT_NC, 3)
  sd_D = nets.init_discriminator(INPUT_NC, opt.ndf, opt.n_layers_D, opt.num_D)
  return sd_G, sd_D


def wide_batch(n, height, width, seed, cell=4):
  """A seeded batch at any size: label ids over the whole range 0..150 on `cell`-pixel squares, the don't-care id 150 and
  id 0 forced in; instance ids on 2x2 groups of cells."""
  g = torch.Generator().manual_seed(seed)
  ch, cw = -(-height // cell), -(-width // cell)
  lab = torch.randint(0, NUM_LABELS + 1, (n, 1, ch, cw), generator=g)
  lab[0, 0, 0, 0], lab[-1, 0, -1, -1], lab[0, 0, -1, 0] = NUM_LABELS, NUM_LABELS, 0
  inst = torch.randint(0, 40, (n, 1, -(-ch // 2), -(-cw // 2)), generator=g).repeat_interleave(2, 2).repeat_interleave(2, 3)
  inst = inst[:, :, :ch, :cw] * 1000 + lab
  up = lambda t: t.repeat_interleave(cell, 2).repeat_interleave(cell, 3)[:, :, :height, :width].contiguous()
  image = torch.rand(n, 3, height, width, generator=g) - 0.5
  comp = (image + 0.05 * torch.randn(n, 3, height, width, generator=g)).clamp_(-0.5, 0.5)
  return {'label': up(lab).float(), 'instance': up(inst).long(), 'image': image, 'compressed_img': comp,
          'path': ['wide_%d' % i for i in range(n)]}


def clone(xd):
  return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in xd.items()}


class ZeroSemOracle(omodel.OracleTrainer):
  """--zero_sem (reference pix2pixHD_model.py:585-587): the generator sees zeros in every semantic lane; _get_img returns the
  untouched input_label, so the discriminator and every loss keep the real semantics."""

  def generate(self, input_label, src):
    return super(ZeroSemOracle, self).generate(torch.zeros_like(input_label), src)
