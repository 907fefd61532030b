"""Generate tests/golden/wide_labels_ngf8.npz from the REAL reference (build container only: it needs the reference tree,
imported through oracle._refbridge exactly as scripts/make_golden_zero_flags.py does).

ADE20K's option setter (reference ctu/data/ade20k_dataset.py:26-27) sets num_labels=150, contain_dontcare_label=True with
instance edges on: 151 one-hot lanes + 1 edge lane + 3 image lanes = 155 input channels for G and for D.  No other fixture
runs the reference above 39 input channels, so the torch-CPU oracle (oracle.ctu_cpu.model) was never pinned at this width;
tests/test_wide_labels_host.py pins it to this file, tests/test_hip_wide_labels.py runs the HIP path against both.

Config: batch 2, 32x64, no encoders, G ngf 8 with one ResnetBlock, D ndf 8; torch seed 1234 before the trainer is built.  The
weights regenerate from that seed through oracle.ctu_cpu.nets.init_generator / init_discriminator (checked here tensor by
tensor; the file keeps every tensor's L2 norm, not the 2.5 MB of weights).  The batch does not come from synthetic_batch
(two label cells per image at this size): 4x4-pixel cells with ids from the whole range 0..150, the don't-care id 150 and
id 0 forced in, stored in the file.

Recorded: the inputs, get_img of the batch in eval mode (fp32 [2, 3, 32, 64]), the six losses of one trainer.step captured
from the step's own forward, and that step's gradients of the tensors the tests read: G's and D's first convolutions (the
only weights whose shape depends on the label count) and one deep layer of each.  Data only.

Run:  python scripts/make_golden_wide_labels.py
"""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from oracle import _refbridge  # noqa: E402
from oracle.ctu_cpu import nets, model as omodel  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'wide_labels_ngf8.npz')
SEED, IMG_SEED = 1234, 151
B, H, W = 2, 32, 64
NUM_LABELS = 150                       # + the don't-care label: 151 one-hot lanes
CELL = 4
GRAD_KEYS_G = ('model.1.weight', 'model.10.weight')
GRAD_KEYS_D = ('scale0_layer0.0.weight', 'scale1_layer0.0.weight', 'scale0_layer2.0.weight')


def wide_opt(**over):
  return omodel.default_opt(ngf=8, ndf=8, n_blocks_global=1, num_labels=NUM_LABELS, contain_dontcare_label=True,
                            netE_groups=1, inst_wise_pool=False, label_encoder_out_channels=36, save_dir='/nonexistent',
                            **over)


def wide_batch(seed=IMG_SEED):
  """Label / instance maps on 4x4-pixel cells (ids 0..150, both ends present), uniform image in [-0.5, 0.5)."""
  g = torch.Generator().manual_seed(seed)
  ch, cw = H // CELL, W // CELL
  lab = torch.randint(0, NUM_LABELS + 1, (B, 1, ch, cw), generator=g)
  lab[0, 0, 0, 0], lab[1, 0, ch - 1, cw - 1], lab[0, 0, 1, 2], lab[1, 0, 3, 5] = NUM_LABELS, NUM_LABELS, 0, 0
  inst = torch.randint(0, 40, (B, 1, ch // 2, cw // 2), generator=g).repeat_interleave(2, 2).repeat_interleave(2, 3) * 1000 + lab
  up = lambda t: t.repeat_interleave(CELL, 2).repeat_interleave(CELL, 3)
  image = torch.rand(B, 3, H, W, generator=g) - 0.5
  return {'label': up(lab).float(), 'instance': up(inst).long(), 'image': image, 'compressed_img': image.clone(),
          'path': ['wide_%d' % i for i in range(B)]}


def _clone(xd):
  return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in xd.items()}


def main():
  torch.set_num_threads(8)
  torch.use_deterministic_algorithms(True)
  networks, RefModel, RefTrainer = _refbridge.import_reference(nets.init_vgg19())
  opt = wide_opt()
  nc = omodel.semantics_nc(opt)
  assert nc == 152
  torch.manual_seed(SEED)
  sd_G = nets.init_generator(omodel.gen_cfg(opt), nc + 3, 3)
  sd_D = nets.init_discriminator(nc + 3, 8, 3, 2)
  xd = wide_batch()
  assert int(xd['label'].max()) == NUM_LABELS and int(xd['label'].min()) == 0
  torch.manual_seed(SEED)
  tr = RefTrainer(copy.deepcopy(opt), 'train')
  for k, v in tr.model.netG.state_dict().items():
    assert torch.equal(v, sd_G[k]), k
  for k, v in tr.model.netD.state_dict().items():
    assert torch.equal(v, sd_D[k]), k
  assert tuple(sd_G['model.1.weight'].shape) == (8, 155, 7, 7) and tuple(sd_D['scale0_layer0.0.weight'].shape) == (8, 155, 4, 4)
  rec = dict(seed=np.int64(SEED), batch=np.int64(B), height=np.int64(H), width=np.int64(W), num_labels=np.int64(NUM_LABELS),
             label=xd['label'].numpy().astype(np.uint8), instance=xd['instance'].numpy().astype(np.int32),
             image=xd['image'].numpy().astype(np.float32),
             Gkeys=np.array(list(sd_G.keys())), Dkeys=np.array(list(sd_D.keys())),
             Gnorm=np.array([float(v.double().norm()) for v in sd_G.values()]),
             Dnorm=np.array([float(v.double().norm()) for v in sd_D.values()]))
  with torch.no_grad():
    img = tr.get_img(_clone(xd))
  assert tuple(img.shape) == (B, 3, H, W)
  rec['get_img'] = img.detach().cpu().numpy().astype(np.float32)
  captured = {}
  orig = tr._get_train_loss

  def capture(x_dict):
    L = orig(x_dict)
    captured['losses'] = [float(v.detach()) for v in L]
    return L
  tr._get_train_loss = capture
  tr.step(_clone(xd))
  rec['losses'] = np.array(captured['losses'], dtype=np.float64)
  rec['loss_names'] = np.array(list(tr.model.loss_names))
  # pix2pixHD_trainer.py:64-78: after step() every parameter still holds the gradient its optimizer consumed
  pG, pD = dict(tr.model.netG.named_parameters()), dict(tr.model.netD.named_parameters())
  for k in GRAD_KEYS_G:
    rec['gradG:' + k] = pG[k].grad.detach().numpy().astype(np.float32)
  for k in GRAD_KEYS_D:
    rec['gradD:' + k] = pD[k].grad.detach().numpy().astype(np.float32)
  print('losses %s' % ' '.join('%.6f' % v for v in captured['losses']))
  np.savez_compressed(OUT, **rec)
  print('%s: %.1f KB' % (OUT, os.path.getsize(OUT) / 1024.0))


if __name__ == '__main__':
  main()
