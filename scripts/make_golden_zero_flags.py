"""Generate tests/golden/zero_flags_ngf8.npz from the REAL reference (build container only: it needs the reference tree,
imported through oracle._refbridge exactly as scripts/make_golden_learned_codec.py does).

The ablation inputs --zero_vis, --zero_ins and --zero_sem (reference pix2pixHD_model.py:583-606) blank the visual lanes, the
instance-edge lane or every semantic lane of the generator input.  --zero_sem has no equivalent among the torch-CPU oracle's
inputs (the discriminator keeps the real semantics while the generator sees none), so tests/test_hip_zero_flags.py pins all
three to what the reference itself computes.

Config: batch 2, 64x128, no encoders, G ngf 8 with one ResnetBlock, D ndf 8; torch seed 1234 before each trainer is built, so
the three trainers start from the same weights, which regenerate from that seed through oracle.ctu_cpu.nets.init_generator /
init_discriminator (checked here tensor by tensor, not stored).  The batch regenerates from its seed
(oracle.ctu_cpu.model.synthetic_batch).

Recorded per flag: get_img of the batch in eval mode (fp32 [2, 3, 64, 128]) and the six losses of one trainer.step, captured
from the step's own forward.  Data only.

Run:  python scripts/make_golden_zero_flags.py
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

OUT = os.path.join(ROOT, 'tests', 'golden', 'zero_flags_ngf8.npz')
SEED, IMG_SEED = 1234, 83
B, H, W = 2, 64, 128
FLAGS = ('zero_vis', 'zero_ins', 'zero_sem')


def flag_opt(**over):
  return omodel.default_opt(ngf=8, ndf=8, n_blocks_global=1, netE_groups=1, inst_wise_pool=False,
                            label_encoder_out_channels=36, save_dir='/nonexistent', **over)


def _clone(xd):
  return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in xd.items()}


def main():
  torch.set_num_threads(8)
  torch.use_deterministic_algorithms(True)
  networks, RefModel, RefTrainer = _refbridge.import_reference(nets.init_vgg19())
  torch.manual_seed(SEED)
  sd_G = nets.init_generator(omodel.gen_cfg(flag_opt()), 36 + 3, 3)
  sd_D = nets.init_discriminator(36 + 3, 8, 3, 2)
  rec = dict(seed=np.int64(SEED), img_seed=np.int64(IMG_SEED), batch=np.int64(B), height=np.int64(H), width=np.int64(W),
             flags=np.array(FLAGS))
  xd = omodel.synthetic_batch(B, H, W, seed=IMG_SEED)
  for flag in FLAGS:
    torch.manual_seed(SEED)
    tr = RefTrainer(copy.deepcopy(flag_opt(**{flag: True})), 'train')
    for k, v in tr.model.netG.state_dict().items():
      assert torch.equal(v, sd_G[k]), k
    for k, v in tr.model.netD.state_dict().items():
      assert torch.equal(v, sd_D[k]), k
    with torch.no_grad():
      img = tr.get_img(_clone(xd))
    assert tuple(img.shape) == (B, 3, H, W)
    rec['img:' + flag] = img.detach().cpu().numpy().astype(np.float32)
    captured = {}
    orig = tr._get_train_loss

    def capture(x_dict, orig=orig, captured=captured):
      L = orig(x_dict)
      captured['losses'] = [float(v.detach()) for v in L]
      return L
    tr._get_train_loss = capture
    tr.step(_clone(xd))
    rec['losses:' + flag] = np.array(captured['losses'], dtype=np.float64)
    rec['loss_names'] = np.array(list(tr.model.loss_names))
    print('%-8s losses %s' % (flag, ' '.join('%.6f' % v for v in captured['losses'])))
  np.savez_compressed(OUT, **rec)
  print('%s: %.1f KB' % (OUT, os.path.getsize(OUT) / 1024.0))


if __name__ == '__main__':
  main()
