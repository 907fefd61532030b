"""GPU: the ablation inputs --zero_vis, --zero_ins and --zero_sem (reference pix2pixHD_model.py:583-606) at ngf 8 / ndf 8,
64x128, fp32, with the tolerances of tests/test_hip_learned_codec.py.

Two of the three have an exact equivalent among the inputs of the torch-CPU oracle (oracle.ctu_cpu.model.OracleTrainer):

  --zero_vis  reference :583-584 replaces feat_map -- the image itself without encoders (:566-567) -- by zeros before the
              concat (:595); every loss still compares with x_dict['real_image'] (:711, :722, :756, :767).  The oracle run with
              use_compressed and an all-zero `compressed_img` feeds exactly that: only G's input is the "decoded frame"
              (:517-518), here zeros.
  --zero_ins  reference :591 zeroes the last channel of input_label in place, and _get_img returns that tensor (:610) to
              get_train_loss, which hands it to the discriminator (:717-733): G and D both see a zero edge lane.  The oracle
              run with a constant instance map computes an all-zero edge lane (get_edges, :774-783) for both.
  --zero_sem  G sees zeros in all label_nc semantic lanes (:587) while _get_img returns the untouched input_label, so D keeps
              the real semantics.  No oracle input does that: pinned to tests/golden/zero_flags_ngf8.npz, recorded from the
              reference by scripts/make_golden_zero_flags.py -- which holds all three flags, so the two equivalences above
              are themselves checked against the reference here."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'jpd-se_amd'), os.path.dirname(os.path.abspath(__file__))):
  if _p not in sys.path:
    sys.path.insert(0, _p)

from oracle.ctu_cpu import model as omodel, nets  # noqa: E402

NET_TOL = 2e-4        # fp32 network outputs, max-abs relative to the output's max
LOSS_TOL = 1e-3
NET = dict(ngf=8, ndf=8, n_blocks_global=1)


@pytest.fixture(scope='module')
def gold(golden_dir):
  z = np.load(os.path.join(golden_dir, 'zero_flags_ngf8.npz'))
  return {k: z[k] for k in z.files}


def _weights(seed):
  torch.manual_seed(seed)
  sd_G = nets.init_generator(omodel.gen_cfg(omodel.default_opt(**NET)), 36 + 3, 3)
  sd_D = nets.init_discriminator(36 + 3, 8, 3, 2)
  return sd_G, sd_D


def _trainer(sd_G, sd_D, **flags):
  from ctu.trainers import get_trainer
  opt = omodel.default_opt(gpu_ids=[0], print_losses=False, **dict(NET, **flags))
  tr = get_trainer(opt)(opt, 'train')
  tr.model.netG.load_state_dict(sd_G)
  tr.model.netD.load_state_dict(sd_D)
  return tr


def _clone(xd):
  return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in xd.items()}


def _img_close(got, want, what):
  got, want = got.detach().cpu().double(), want.detach().cpu().double()
  err, scale = (got - want).abs().max().item(), want.abs().max().item()
  print('%s: get_img max abs error %.3e, bound %.3e' % (what, err, NET_TOL * scale))
  assert err <= NET_TOL * scale, '%s: get_img differs by %.3e (bound %.3e)' % (what, err, NET_TOL * scale)


def _losses_close(got, want, what):
  for k in omodel.LOSS_NAMES:
    print('%s: loss %s %.6f vs %.6f' % (what, k, got[k], want[k]))
    assert abs(got[k] - want[k]) <= LOSS_TOL * max(1.0, abs(want[k])), '%s: loss %s %.6f vs %.6f' % (what, k, got[k], want[k])


def _against_oracle(flag, oracle_opt_over, oracle_batch):
  sd_G, sd_D = _weights(1234)
  tr = _trainer(sd_G, sd_D, **{flag: True})
  ora = omodel.OracleTrainer(omodel.default_opt(**dict(NET, **oracle_opt_over)), sd_G=sd_G, sd_D=sd_D)
  xd = omodel.synthetic_batch(2, 64, 128, seed=57)
  xo = oracle_batch(_clone(xd))
  _img_close(tr.get_img(_clone(xd)), ora.get_img(xo), '--' + flag)
  tr.step(_clone(xd))
  ora.step(xo)
  torch.cuda.synchronize()
  _losses_close(tr.last_losses, ora.last_losses, '--' + flag + ' step')
  return tr, xd


def test_zero_vis_equals_the_oracle_fed_an_all_zero_decoded_frame():
  def blank(xd):
    xd['compressed_img'] = torch.zeros_like(xd['image'])
    return xd
  tr, xd = _against_oracle('zero_vis', dict(use_compressed=True), blank)
  # and it is not the unablated run
  plain = _trainer(*_weights(1234))
  assert (plain.get_img(_clone(xd)) - _trainer(*_weights(1234), zero_vis=True).get_img(_clone(xd))).abs().max().item() > 1e-2


def test_zero_ins_equals_the_oracle_fed_a_constant_instance_map():
  def constant(xd):
    xd['instance'] = torch.zeros_like(xd['instance'])
    return xd
  _against_oracle('zero_ins', dict(), constant)


@pytest.mark.parametrize('flag', ['zero_vis', 'zero_ins', 'zero_sem'])
def test_zero_flags_equal_the_reference_golden(gold, flag):
  assert [str(f) for f in gold['flags']] == ['zero_vis', 'zero_ins', 'zero_sem']
  assert tuple(str(n) for n in gold['loss_names']) == omodel.LOSS_NAMES
  sd_G, sd_D = _weights(int(gold['seed']))
  tr = _trainer(sd_G, sd_D, **{flag: True})
  xd = omodel.synthetic_batch(int(gold['batch']), int(gold['height']), int(gold['width']), seed=int(gold['img_seed']))
  _img_close(tr.get_img(_clone(xd)), torch.from_numpy(gold['img:' + flag]), 'reference --' + flag)
  tr.step(_clone(xd))
  want = dict(zip(omodel.LOSS_NAMES, gold['losses:' + flag].tolist()))
  _losses_close(tr.last_losses, want, 'reference --' + flag + ' step')
  # the other inference paths take the same generator input
  assert isinstance(tr.get_eval_loss(_clone(xd)), float)


def test_zero_sem_with_zero_ins_behaves_as_zero_sem():
  """model.py:585-588: --zero_ins is only consulted when --zero_sem is off (an elif), so the discriminator keeps its edge
  lane: bit-identical images and losses."""
  xd = omodel.synthetic_batch(2, 64, 128, seed=58)
  runs = []
  for flags in (dict(zero_sem=True), dict(zero_sem=True, zero_ins=True)):
    tr = _trainer(*_weights(1234), **flags)
    img = tr.get_img(_clone(xd))
    tr.step(_clone(xd))
    runs.append((img, dict(tr.last_losses)))
  assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
  # while --zero_ins alone is a different computation
  tr = _trainer(*_weights(1234), zero_ins=True)
  tr.step(_clone(xd))
  assert dict(tr.last_losses) != runs[0][1]


def test_zero_ins_is_a_no_op_under_no_instance():
  """model.py:588: `not self.opt.no_instance and self.opt.zero_ins` -- without an edge lane there is nothing to blank."""
  xd = omodel.synthetic_batch(2, 64, 128, seed=59)
  torch.manual_seed(1234)
  cfg = omodel.gen_cfg(omodel.default_opt(**NET))
  sd_G = nets.init_generator(cfg, 35 + 3, 3)
  sd_D = nets.init_discriminator(35 + 3, 8, 3, 2)
  runs = []
  for flags in (dict(no_instance=True), dict(no_instance=True, zero_ins=True)):
    tr = _trainer(sd_G, sd_D, **flags)
    img = tr.get_img(_clone(xd))
    tr.step(_clone(xd))
    runs.append((img, dict(tr.last_losses)))
  assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
