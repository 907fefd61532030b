"""Learned codec, host side (no GPU): the numpy Philox4x32-10 of the test helper against the Random123 known-answer
vectors, the encoder's reference checkpoint layout, and every still-refused flag combination failing before any
device work."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'jpd-se_amd'), os.path.dirname(os.path.abspath(__file__))):
  if p not in sys.path:
    sys.path.insert(0, p)

import learned_codec_util as lcu  # noqa: E402
from oracle.ctu_cpu import model as omodel  # noqa: E402


@pytest.mark.parametrize('ctr,key,want', [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_numpy_philox_known_answers(ctr, key, want):
  got = lcu.philox4x32_10(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))
  assert tuple(int(x) for x in got) == want


def test_codec_noise_layout():
  """u of element e is word e & 3 of the block e >> 2; images and draws get independent streams."""
  u = lcu.codec_noise(3, 5, 4, 6, seed=0x123456789, draw=7)
  assert u.shape == (5, 4, 6) and u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
  e = 37
  words = lcu.philox4x32_10(np.array([e >> 2, 3, 7, 0], dtype=np.uint32), np.array([0x23456789, 0x1], dtype=np.uint32))
  assert u.reshape(-1)[e] == np.float32(int(words[e & 3]) >> 8) * np.float32(2.0 ** -24)
  assert not np.array_equal(u, lcu.codec_noise(4, 5, 4, 6, seed=0x123456789, draw=7))
  assert not np.array_equal(u, lcu.codec_noise(3, 5, 4, 6, seed=0x123456789, draw=8))


def test_encoder_state_dict_matches_reference_layout():
  """nef 8, n_downsample_E 4, B 32: the keys / shapes of a reference net_E.pth (networks.py:307-350)."""
  from ctu.models.pix2pixHD_networks import networks
  enc = networks.define_G(3, 3, 8, 'encoder', 4, binarize_encoder=True, encoder_binarizer_out_channels=32)
  sd = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
  want = {}
  for i, (ci, co) in zip((1, 4, 7, 10, 13), ((3, 8), (8, 16), (16, 32), (32, 64), (64, 128))):
    k = 7 if i == 1 else 3
    want['model.%d.weight' % i], want['model.%d.bias' % i] = (co, ci, k, k), (co,)
  want['model.16.conv.weight'] = (32, 128, 1, 1)
  for i, (ci, co) in zip((17, 20, 23, 26), ((32, 64), (64, 32), (32, 16), (16, 8))):
    want['model.%d.weight' % i], want['model.%d.bias' % i] = (ci, co, 3, 3), (co,)
  want['model.30.weight'], want['model.30.bias'] = (3, 8, 7, 7), (3,)
  assert sd == want
  plain = networks.define_G(3, 3, 8, 'encoder', 4, binarize_encoder=False)
  assert tuple(plain.state_dict()['model.16.weight'].shape) == (128, 64, 3, 3)     # first ConvT takes nef * 2^n
  with pytest.raises(AttributeError, match='no binarizer'):
    plain(torch.zeros(1, 3, 32, 32), mode='get_binary_code')


def _codec_opts(**over):
  kw = dict(no_feat_encoding=False, no_encoder_binarization=False, feat_num=3, nef=8, n_downsample_E=4,
            encoder_binarizer_out_channels=32)
  kw.update(over)
  return omodel.default_opt(**kw)


@pytest.mark.parametrize('over', [
    dict(no_generator_binarization=False),
    dict(no_label_encoding=False),
    dict(sem_masking=True),
    dict(inst_wise_pool=True),
    dict(netE_groups=2),
    dict(use_netE_output=True),
    dict(pool_size=5),
    dict(netG='local'),
    dict(n_downsample_E=0),
], ids=lambda d: ','.join('%s=%s' % kv for kv in d.items()))
def test_still_refused_combinations_fail_before_device_work(over, monkeypatch):
  """Every combination outside the accelerated learned-codec path raises NotImplementedError in Pix2PixHDModel.__init__,
  before any network (hence any device allocation) exists -- checked with the GPU hidden."""
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  import jpdse_hip
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  touched = lambda: (_ for _ in ()).throw(AssertionError('library touched'))
  import jpdse_hip.ops, jpdse_hip.layers  # noqa: E401
  monkeypatch.setattr(jpdse_hip, 'lib', touched)
  monkeypatch.setattr(jpdse_hip.ops, 'lib', touched)           # ops binds `lib` at import time
  monkeypatch.setattr(jpdse_hip.streams, 'lib', touched)
  with pytest.raises(NotImplementedError):
    Pix2PixHDModel(_codec_opts(gpu_ids=[0], **over))


def test_oracle_composition_equals_reference_golden(golden_dir):
  """The torch-CPU learned-codec composition the GPU tests compare against (tests/test_hip_learned_codec.py: CodecOracle) is
  pinned to the REAL reference: fed the reference's own noise, one step reproduces tests/golden/learned_codec_nef8.npz's six
  losses and E gradients exactly."""
  from test_hip_learned_codec import CodecOracle
  import test_hip_learned_codec_golden as tg
  z = np.load(os.path.join(golden_dir, 'learned_codec_nef8.npz'))
  gold = {k: z[k] for k in z.files}
  sd_G, sd_D, sd_E = tg._weights(gold)
  opt = omodel.default_opt(ngf=8, ndf=8, n_blocks_global=1, no_feat_encoding=False, no_encoder_binarization=False,
                           feat_num=3, nef=8, n_downsample_E=4, encoder_binarizer_out_channels=32, seed=0)
  ora = CodecOracle(opt, sd_E, sd_G=sd_G, sd_D=sd_D)
  ora.u_override = torch.from_numpy(gold['step_u'])
  ora.step(tg._batch(gold))
  for name, v in zip(gold['step_loss_names'], gold['step_losses']):
    assert ora.last_losses[str(name)] == float(v), str(name)
  for k in gold:
    if k.startswith('step_E_g:'):
      assert np.array_equal(ora.G['E.' + k[len('step_E_g:'):]].grad.numpy(), gold[k]), k
