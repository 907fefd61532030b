"""Wide label sets (ADE20K: num_labels=150 + don't-care + instance edge = 155 input channels), host only (no GPU):
jpdse_input_builder_wide is declared, exported and refuses bad arguments before any launch; jpdse_input_builder keeps its
recorded refusal of 72 storage channels; the model's channel bookkeeping at 151 classes; and the torch-CPU oracle, which no
other fixture runs above 39 input channels, reproduces what the reference computed at this width
(tests/golden/wide_labels_ngf8.npz, scripts/make_golden_wide_labels.py)."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'jpd-se_amd'), os.path.dirname(os.path.abspath(__file__))):
  if _p not in sys.path:
    sys.path.insert(0, _p)

import jpdse_hip  # noqa: E402
from jpdse_hip import F32, BF16  # noqa: E402
from oracle.ctu_cpu import model as omodel  # noqa: E402

import wide_labels_util as wl  # noqa: E402

RTOL = 2e-5          # tests/test_oracle_golden.py: oracle network outputs against the reference's, max-abs over the output's max
LOSS_RTOL = 1e-4     # tests/test_oracle_golden.py: oracle step losses and gradient norms against the reference's


def test_wide_builder_is_declared_and_exported_under_version_2():
  header = open(os.path.join(ROOT, 'include', 'jpdse.h')).read()
  declared = set(re.findall(r'\b(jpdse_[a-zA-Z0-9_]+)\s*\(', header))
  assert 'jpdse_input_builder_wide' in declared, 'jpdse_input_builder_wide missing from include/jpdse.h'
  assert 'jpdse_input_builder_wide' in jpdse_hip.SIGNATURES
  # the same argument list as the entry point it widens
  assert jpdse_hip.SIGNATURES['jpdse_input_builder_wide'] == jpdse_hip.SIGNATURES['jpdse_input_builder']
  L = jpdse_hip.lib()
  assert hasattr(L, 'jpdse_input_builder_wide') and hasattr(ctypes.CDLL(jpdse_hip.DEV_LIB_PATH), 'jpdse_input_builder_wide')
  assert L.jpdse_version() == 2
  assert re.search(r'#define\s+JPDSE_ABI_VERSION\s+2\b', header)


def _call(entry, dtype=BF16, N=1, H=8, W=8, num_labels=150, label=4096, inst=4096, n_dst=2, dst=(4096, 4096), img=(4096, 4096),
          cs=160, img_cs=8, c0=152, nch=3):
  """Pointers are never dereferenced: every call below is refused on its arguments (no device exists here: a call that got
  as far as a launch could not return JPDSE_EINVAL)."""
  P = ctypes.c_void_p
  arr = lambda v: None if v is None else (P * len(v))(*v)
  return entry(dtype, N, H, W, num_labels, P(label), P(inst), n_dst, arr(dst), arr(img), cs, img_cs, c0, nch, None)


def test_wide_builder_refuses_bad_arguments_before_any_launch():
  L = jpdse_hip.lib()
  three = (4096, 4096, 4096, 4096)
  for what, kw in (('null destination', dict(dst=(4096, None))),
                   ('null destination array', dict(dst=None)),
                   ('n_dst = 0', dict(n_dst=0)),
                   ('n_dst = 4', dict(n_dst=4, dst=three, img=three)),
                   ('cs % 8 != 0', dict(cs=156)),
                   ('num_labels == cs', dict(num_labels=160)),
                   ('num_labels > cs', dict(num_labels=161)),
                   ('image channels past cs', dict(c0=158)),
                   ('image channels before 0', dict(c0=-1)),
                   ('no image channels', dict(nch=0)),
                   ('bad dtype', dict(dtype=2)),
                   ('null label', dict(label=None)),
                   ('N = 0', dict(N=0)),
                   ('fp32, cs % 8 != 0', dict(dtype=F32, cs=260, c0=256, num_labels=255))):
    L.jpdse_code_export(7, 0, 0, 0, 0, None, 0, None, None)      # leaves another call's message behind
    stale = jpdse_hip.last_error()
    assert _call(L.jpdse_input_builder_wide, **kw) == -1, what    # JPDSE_EINVAL
    msg = jpdse_hip.last_error()
    assert msg and msg != stale and 'input_builder' in msg, (what, msg)
  # the refusals are those of jpdse_input_builder, text included
  for kw in (dict(cs=40, num_labels=40, c0=36), dict(cs=40, num_labels=35, c0=38), dict(cs=40, num_labels=35, c0=36, n_dst=4, dst=three, img=three),
             dict(cs=40, num_labels=35, c0=36, dst=(4096, None))):
    assert _call(L.jpdse_input_builder, **kw) == -1
    narrow = jpdse_hip.last_error()
    assert _call(L.jpdse_input_builder_wide, **kw) == -1
    assert jpdse_hip.last_error() == narrow
  with pytest.raises(jpdse_hip.JpdseError):
    jpdse_hip.check(_call(L.jpdse_input_builder_wide, n_dst=0), 'input_builder')


def test_narrow_builder_still_refuses_72_storage_channels_with_its_recorded_message():
  fix = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'ew_host_queries.json')))
  recorded = [c for c in fix['refusals'] if c[0] == 'jpdse_input_builder' and 'unsupported storage width' in c[1]]
  assert len(recorded) == 2 and all(c[3] == -1 for c in recorded)
  L = jpdse_hip.lib()
  for dtype, rec in zip((BF16, F32), recorded):
    assert _call(L.jpdse_input_builder, dtype=dtype, num_labels=35, cs=72, c0=36) == -1
    assert jpdse_hip.last_error() == rec[4] == 'input_builder: 72 storage channels unsupported (<= 64)'


def test_ops_input_builder_picks_the_entry_point_by_storage_width(monkeypatch):
  import jpdse_hip.ops as ops
  calls = []

  class Lib(object):
    def jpdse_input_builder(self, *a):
      calls.append(('narrow', a[10]))
      return 0

    def jpdse_input_builder_wide(self, *a):
      calls.append(('wide', a[10]))
      return 0
  monkeypatch.setattr(ops, 'lib', lambda: Lib())
  monkeypatch.setattr(ops, '_stream', lambda: None)
  lab, ins = torch.zeros(1, 1, 2, 2), torch.zeros(1, 1, 2, 2, dtype=torch.int64)
  for C, want in ((39, 'narrow'), (58, 'narrow'), (64, 'narrow'), (65, 'wide'), (69, 'wide'), (155, 'wide'), (259, 'wide')):
    d = ops.Act(torch.zeros(1, 2, 2, (C + 7) & ~7), C)
    ops.input_builder(lab, ins, C - 4, [d], [None], C - 3)
    assert calls[-1] == (want, (C + 7) & ~7), (C, calls[-1])


def test_model_channel_bookkeeping_at_151_classes():
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  opt = omodel.default_opt(print_losses=False, **wl.NET)
  m = Pix2PixHDModel(opt)
  assert m.n_onehot == wl.N_ONEHOT == 151 and m.label_nc == wl.LABEL_NC == 152
  assert m.label_nc + m.feat_nc == wl.INPUT_NC == 155
  sd_G, sd_D = wl.weights(1234)
  assert {k: tuple(v.shape) for k, v in m.netG.state_dict().items()} == {k: tuple(v.shape) for k, v in sd_G.items()}
  assert {k: tuple(v.shape) for k, v in m.netD.state_dict().items()} == {k: tuple(v.shape) for k, v in sd_D.items()}
  assert tuple(m.netG.state_dict()['model.1.weight'].shape) == (8, 155, 7, 7)
  assert tuple(m.netD.state_dict()['scale1_layer0.0.weight'].shape) == (8, 155, 4, 4)
  assert omodel.semantics_nc(opt) == 152


def test_synthetic_batch_emits_the_dontcare_id():
  """num_labels counts the ids synthetic_batch draws from: 151 covers ADE20K's 150 labels and the don't-care id 150."""
  from ctu.utils import synthetic
  xd = synthetic.synthetic_batch(4, 512, 512, seed=3, num_labels=wl.N_ONEHOT)
  assert int(xd['label'].max()) == 150 and int(xd['label'].min()) >= 0
  assert torch.equal(xd['label'], omodel.synthetic_batch(4, 512, 512, seed=3, num_labels=wl.N_ONEHOT)['label'])


@pytest.fixture(scope='module')
def gold(golden_dir):
  return wl.load_gold(golden_dir)


def test_golden_is_data_at_the_stated_shape(gold):
  assert int(gold['num_labels']) == 150 and (int(gold['batch']), int(gold['height']), int(gold['width'])) == (2, 32, 64)
  assert tuple(str(n) for n in gold['loss_names']) == omodel.LOSS_NAMES
  lab = gold['label']
  assert lab.shape == (2, 1, 32, 64) and lab.max() == 150 and lab.min() == 0 and len(np.unique(lab)) > 60
  assert gold['gradG:model.1.weight'].shape == (8, 155, 7, 7) and gold['gradD:scale0_layer0.0.weight'].shape == (8, 155, 4, 4)
  assert all(v.dtype != object for v in gold.values())
  assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'wide_labels_ngf8.npz')) < 1 << 20


def test_oracle_reproduces_the_reference_at_155_input_channels(gold):
  sd_G, sd_D = wl.weights(int(gold['seed']))
  assert list(sd_G.keys()) == [str(k) for k in gold['Gkeys']] and list(sd_D.keys()) == [str(k) for k in gold['Dkeys']]
  np.testing.assert_allclose([float(v.double().norm()) for v in sd_G.values()], gold['Gnorm'], rtol=1e-12)
  np.testing.assert_allclose([float(v.double().norm()) for v in sd_D.values()], gold['Dnorm'], rtol=1e-12)
  ora = omodel.OracleTrainer(omodel.default_opt(**wl.NET), sd_G=sd_G, sd_D=sd_D)
  xd = wl.batch(gold)
  # the one-hot input the oracle builds: 151 class lanes + the edge lane, the don't-care id in lane 150
  pre = omodel.preprocess(xd, ora.opt)
  assert tuple(pre.shape) == (2, 152, 32, 64) and torch.equal(pre[:, :151].sum(1), torch.ones(2, 32, 64))
  assert torch.equal(pre[:, 150], (xd['label'][:, 0] == 150).float()) and pre[:, 150].sum() > 0 and pre[:, 151].sum() > 0
  img = ora.get_img(wl.clone(xd)).numpy().astype(np.float64)
  ref = gold['get_img'].astype(np.float64)
  err, scale = np.abs(img - ref).max(), np.abs(ref).max()
  print('oracle get_img vs reference: max abs error %.3e, bound %.3e' % (err, RTOL * scale))
  assert err <= RTOL * scale
  ora.step(wl.clone(xd), keep_grads=True)
  got = [ora.last_losses[k] for k in omodel.LOSS_NAMES]
  print('oracle losses %s\nreference     %s' % (got, gold['losses'].tolist()))
  np.testing.assert_allclose(got, gold['losses'], rtol=LOSS_RTOL)
  for key, grads in (('gradG:', ora.grads_G), ('gradD:', ora.grads_D)):
    for k in [f for f in gold if f.startswith(key)]:
      g, r = grads[k[len(key):]].double(), torch.from_numpy(gold[k]).double()
      rel = ((g - r).norm() / r.norm()).item()
      print('oracle %s vs reference: norms %.6e / %.6e, relative L2 difference %.3e' % (k, g.norm().item(), r.norm().item(), rel))
      np.testing.assert_allclose(g.norm().item(), r.norm().item(), rtol=LOSS_RTOL)


def test_zero_sem_oracle_reproduces_the_reference_record(golden_dir):
  """wl.ZeroSemOracle, the yardstick of the GPU test of --zero_sem at 151 classes, against what the reference recorded for the
  flag at 36 semantic lanes (tests/golden/zero_flags_ngf8.npz, scripts/make_golden_zero_flags.py)."""
  from oracle.ctu_cpu import nets
  z = np.load(os.path.join(golden_dir, 'zero_flags_ngf8.npz'))
  net = dict(ngf=8, ndf=8, n_blocks_global=1)
  torch.manual_seed(int(z['seed']))
  sd_G = nets.init_generator(omodel.gen_cfg(omodel.default_opt(**net)), 36 + 3, 3)
  sd_D = nets.init_discriminator(36 + 3, 8, 3, 2)
  ora = wl.ZeroSemOracle(omodel.default_opt(**net), sd_G=sd_G, sd_D=sd_D)
  xd = omodel.synthetic_batch(int(z['batch']), int(z['height']), int(z['width']), seed=int(z['img_seed']))
  img, ref = ora.get_img(wl.clone(xd)).numpy().astype(np.float64), z['img:zero_sem'].astype(np.float64)
  assert np.abs(img - ref).max() <= RTOL * np.abs(ref).max()
  ora.step(wl.clone(xd))
  np.testing.assert_allclose([ora.last_losses[k] for k in omodel.LOSS_NAMES], z['losses:zero_sem'], rtol=LOSS_RTOL)
