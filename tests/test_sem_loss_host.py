"""CPU-only checks of the semantics-weighted distortion (jpdse_sem_weighted_loss): the flag parser and the
model's refusals (before any network or device work, with the GPU hidden), every JPDSE_EINVAL of the entry point with its
text, and the float64 yardstick of the GPU test (tests/sem_loss_ref.py) against hand-written examples.  No device kernel is
launched here."""
import ctypes
import math
import os
import re

import pytest
import torch

import jpdse_hip
from jpdse_hip import F32, BF16
from oracle.ctu_cpu import model as omodel

import sem_loss_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_declared_bound_and_exported():
  header = open(os.path.join(ROOT, 'include', 'jpdse.h')).read()
  declared = set(re.findall(r'\b(jpdse_[a-zA-Z0-9_]+)\s*\(', header))
  assert 'jpdse_sem_weighted_loss' in declared and 'jpdse_sem_weighted_loss' in jpdse_hip.SIGNATURES
  L = jpdse_hip.lib()
  assert hasattr(L, 'jpdse_sem_weighted_loss') and hasattr(ctypes.CDLL(jpdse_hip.DEV_LIB_PATH), 'jpdse_sem_weighted_loss')
  assert L.jpdse_version() == 2
  from jpdse_hip import ops
  assert callable(ops.sem_weighted_loss) and ops.SEM_TABLE == 256


# ---- flags ------------------------------------------------------------------------------------------------------------------
def test_parser_builds_the_table():
  from ctu.models.pix2pixHD_model import parse_class_distortion_weights as parse
  assert parse('', 35) == [1.0] * 35
  assert parse(None, 4) == [1.0] * 4
  t = parse('24:4,26:2', 35)
  assert len(t) == 35 and t[24] == 4.0 and t[26] == 2.0 and sum(t) == 33.0 + 6.0
  assert parse(' 0:0 , 3:0.25,1:1e1 ', 4) == [0.0, 10.0, 1.0, 0.25]
  assert parse('0:1', 3) == [1.0, 1.0, 1.0]
  assert parse('255:2', 256)[255] == 2.0


def test_flags_are_declared_with_their_defaults():
  import argparse
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  p = Pix2PixHDModel.modify_commandline_options(argparse.ArgumentParser(), True)
  o = p.parse_args([])
  assert o.class_distortion_weights == '' and o.edge_distortion_weight == 1.0
  o = p.parse_args(['--class_distortion_weights', '24:4,26:2', '--edge_distortion_weight', '3'])
  assert o.class_distortion_weights == '24:4,26:2' and o.edge_distortion_weight == 3.0
  for dest in ('class_distortion_weights', 'edge_distortion_weight'):             # the normaliser is said where the flag is
    assert 'lambda_distortion' in [a for a in p._actions if a.dest == dest][0].help


def _hidden_gpu(monkeypatch):
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  touched = lambda: (_ for _ in ()).throw(AssertionError('library touched'))
  import jpdse_hip.ops, jpdse_hip.layers  # noqa: E401
  monkeypatch.setattr(jpdse_hip, 'lib', touched)
  monkeypatch.setattr(jpdse_hip.ops, 'lib', touched)           # ops binds `lib` at import time


REFUSED = [
    (dict(class_distortion_weights='24'), 'label:weight'),                       # malformed
    (dict(class_distortion_weights='24:4:1'), 'label:weight'),
    (dict(class_distortion_weights='24:4,,26:2'), 'label:weight'),
    (dict(class_distortion_weights='road:4'), 'not an integer'),
    (dict(class_distortion_weights='2.5:4'), 'not an integer'),
    (dict(class_distortion_weights='24:heavy'), 'not a number'),
    (dict(class_distortion_weights='24:-1'), 'finite number >= 0'),
    (dict(class_distortion_weights='24:nan'), 'finite number >= 0'),
    (dict(class_distortion_weights='24:inf'), 'finite number >= 0'),
    (dict(class_distortion_weights='-1:2'), 'outside'),
    (dict(class_distortion_weights='35:2'), 'outside'),                          # n_onehot = 35
    (dict(class_distortion_weights='256:2', num_labels=300), 'outside'),         # the table holds 256 entries
    (dict(class_distortion_weights='24:4,24:2'), 'twice'),
    (dict(edge_distortion_weight=-0.5), 'edge_distortion_weight'),
    (dict(edge_distortion_weight=float('nan')), 'edge_distortion_weight'),
    (dict(edge_distortion_weight=float('inf')), 'edge_distortion_weight'),
    (dict(edge_distortion_weight=3.0, no_instance=True), 'no_instance'),
    (dict(class_distortion_weights='24:4', distortion_loss_fn='ms_ssim'), 'ms_ssim'),
    (dict(edge_distortion_weight=2.0, distortion_loss_fn='ms_ssim'), 'ms_ssim'),
]


@pytest.mark.parametrize('over,text', REFUSED, ids=[','.join('%s=%s' % kv for kv in o.items()) for o, _ in REFUSED])
def test_bad_flags_raise_value_error_before_device_work(over, text, monkeypatch):
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  _hidden_gpu(monkeypatch)
  with pytest.raises(ValueError, match=text):
    Pix2PixHDModel(omodel.default_opt(gpu_ids=[0], ngf=8, ndf=8, n_blocks_global=1, **over))


@pytest.mark.parametrize('over', [dict(), dict(class_distortion_weights='0:1'), dict(class_distortion_weights='0:1,34:1.0'),
                                  dict(edge_distortion_weight=1.0, no_instance=True),
                                  dict(class_distortion_weights='3:1', distortion_loss_fn='ms_ssim')],
                         ids=['defaults', '0:1', '0:1,34:1.0', 'edge 1 with no_instance', '3:1 with ms_ssim'])
def test_trivial_weights_pass_the_checks_and_reach_the_device_check(over, monkeypatch):
  """All-ones weights are no weights: nothing is refused, and the constructor gets as far as asking for the GPU."""
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  with pytest.raises(jpdse_hip.JpdseError, match='no GPU visible'):
    Pix2PixHDModel(omodel.default_opt(gpu_ids=[0], ngf=8, ndf=8, n_blocks_global=1, **over))


# ---- the entry point's refusals -------------------------------------------------------------------------------------------------
def test_every_einval_comes_before_any_launch_with_its_text():
  L = jpdse_hip.lib()
  dummy = (ctypes.c_double * 16)()
  p = ctypes.cast(dummy, ctypes.c_void_p).value
  ones = (ctypes.c_float * 256)(*([1.0] * 256))
  need = L.jpdse_loss_workspace_size(0)

  def call(dtype=F32, n=1, h=8, w=8, c=3, kind=0, fake=p, real=p, label=p, inst=p, table=ones, n_table=35, edge_w=1.0,
           scale=1.0, out=p, dfake=None, ws=p, nbytes=need):
    args = jpdse_hip.SemLossArgs(dtype, n, h, w, c, kind, fake, real, label, inst, table, n_table, edge_w, scale, out, dfake,
                                 ws, nbytes, None)
    return L.jpdse_sem_weighted_loss(ctypes.byref(args))

  def refused(text, **kw):
    assert call(**kw) == -1, kw
    assert text in jpdse_hip.last_error(), (kw, jpdse_hip.last_error())

  assert L.jpdse_sem_weighted_loss(None) == -1 and 'null argument struct' in jpdse_hip.last_error()
  for name in ('fake', 'real', 'label', 'out'):
    refused('null argument', **{name: None})
  refused('null argument', table=ctypes.POINTER(ctypes.c_float)())
  refused('dtype', dtype=7)
  refused('dtype', dtype=-1)
  refused('kind', kind=2)
  refused('kind', kind=-1)
  for name in ('n', 'h', 'w', 'c'):
    refused('non-positive extent', **{name: 0})
    refused('non-positive extent', **{name: -3})
  refused('exceed 2^31 - 1', n=4, h=1 << 15, w=1 << 14)
  refused('table of', n_table=0)
  refused('table of', n_table=257)
  refused('workspace too small', nbytes=need - 1)
  refused('workspace too small', ws=None)
  for bad in (-1.0, float('nan'), float('inf'), -float('inf')):
    t = (ctypes.c_float * 256)(*([1.0] * 256))
    t[17] = bad
    refused('class weight 17', table=t)
    refused('edge weight', edge_w=bad, dtype=BF16)
  t = (ctypes.c_float * 256)(*([1.0] * 256))
  t[40] = -1.0                                    # past n_table: not part of the table
  refused('workspace too small', table=t, nbytes=0)
  refused('scale is NaN', scale=float('nan'), dfake=p)
  with pytest.raises(jpdse_hip.JpdseError, match='kind'):
    jpdse_hip.check(call(kind=5), 'sem_weighted_loss')


# ---- the yardstick ----------------------------------------------------------------------------------------------------------
def test_yardstick_edge_rule_on_a_hand_written_example():
  # row 0 ends in 2 and row 1 starts with 1: adjacent in memory (the row wrap), not neighbours
  inst = torch.tensor([[[1, 1, 1, 2],
                        [1, 1, 1, 1],
                        [1, 3, 1, 1]]])
  want = torch.tensor([[[0, 0, 1, 1],
                        [0, 1, 0, 1],
                        [1, 1, 1, 0]]], dtype=torch.bool)
  assert torch.equal(ref.edges(inst), want)
  assert not ref.edges(inst)[0, 1, 0]             # (1, 0): its memory predecessor is the 2 of (0, 3)
  # two images that differ only across the batch boundary: no edge anywhere
  two = torch.stack([torch.full((3, 4), 5), torch.full((3, 4), 6)])
  assert not ref.edges(two).any()
  # ids that float32 cannot tell apart
  big = torch.tensor([[[2 ** 30 + 1, 2 ** 30 + 2]]])
  assert big.float()[0, 0, 0] == big.float()[0, 0, 1]
  assert torch.equal(ref.edges(big), torch.tensor([[[True, True]]]))
  assert not ref.edges(torch.tensor([[[7]]])).any()


def test_yardstick_weight_map_value_and_gradient():
  label = torch.tensor([[[0.0, 1.0, 2.9, -1.0],
                         [300.0, 2.0, -0.5, float('nan')],
                         [1.0, 1.0, 3.0, 256.0]]])
  inst = torch.tensor([[[1, 1, 1, 2],
                        [1, 1, 1, 1],
                        [1, 3, 1, 1]]])
  table = [0.0, 0.5, 4.0]                         # label 3 and beyond: outside the table, weight 1
  w = ref.weight_map(label, None, table, 3.0)
  assert torch.equal(w, torch.tensor([[[0.0, 0.5, 4.0, 1.0],
                                       [1.0, 4.0, 0.0, 1.0],
                                       [0.5, 0.5, 1.0, 1.0]]], dtype=torch.float64))
  we = ref.weight_map(label, inst, table, 3.0)
  e = ref.edges(inst)
  assert torch.equal(we, torch.where(e, 3.0 * w, w)) and torch.equal(ref.weight_map(label, inst, table, 1.0), w)
  g = torch.Generator().manual_seed(3)
  fake = torch.randn(1, 3, 3, 4, generator=g, dtype=torch.float64)
  real = torch.randn(1, 3, 3, 4, generator=g, dtype=torch.float64)
  # all-ones weights are the plain means
  ones = [1.0] * 3
  assert math.isclose(ref.loss(fake, real, label, inst, ones, 1.0, 'l1'), (fake - real).abs().mean().item(), rel_tol=1e-15)
  assert math.isclose(ref.loss(fake, real, label, inst, ones, 1.0, 'mse'), ((fake - real) ** 2).mean().item(), rel_tol=1e-15)
  # by hand: sum over pixels of w * sum_c f(d), over N H W C
  for kind, f in (('l1', lambda d: d.abs()), ('mse', lambda d: d * d)):
    by_hand = sum(we[0, y, x].item() * f(fake[0, :, y, x] - real[0, :, y, x]).sum().item() for y in range(3) for x in range(4)) / 36
    assert math.isclose(ref.loss(fake, real, label, inst, table, 3.0, kind), by_hand, rel_tol=1e-14)
    # the gradient is the derivative of the value
    fr = fake.clone().requires_grad_(True)
    (2.5 * (we[:, None] * f(fr - real)).sum() / 36).backward()
    assert torch.allclose(ref.grad(fake, real, label, inst, table, 3.0, kind, 2.5), fr.grad, rtol=1e-14, atol=0)
