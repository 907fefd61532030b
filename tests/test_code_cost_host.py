"""Code-length map of the learned codec, host side (no GPU): the three entry points in the header, the
library and the ctypes table; the cost table against Python's math.log2 entry by entry; every refusal answered before any
launch, with its message; the workspace query; the identities of the Python restatement (tests/code_cost_ref.py); the bound
between the model's code length and the bytes the Python CODER (tests/rc_ref.py / tests/entropy_ref.py) writes, on the codes
the device tests use; and the trainer's refusal without an encoder binarizer, with the GPU hidden."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'jpd-se_amd'), os.path.dirname(os.path.abspath(__file__))):
  if p not in sys.path:
    sys.path.insert(0, p)

import jpdse_hip  # noqa: E402
from jpdse_hip import F32, BF16, CodeCostArgs  # noqa: E402
import code_cost_cases as cases  # noqa: E402
import code_cost_ref as ccref  # noqa: E402

NAMES = ('jpdse_code_cost_table', 'jpdse_code_cost_workspace_size', 'jpdse_code_cost')
_shape = dict(argnames='shape', argvalues=cases.SHAPES, ids=cases.shape_id)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_exported_under_version_2():
  header = open(os.path.join(ROOT, 'include', 'jpdse.h')).read()
  declared = set(re.findall(r'\b(jpdse_[a-zA-Z0-9_]+)\s*\(', header))
  L, dev = jpdse_hip.lib(), ctypes.CDLL(jpdse_hip.DEV_LIB_PATH)
  for name in NAMES:
    assert name in declared, name + ' missing from include/jpdse.h'
    assert name in jpdse_hip.SIGNATURES and hasattr(L, name) and hasattr(dev, name), name
  assert L.jpdse_version() == 2 and re.search(r'#define\s+JPDSE_ABI_VERSION\s+2\b', header)
  # the struct of the header, field by field, against the ctypes mirror
  body = re.search(r'typedef struct jpdse_code_cost_args \{(.*?)\} jpdse_code_cost_args;', header, re.S).group(1)
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  fields = [f.strip().lstrip('*') for decl in body.split(';') if decl.strip()
            for f in re.sub(r'^\s*(const\s+)?\w+\s*\**', '', decl.strip()).split(',')]
  assert fields == [f[0] for f in CodeCostArgs._fields_]


def test_cost_table_equals_the_python_rule_entry_by_entry():
  L = jpdse_hip.lib()
  out = (ctypes.c_uint32 * 2049)()
  assert L.jpdse_code_cost_table(out) == 0
  got = list(out)
  assert got[0] == 0 and got[2048] == 0
  for v in range(1, 2048):
    assert got[v] == round(-math.log2(v / 2048) * 65536), v
  assert tuple(got) == ccref.table()
  assert max(got) == got[1] and got[1024] == 65536 and got[31] == 396218     # T[31]: the dearest symbol a stream can hold
  assert L.jpdse_code_cost_table(None) == -1 and 'null pointer' in jpdse_hip.last_error()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_workspace_query():
  ws = jpdse_hip.lib().jpdse_code_cost_workspace_size
  for N, C, h, w in cases.SHAPES + [(4, 128, 32, 64)]:
    want = (2049 * 4 + 255) // 256 * 256 + 4 * N * h * w * C
    assert ws(N, h, w, C, 0) == ws(N, h, w, C, 35) == ws(N, h, w, C, 256) == want
  # every shape the call refuses: 0, never a wrapped size
  for N, h, w, C, k in ((0, 4, 8, 32, 0), (2, 0, 8, 32, 0), (2, 4, 0, 32, 0), (2, 4, 8, 0, 0), (-1, 4, 8, 32, 0),
                        (2, 4, 4097, 32, 0), (65536, 4, 8, 32, 0), (2, 4, 8, 64 * 65535 + 1, 0), (2, 1 << 20, 4096, 512, 0),
                        (65535, 1 << 30, 4096, 1 << 20, 0), (2, 4, 8, 32, -1), (2, 4, 8, 32, 257)):
    assert ws(N, h, w, C, k) == 0, (N, h, w, C, k)
  assert ws(65535, 1, 1, 1, 256) > 0 and ws(1, 1, 4096, 1, 0) > 0


def test_bad_arguments_are_refused_before_any_launch():
  """No device exists here: a call that got as far as a copy or a launch could not return JPDSE_EINVAL / JPDSE_EWORKSPACE."""
  L = jpdse_hip.lib()
  P = 4096                             # never dereferenced: every call below is refused on its arguments
  N, h, w, C = 2, 4, 8, 32
  need = L.jpdse_code_cost_workspace_size(N, h, w, C, 35)

  def call(**over):
    kw = dict(dtype=BF16, N=N, h=h, w=w, C=C, b=P, H=64, W=128, label=P, n_classes=35, symbol=P, cell=P, channel=P,
              class_units=P, class_pixels=P, ws=P, ws_bytes=need, stream=None)
    kw.update(over)
    return L.jpdse_code_cost(ctypes.byref(CodeCostArgs(**kw)))
  extent = 'non-positive extent'
  refused = [
      (dict(b=None), 'null pointer b'), (dict(cell=None), 'null pointer cell or channel'),
      (dict(channel=None), 'null pointer cell or channel'), (dict(class_units=None), 'null pointer class_units or class_pixels'),
      (dict(class_pixels=None), 'null pointer class_units or class_pixels'),
      (dict(dtype=7), 'bad dtype 7'), (dict(dtype=-1), 'bad dtype -1'),
      (dict(N=0), extent), (dict(h=-1), extent), (dict(w=0), extent), (dict(C=0), extent), (dict(H=0), extent), (dict(W=-4), extent),
      (dict(w=4097, W=4097 * 16), 'above the walk\'s row limit 4096'),
      (dict(N=65536), 'beyond the limits'), (dict(C=64 * 65535 + 1), 'beyond the limits'),
      (dict(h=1 << 20, w=4096, C=512), 'beyond the limits'),
      (dict(H=64, W=64), 'power-of-two multiple'),        # 16 x and 8 x
      (dict(H=12, W=24), 'power-of-two multiple'),        # 3 x
      (dict(H=2, W=4), 'power-of-two multiple'),          # below the code's own size
      (dict(H=65, W=128), 'power-of-two multiple'),
      (dict(n_classes=0), 'n_classes 0 outside [1, 256]'), (dict(n_classes=257), 'n_classes 257 outside [1, 256]'),
      (dict(n_classes=-3), 'n_classes -3 outside [1, 256]'),
  ]
  for over, text in refused:
    assert call(**over) == -1, over
    assert jpdse_hip.last_error().startswith('code_cost: ') and text in jpdse_hip.last_error(), (over, jpdse_hip.last_error())
  for over in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
    assert call(**over) == -2 and 'workspace too small' in jpdse_hip.last_error(), over
  assert call(ws=P + 4) == -1 and 'not 16-byte aligned' in jpdse_hip.last_error()
  assert L.jpdse_code_cost(None) == -1 and 'null argument struct' in jpdse_hip.last_error()
  # without a label map the class arguments are not read: the same bad values get past the argument checks, as far as the
  # workspace check (the last one before the device is touched)
  for over in (dict(H=0), dict(H=65, W=128), dict(n_classes=999), dict(class_units=None, class_pixels=None), dict(symbol=None)):
    assert call(label=None, ws_bytes=need - 1, **over) == -2, over
  with pytest.raises(jpdse_hip.JpdseError, match='power-of-two multiple'):
    jpdse_hip.check(call(H=12, W=24), 'code_cost')


# ---- the yardstick ----------------------------------------------------------------------------------------------------------
def test_reference_on_hand_worked_streams():
  T = ccref.table()
  # one symbol: probability 1024 either way, one bit
  assert ccref.stream_costs([0], 1, 1) == [65536] and ccref.stream_costs([1], 1, 1) == [65536]
  # a row of three zeros: context 0 each time, q = 1024 -> 1056 -> 1087
  assert ccref.stream_costs([0, 0, 0], 1, 3) == [T[1024], T[1056], T[1087]]
  # 1 1 / 0 1: contexts 0, 1 (left), 2 | 8 (up, upright), 2 | 4 (up, upleft); every context is met for the first time
  assert ccref.stream_costs([1, 1, 0, 1], 2, 2) == [T[1024]] * 4
  # a column of ones: context 0, then context 2 (up) from its start value, then again with q = 1024 - 32
  assert ccref.stream_costs([1, 1, 1], 3, 1) == [T[1024], T[1024], T[2048 - 992]]
  assert ccref.adapted(1024, 0) == 1056 and ccref.adapted(1024, 1) == 992 and ccref.adapted(2017, 0) == 2017 and ccref.adapted(31, 1) == 31


@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize(**_shape)
def test_reference_identities(shape, kind):
  N, C, h, w = shape
  b, r = cases.reference(shape, kind)
  assert r['symbol'].shape == (N, h, w, C) and r['symbol'].min() >= ccref.table()[2017] and r['symbol'].max() <= ccref.table()[31]
  assert np.array_equal(r['cell'].sum(axis=(1, 2)), r['channel'].sum(axis=1))
  for s, n_classes in ((2, 35), (16, 151)):
    label = cases.make_label(N, s * h, s * w, n_classes, seed=s)
    units, pixels = ccref.class_tables(r['cell'], label, n_classes)
    assert np.array_equal(units.sum(axis=1), s * s * r['cell'].sum(axis=(1, 2)))
    assert np.array_equal(pixels.sum(axis=1), np.full(N, s * s * h * w))
    assert (pixels[:, -1] >= 1).all() and (units[:, -1] > 0).all()        # the strays of make_label: the remainder row is in use


@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize(**_shape)
def test_stream_size_bound_against_the_python_coder(shape, kind):
  """|8 * stream bytes - units / 65536| <= 48 + h * w / 64 per stream, the bytes being those the Python
  restatement of the CODER writes -- no device, no kernel: this is where the derivation is checked."""
  N, C, h, w = shape
  _, r = cases.reference(shape, kind)
  gap = 8.0 * cases.stream_bytes(shape, kind) - r['channel'] / 65536.0
  print('%s %s: 8 * bytes - bits in [%.3f, %.3f], bound %.3f' % (cases.shape_id(shape), kind, gap.min(), gap.max(),
                                                                 ccref.bound_bits(h, w)))
  assert np.abs(gap).max() <= ccref.bound_bits(h, w)


# ---- the trainer --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method', ['get_rate_map', 'get_class_rates'])
def test_trainer_refuses_without_an_encoder_binarizer_before_device_work(method, monkeypatch):
  """The ValueError of the other coded paths (get_code, get_coded, decode), with the GPU hidden and the library untouched.  A
  model cannot be constructed without a device, so the trainer here is a bare one around a model without an encoder -- and
  around one whose encoder does not binarize: the two states the check tells apart."""
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  from ctu.trainers.pix2pixHD_trainer import Pix2PixHDTrainer
  from oracle.ctu_cpu import model as omodel
  import jpdse_hip.ops, jpdse_hip.layers  # noqa: E401
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  touched = lambda: (_ for _ in ()).throw(AssertionError('library touched'))
  monkeypatch.setattr(jpdse_hip, 'lib', touched)
  monkeypatch.setattr(jpdse_hip.ops, 'lib', touched)           # ops binds `lib` at import time
  xd = omodel.synthetic_batch(1, 32, 64, seed=3)

  class PlainEncoder(torch.nn.Module):
    binarize = False

  for enc in (None, PlainEncoder()):
    model = Pix2PixHDModel.__new__(Pix2PixHDModel)
    torch.nn.Module.__init__(model)
    model.netE = enc
    tr = Pix2PixHDTrainer.__new__(Pix2PixHDTrainer)
    torch.nn.Module.__init__(tr)
    tr.opt, tr.mode, tr.model = None, 'test', model
    with pytest.raises(ValueError, match='binary codes need the learned codec with encoder binarization'):
      getattr(tr, method)(xd)
    with pytest.raises(ValueError, match='binary codes need the learned codec with encoder binarization'):
      model(xd, None, mode=method)
