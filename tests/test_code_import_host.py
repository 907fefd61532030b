"""Receiver side of the learned codec, host only (no GPU): jpdse_code_import is declared, exported and refuses bad
arguments before any launch; ops.code_import refuses a wrong row length without touching the library; the bitstream file
(ctu.utils.bitstream) round-trips and refuses malformed files; the encoder knows its code shape and the trainer has the
decoder's two methods.  The numpy yardstick of the GPU tests (tests/code_import_ref.py) is pinned to hand-made examples."""
import ctypes
import inspect
import os
import re
import struct
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

import code_import_ref as cref  # noqa: E402


def test_code_import_is_declared_and_exported_under_version_2():
  header = open(os.path.join(ROOT, 'include', 'jpdse.h')).read()
  declared = set(re.findall(r'\b(jpdse_[a-zA-Z0-9_]+)\s*\(', header))
  assert 'jpdse_code_import' in declared, 'jpdse_code_import missing from include/jpdse.h'
  assert 'jpdse_code_import' in jpdse_hip.SIGNATURES
  # the same argument list as the export it inverts
  assert jpdse_hip.SIGNATURES['jpdse_code_import'] == jpdse_hip.SIGNATURES['jpdse_code_export']
  L = jpdse_hip.lib()
  assert hasattr(L, 'jpdse_code_import') and hasattr(ctypes.CDLL(jpdse_hip.DEV_LIB_PATH), 'jpdse_code_import')
  assert L.jpdse_version() == 2
  assert re.search(r'#define\s+JPDSE_ABI_VERSION\s+2\b', header)


def test_bad_arguments_are_refused_before_any_launch():
  """No device exists here: a call that got as far as a launch could not return JPDSE_EINVAL.  The return code and the
  jpdse_last_error() text of every refusal of this entry point are pinned here (tests/golden/ew_host_queries.json, the
  record of the older entry points' refusals, has no row for it)."""
  L = jpdse_hip.lib()
  P = ctypes.c_void_p(4096)          # never dereferenced: every call below is refused on its arguments

  def call(dtype=BF16, N=2, H=4, W=8, C=32, src=P, packed=1, dst=P):
    return L.jpdse_code_import(dtype, N, H, W, C, src, packed, dst, None)
  null, extent = 'code_import: null pointer', 'code_import: non-positive extent (N %d, H %d, W %d, C %d)'
  for what, kw, want in (('NULL in', dict(src=None), null), ('NULL b', dict(dst=None), null),
                         ('N = 0', dict(N=0), extent % (0, 4, 8, 32)), ('C = 0', dict(C=0), extent % (2, 4, 8, 0)),
                         ('dtype = 7', dict(dtype=7), 'code_import: bad dtype 7'), ('H < 0', dict(H=-1), extent % (2, -1, 8, 32)),
                         ('W = 0', dict(W=0, packed=0), extent % (2, 4, 0, 32)),
                         ('NULL in, fp32', dict(src=None, packed=0, dtype=F32), null)):
    L.jpdse_code_export(7, 0, 0, 0, 0, None, 0, None, None)      # leaves another call's message behind
    stale = jpdse_hip.last_error()
    assert call(**kw) == -1, what                                 # JPDSE_EINVAL
    msg = jpdse_hip.last_error()
    assert msg and msg != stale and 'code_import' in msg, (what, msg)
    assert msg == want, (what, msg)
  with pytest.raises(jpdse_hip.JpdseError):
    jpdse_hip.check(call(N=0), 'code_import')


def test_ops_code_import_refuses_a_wrong_row_length_without_the_library(monkeypatch):
  import jpdse_hip.ops as ops
  touched = lambda: (_ for _ in ()).throw(AssertionError('library touched'))
  monkeypatch.setattr(jpdse_hip, 'lib', touched)
  monkeypatch.setattr(ops, 'lib', touched)                       # ops binds `lib` at import time
  monkeypatch.setattr(jpdse_hip.streams, 'lib', touched)
  N, H, W, C = 2, 5, 7, 9                                         # 315 bits: 40 bytes
  for bad in (torch.zeros(N, 39, dtype=torch.uint8), torch.zeros(N, 41, dtype=torch.uint8),
              torch.zeros(N + 1, 40, dtype=torch.uint8), torch.zeros(N * 40, dtype=torch.uint8),
              torch.zeros(N, 314), torch.zeros(N, 316), torch.zeros(N, 40), torch.zeros(1, 315),
              torch.zeros(N, C, H, W), torch.zeros(N, 315, dtype=torch.float64)):
    with pytest.raises(ValueError, match='code_import'):
      ops.code_import(bad, N, H, W, C, BF16)


# ---- the yardstick ------------------------------------------------------------------------------------------------------------
def test_yardstick_on_hand_made_codes():
  # one image, C 3, H 1, W 3: elements in NCHW order c0 (+,-,+) c1 (-,-,+) c2 (0,+,-): bits 101 001 010 -> 0xA5, 0x00
  b = np.array([1, -1, 1, -1, -1, 1, 0, 1, -1], dtype=np.float32).reshape(1, 3, 1, 3)
  packed = cref.export_packed(b)
  assert packed.dtype == np.uint8 and packed.tolist() == [[0b10100101, 0b00000000]]
  assert cref.export_float(b).tolist() == [[1, 0, 1, 0, 0, 1, 0.5, 1, 0]]
  back = cref.import_packed(packed, 1, 3, 1, 3)
  want = b.copy()
  want[0, 2, 0, 0] = -1                                           # the exact zero was stored as a 0 bit
  assert back.dtype == np.float32 and np.array_equal(back, want)
  assert np.array_equal(cref.import_float(cref.export_float(b), 1, 3, 1, 3), want)
  # unused low bits of the last byte are ignored; every image starts on its own byte
  two = np.array([[0b10100101, 0b01111111], [0b00000000, 0b10000000]], dtype=np.uint8)
  got = cref.import_packed(two, 2, 3, 1, 3)
  assert np.array_equal(got[0], want[0]) and got[1].reshape(-1).tolist() == [-1] * 8 + [1]
  assert cref.import_float(np.array([[0.5, 0.50001, -3, np.nan, 1]], dtype=np.float32), 1, 5, 1, 1).reshape(-1).tolist() \
      == [-1, 1, -1, -1, 1]
  stored = cref.to_nhwc(want)
  assert stored.shape == (1, 1, 3, 8) and np.all(stored[..., 3:] == 0) and stored[0, 0, 1, :3].tolist() == [-1, -1, 1]


# ---- the file -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 1, 1), (7, 1, 1), (1, 2, 4), (1, 3, 3), (32, 4, 8)], ids=lambda s: '%dbits' % (s[0] * s[1] * s[2]))
def test_bitstream_file_round_trips(shape, tmp_path):
  from ctu.utils import bitstream
  bits = shape[0] * shape[1] * shape[2]
  assert bits in (1, 7, 8, 9, 32 * 4 * 8)
  g = np.random.default_rng(bits)
  b = np.where(g.random((1,) + shape) < 0.5, -1.0, 1.0).astype(np.float32)
  row = torch.from_numpy(cref.export_packed(b)[0])
  path = str(tmp_path / 'one.jpdc')
  n = bitstream.write_code(path, row, shape)
  assert n == os.path.getsize(path) == bitstream.HEADER_BYTES + (bits + 7) // 8
  raw = open(path, 'rb').read()
  assert raw[:4] == bitstream.MAGIC and struct.unpack('<IIII', raw[4:20]) == (bitstream.VERSION,) + shape
  got, got_shape = bitstream.read_code(path)
  assert got_shape == shape and got.dtype == torch.uint8 and got.device.type == 'cpu' and torch.equal(got, row)
  assert np.array_equal(cref.import_packed(got.numpy()[None], 1, *shape), b)
  with pytest.raises(ValueError):
    bitstream.write_code(path, torch.cat([row, row[:1]]), shape)          # a row that does not fit the shape


def test_bitstream_reader_refuses_malformed_files(tmp_path):
  from ctu.utils import bitstream
  shape = (32, 4, 8)
  row = torch.arange(128, dtype=torch.uint8)
  good = str(tmp_path / 'good.jpdc')
  bitstream.write_code(good, row, shape)
  raw = open(good, 'rb').read()
  assert torch.equal(bitstream.read_code(good)[0], row)

  def refused(name, data, match):
    path = str(tmp_path / name)
    with open(path, 'wb') as fh:
      fh.write(data)
    with pytest.raises(ValueError, match=match):
      bitstream.read_code(path)
  refused('magic', b'JPDX' + raw[4:], 'magic')
  refused('version', raw[:4] + struct.pack('<I', bitstream.VERSION + 1) + raw[8:], 'version')
  refused('truncated', raw[:-1], 'truncated')
  refused('overlong', raw + b'\x00', 'beyond')
  refused('header_only_half', raw[:10], 'header')


# ---- the layers ---------------------------------------------------------------------------------------------------------------
def test_encoder_code_shape():
  from ctu.models.pix2pixHD_networks import networks
  enc = networks.define_G(3, 3, 8, 'encoder', 4, binarize_encoder=True, encoder_binarizer_out_channels=32)
  assert enc.code_shape(64, 128) == (32, 4, 8)
  assert enc.code_shape(512, 1024) == (32, 32, 64)
  plain = networks.define_G(3, 3, 8, 'encoder', 4, binarize_encoder=False)
  with pytest.raises(AttributeError, match='Encoder: no binarizer found'):
    plain.code_shape(64, 128)
  with pytest.raises(AttributeError, match='Encoder: no binarizer found'):
    plain.decode_code(None)


def test_trainer_and_model_have_the_decoder_calls():
  from jpdse_hip import ops
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  from ctu.trainers.pix2pixHD_trainer import Pix2PixHDTrainer
  for cls in (Pix2PixHDModel, Pix2PixHDTrainer):
    assert list(inspect.signature(cls.decode).parameters) == ['self', 'code', 'x_dict']
    par = inspect.signature(cls.get_eval_metrics_decoded).parameters
    assert list(par) == ['self', 'code', 'x_dict', 'per_class'] and par['per_class'].default is False
    assert 'zero' in cls.decode.__doc__                                 # the zero rule is stated where the call is
  assert list(inspect.signature(ops.code_import).parameters)[:6] == ['code', 'N', 'H', 'W', 'C', 'dtype_code']
