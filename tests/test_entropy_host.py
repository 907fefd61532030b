"""Entropy-coded bitstream of the learned codec, host only (no GPU): the pure-Python coder tests/entropy_ref.py inverts
itself on every shape and input kind of the GPU tests; the .jpda container (ctu.utils.entropy) round-trips in both modes,
refuses malformed files and is never more than 4 bytes larger than the .jpdc file; two rate figures of the reference coder
sit inside bounds derived from the format; the four C entry points are declared, exported, answer their host queries and
refuse bad arguments before any launch."""
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
import entropy_cases as cases  # noqa: E402
import entropy_ref as eref  # noqa: E402

_shape = dict(argnames='shape', argvalues=cases.SHAPES, ids=cases.shape_id)


# ---- the yardstick ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize(**_shape)
def test_reference_round_trip(shape, kind):
  N, C, H, W = shape
  b, payloads, _ = cases.reference(shape, kind)
  assert (kind == 'zeros') == bool((b == 0).any())
  want = np.where(b > 0, np.float32(1), np.float32(-1))            # the zero rule of code_export: an exact 0 is bit 0
  assert np.array_equal(eref.decode(payloads, C, H, W), want)
  assert np.array_equal(cref.import_packed(cref.export_packed(b), N, C, H, W), want)
  for p in payloads:
    streams = eref.split_payload(p, C)
    assert len(streams) == C and all(4 <= len(s) <= eref.stream_capacity(H, W) for s in streams)
    assert len(p) <= C * (4 + eref.stream_capacity(H, W))


def test_reference_on_a_hand_checked_stream():
  """One symbol, bit 0, by hand from the format text: bound = (0xFFFFFFFF >> 11) * 1024 = 0x7FFFFC00, range = bound, no
  normalisation (range >= 2^24), low stays 0; the flush emits 0 five times, the first of which is not stored."""
  assert eref.encode_stream([0], 1, 1) == b'\0\0\0\0'
  # bit 1: low = bound = 0x7FFFFC00, range = 0xFFFFFFFF - bound; flush: 0x00 (dropped), 0x7F, 0xFF, 0xFC, 0x00
  assert eref.encode_stream([1], 1, 1) == bytes([0x7F, 0xFF, 0xFC, 0x00])
  assert eref.decode_stream(b'\0\0\0\0', 1, 1) == [0] and eref.decode_stream(bytes([0x7F, 0xFF, 0xFC, 0x00]), 1, 1) == [1]
  # bytes past the end read as 0, and the symbol count is fixed whatever the bytes are
  assert eref.decode_stream(b'', 2, 3) == [0] * 6
  assert len(eref.decode_stream(b'\xff' * 3, 2, 3)) == 6
  # the context: after a 1 at x = 0 of a row, x = 1 is coded in context `left` = 1, not 0 -- visible in the adapted tables
  p = eref.encode_image(np.array([[[1, 1, -1]]], dtype=np.float32))
  assert struct.unpack('<I', p[:4])[0] == len(p) - 4


def test_the_inputs_exercise_carry_propagation():
  total = eref.Counters()
  for shape in cases.SHAPES:
    total.add(cases.reference(shape, 'half')[2])
  assert total.carries_into_run2 >= 1 and total.longest_run >= 2 and total.carries >= 100


def test_rate_sanity_of_the_reference():
  """Bars from the format, not from the coder's output.  All-equal: the raw channel is 256 bytes, a quarter is 64.  i.i.d.:
  a probability stays within [31, 2017] of 2048, so a symbol costs less than log2(2048 / 31) < 6.05 bits, and the flush
  stores 4 bytes: 2048 * 6.05 / 8 + 4 < 1553 bytes.  Measured: 12 bytes (all -1), 20 bytes (all +1) and
  261 bytes (p = 0.5, seed 0; the raw channel is 256)."""
  H, W = 32, 64
  for v in (0, 1):
    n = len(eref.encode_stream([v] * (H * W), H, W))
    print('all-%d channel of 2048 symbols: %d bytes' % (v, n))
    assert n < 256 // 4
  bits = (np.random.default_rng(0).random(H * W) < 0.5).astype(np.uint8).tolist()
  data = eref.encode_stream(bits, H, W)
  print('i.i.d. p = 0.5 channel of 2048 symbols: %d bytes' % len(data))
  assert len(data) < 2048 * 6.05 / 8 + 4 and len(data) <= eref.stream_capacity(H, W)
  assert eref.decode_stream(data, H, W) == bits


# ---- the container --------------------------------------------------------------------------------------------------------------
def _coded_and_raw(shape, kind):
  """Per image of the case: (payload, packed row as a uint8 tensor)."""
  b, payloads, _ = cases.reference(shape, kind)
  rows = cref.export_packed(b)
  return [(payloads[n], torch.from_numpy(rows[n].copy())) for n in range(shape[0])]


@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize(**_shape)
def test_jpda_round_trip_and_the_four_byte_bound(shape, kind, tmp_path):
  from ctu.utils import bitstream, entropy
  N, C, H, W = shape
  for n, (payload, row) in enumerate(_coded_and_raw(shape, kind)):
    path, plain = str(tmp_path / ('i%d.jpda' % n)), str(tmp_path / ('i%d.jpdc' % n))
    size = entropy.write_coded(path, payload, row, (C, H, W))
    assert size == os.path.getsize(path) == entropy.file_bytes(len(payload), (C, H, W))
    assert size <= bitstream.write_code(plain, row, (C, H, W)) + 4
    raw = open(path, 'rb').read()
    mode = entropy.mode_of(len(payload), (C, H, W))
    assert raw[:4] == b'JPDA' and struct.unpack('<IIIII', raw[4:24]) == (1, C, H, W, mode)
    back, got_mode, got_shape = entropy.read_coded(path)
    assert (got_mode, got_shape) == (mode, (C, H, W))
    if mode == entropy.MODE_CODED:
      assert len(payload) < row.numel() and isinstance(back, bytes) and back == payload
    else:
      assert len(payload) >= row.numel() and back.dtype == torch.uint8 and torch.equal(back, row)
    if shape in ((1, 1, 1, 1), (2, 32, 4, 8)):
      assert mode == entropy.MODE_RAW, 'coding cannot pay here: the length table alone is as large as the raw code'


def test_both_modes_occur():
  from ctu.utils import entropy
  modes = {entropy.mode_of(len(p), s[1:]) for s in cases.SHAPES for k in cases.KINDS for p in cases.reference(s, k)[1]}
  assert modes == {entropy.MODE_RAW, entropy.MODE_CODED}
  assert entropy.mode_of(len(cases.reference((3, 64, 16, 33), 'blob')[1][0]), (64, 16, 33)) == entropy.MODE_CODED


def test_jpda_reader_refuses_malformed_files(tmp_path):
  from ctu.utils import entropy
  shape = (3, 64, 16, 33)
  (coded, row), = _coded_and_raw(shape, 'blob')[:1]
  (noise, noise_row), = _coded_and_raw(shape, 'half')[:1]
  cshape = shape[1:]
  good1, good0 = str(tmp_path / 'good1.jpda'), str(tmp_path / 'good0.jpda')
  entropy.write_coded(good1, coded, row, cshape)
  entropy.write_coded(good0, noise, noise_row, cshape)
  raw1, raw0 = open(good1, 'rb').read(), open(good0, 'rb').read()
  assert entropy.read_coded(good1)[1] == 1 and entropy.read_coded(good0)[1] == 0

  def refused(name, data, match):
    path = str(tmp_path / name)
    with open(path, 'wb') as fh:
      fh.write(data)
    with pytest.raises(ValueError, match=match):
      entropy.read_coded(path)
  word = lambda v: struct.pack('<I', v)
  for tag, raw in (('m1', raw1), ('m0', raw0)):
    refused(tag + 'magic', b'JPDC' + raw[4:], 'magic')
    refused(tag + 'version', raw[:4] + word(2) + raw[8:], 'version')
    refused(tag + 'mode', raw[:20] + word(2) + raw[24:], 'unknown mode')
    refused(tag + 'emptyC', raw[:8] + word(0) + raw[12:], 'empty code shape')
    refused(tag + 'emptyW', raw[:16] + word(0) + raw[20:], 'empty code shape')
    refused(tag + 'header', raw[:23], 'header')
  refused('m0short', raw0[:-1], 'truncated')
  refused('m0long', raw0 + b'\0', 'trailing')
  refused('m1table', raw1[:24 + 4 * 64 - 1], 'truncated')                       # the file ends inside the length table
  refused('m1short', raw1[:-1], 'length table sums to')
  refused('m1long', raw1 + b'\0', 'length table sums to')
  refused('m1sum', raw1[:24] + word(struct.unpack('<I', raw1[24:28])[0] + 1) + raw1[28:], 'length table sums to')
  # the writer refuses what the reader would
  with pytest.raises(ValueError, match='length table sums to'):
    entropy.write_coded(good1, coded[:-1], row, cshape)
  with pytest.raises(ValueError, match='bytes'):
    entropy.write_coded(good1, np.frombuffer(coded, dtype=np.uint8), row, cshape)
  with pytest.raises(ValueError, match='uint8 values in one row'):
    entropy.write_coded(good1, coded, row[:-1], cshape)
  with pytest.raises(ValueError, match='bad code shape'):
    entropy.write_coded(good1, coded, row, (0, 16, 33))


def test_bitstream_module_is_unchanged_by_the_container():
  from ctu.utils import bitstream, entropy
  assert bitstream.VERSION == 1 and bitstream.MAGIC == b'JPDC' and bitstream.HEADER_BYTES == 20
  assert entropy.HEADER_BYTES == 24 and entropy.SUFFIX == '.jpda'
  assert 'no entropy coding' in bitstream.__doc__


# ---- the ABI --------------------------------------------------------------------------------------------------------------------
NAMES = ('jpdse_code_entropy_capacity', 'jpdse_code_entropy_workspace_size', 'jpdse_code_entropy_encode',
         'jpdse_code_entropy_decode')


def test_entry_points_are_declared_and_exported_under_version_2():
  header = open(os.path.join(ROOT, 'include', 'jpdse.h')).read()
  declared = set(re.findall(r'\b(jpdse_[a-zA-Z0-9_]+)\s*\(', header))
  L, dev = jpdse_hip.lib(), ctypes.CDLL(jpdse_hip.DEV_LIB_PATH)
  for name in NAMES:
    assert name in declared and name in jpdse_hip.SIGNATURES and hasattr(L, name) and hasattr(dev, name), name
  assert declared == set(jpdse_hip.SIGNATURES.keys())
  # argument counts of the header's declarations against the ctypes table
  for name in NAMES:
    args = re.search(r'\b%s\s*\(([^)]*)\)\s*;' % name, header).group(1)
    assert len(args.split(',')) == len(jpdse_hip.SIGNATURES[name][1]), name
  assert L.jpdse_version() == 2 and re.search(r'#define\s+JPDSE_ABI_VERSION\s+2\b', header)


def test_host_queries_without_a_gpu():
  L = jpdse_hip.lib()
  cap, ws = L.jpdse_code_entropy_capacity, L.jpdse_code_entropy_workspace_size
  for N, C, H, W in cases.SHAPES + [(4, 128, 32, 64)]:
    assert cap(H, W, C) == C * (4 + H * W + 8) == C * (4 + eref.stream_capacity(H, W))
    slots = N * C * (H * W + 8)
    assert ws(N, H, W, C) == (slots + 15) // 16 * 16 + 4 * N * C
  # outside the limits: 0, never a wrapped size
  for H, W, C in ((0, 8, 32), (4, 0, 32), (4, 8, 0), (-1, 8, 32), (4, 4097, 32), (1 << 15, 4096, 32), (1 << 20, 2048, 1)):
    assert cap(H, W, C) == 0 and ws(1, H, W, C) == 0, (H, W, C)
  assert cap(1, 4096, 1) == 4 + 4096 + 8
  assert ws(0, 4, 8, 32) == 0 and ws(65536, 4, 8, 32) == 0 and ws(65535, 1, 1, 1) > 0


def test_bad_arguments_are_refused_before_any_launch():
  """No device exists here: a call that got as far as a launch could not return JPDSE_EINVAL."""
  L = jpdse_hip.lib()
  P = ctypes.c_void_p(4096)            # never dereferenced: every call below is refused on its arguments
  N, H, W, C = 2, 4, 8, 32
  cap, ws = L.jpdse_code_entropy_capacity(H, W, C), L.jpdse_code_entropy_workspace_size(N, H, W, C)

  def enc(dtype=BF16, N=N, H=H, W=W, C=C, b=P, out=P, stride=cap, sizes=P, status=P, wsp=P, ws_bytes=ws):
    return L.jpdse_code_entropy_encode(dtype, N, H, W, C, b, out, stride, sizes, status, wsp, ws_bytes, None)
  good_sizes = (ctypes.c_int32 * N)(4 * C, cap)

  def dec(dtype=F32, N=N, H=H, W=W, C=C, src=P, stride=cap, sizes=good_sizes, b=P):
    return L.jpdse_code_entropy_decode(dtype, N, H, W, C, src, stride, sizes, b, None)
  null, extent, limits = 'null pointer', 'non-positive extent', 'beyond the coder\'s limits'
  for who, call, cases_ in (
      ('code_entropy_encode', enc, [(dict(b=None), null), (dict(out=None), null), (dict(sizes=None), null),
                                    (dict(status=None), null), (dict(dtype=7), 'bad dtype 7'), (dict(N=0), extent),
                                    (dict(H=-1), extent), (dict(W=0), extent), (dict(C=0), extent), (dict(W=4097), limits),
                                    (dict(N=65536), limits), (dict(H=1 << 20, W=4096), limits),
                                    (dict(stride=cap - 1), 'below the payload capacity')]),
      ('code_entropy_decode', dec, [(dict(src=None), null), (dict(sizes=None), null), (dict(b=None), null),
                                    (dict(dtype=-1), 'bad dtype -1'), (dict(N=0), extent), (dict(C=-3), extent),
                                    (dict(W=4097), limits), (dict(stride=4 * C - 1), 'length table'),
                                    (dict(sizes=(ctypes.c_int32 * N)(4 * C, cap + 1)), 'payload 1 of %d bytes' % (cap + 1)),
                                    (dict(sizes=(ctypes.c_int32 * N)(4 * C - 1, cap)), 'payload 0 of %d bytes' % (4 * C - 1)),
                                    (dict(sizes=(ctypes.c_int32 * N)(-1, cap)), 'payload 0 of -1 bytes')])):
    for kw, want in cases_:
      L.jpdse_code_export(7, 0, 0, 0, 0, None, 0, None, None)      # leaves another call's message behind
      assert call(**kw) == -1, (who, kw)                            # JPDSE_EINVAL
      msg = jpdse_hip.last_error()
      assert msg.startswith(who + ': ') and want in msg, (who, kw, msg)
  for kw in (dict(wsp=None), dict(ws_bytes=ws - 1), dict(ws_bytes=0)):
    assert enc(**kw) == -2 and 'workspace too small' in jpdse_hip.last_error()      # JPDSE_EWORKSPACE, as jpdse_code_stats
  with pytest.raises(jpdse_hip.JpdseError):
    jpdse_hip.check(enc(N=0), 'code_entropy_encode')


def test_ops_decode_refuses_bad_payloads_without_the_library(monkeypatch):
  import jpdse_hip.ops as ops
  touched = lambda: (_ for _ in ()).throw(AssertionError('library touched'))
  monkeypatch.setattr(jpdse_hip, 'lib', touched)
  monkeypatch.setattr(ops, 'lib', touched)
  monkeypatch.setattr(jpdse_hip.streams, 'lib', touched)
  shape = (2, 3, 1, 9)
  good = list(cases.reference(shape, 'half')[1])
  bump = bytearray(good[0])
  bump[4] ^= 1
  for bad in (good[:1], good + good, good[0], None, [good[0], 'text'], [good[0], np.zeros(20, dtype=np.uint8)],
              [bytes(bump), good[1]], [good[0], good[1][:-1]], [good[0], good[1] + b'\0'], [good[0], b'\0' * 11]):
    with pytest.raises(ValueError, match='code_entropy_decode'):
      ops.code_entropy_decode(bad, 2, 1, 9, 3, BF16)


def test_trainer_and_model_have_the_coded_calls():
  from jpdse_hip import ops
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  from ctu.trainers.pix2pixHD_trainer import Pix2PixHDTrainer
  for cls in (Pix2PixHDModel, Pix2PixHDTrainer):
    assert list(inspect.signature(cls.get_coded).parameters) == ['self', 'x_dict']
    assert list(inspect.signature(cls.decode_coded).parameters) == ['self', 'payloads', 'x_dict']
    assert list(inspect.signature(cls.get_coded_rate).parameters) == ['self', 'x_dict']
  assert list(inspect.signature(ops.code_entropy_encode).parameters) == ['b']
  assert list(inspect.signature(ops.code_entropy_decode).parameters)[:6] == ['payloads', 'N', 'H', 'W', 'C', 'dtype_code']
