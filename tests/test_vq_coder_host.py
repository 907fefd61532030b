"""Coded index stream of the vector quantizer, host only (no GPU): the pure-Python coder tests/vq_coder_ref.py inverts
itself on every shape and input kind of the GPU tests and its inputs exercise the carry path; the size claims of DESIGN.md
4.14 hold on the reference coder; the .jpdv container (ctu.utils.vqstream) packs, round-trips and refuses malformed blobs,
one test per refusal; the four C entry points are declared, exported, answer their host queries with the closed forms and
refuse bad arguments before any launch."""
import ctypes
import inspect
import os
import re
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'jpd-se_amd'), os.path.dirname(os.path.abspath(__file__))):
  if _p not in sys.path:
    sys.path.insert(0, _p)

import jpdse_hip  # noqa: E402
from jpdse_hip import VqIndexEncodeArgs, VqIndexDecodeArgs  # noqa: E402

import vq_coder_cases as cases  # noqa: E402
import vq_coder_ref as vref  # noqa: E402

_shape = dict(argnames='shape', argvalues=cases.SHAPES, ids=cases.shape_id)


# ---- the yardstick ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize(**_shape)
def test_reference_round_trip(shape, kind):
  M, L, S = shape
  v, payload, _ = cases.reference(shape, kind)
  assert v.shape == (M,) and v.min() >= 0 and v.max() < L
  assert vref.decode(payload, M, L, S) == v.tolist()
  streams = vref.split_payload(payload, S)
  assert len(streams) == S
  for s, data in enumerate(streams):
    assert 4 <= len(data) <= vref.stream_capacity(M, L, S, s), (s, len(data))
  assert len(payload) <= vref.capacity(M, L, S) == vref.index_bits(L) * M + 12 * S


def test_reference_on_hand_checked_streams():
  """By hand from the format text.  L = 2: nb = 1, the one decision uses probs[1] and is 4.8's: a 0 leaves low at 0 (four
  stored zero bytes), a 1 sets low = bound = (0xFFFFFFFF >> 11) * 1024 = 0x7FFFFC00.  L = 4, symbol 2 = bits 1, 0: the first
  decision (probs[1]) is that 1; the second is coded with probs[3] = 1024, still untouched, as a 0 -- range becomes
  (0x80000003 >> 11) * 1024 and low stays 0x7FFFFC00: the same four bytes."""
  assert vref.index_bits(2) == 1 and vref.index_bits(3) == 2 and vref.index_bits(64) == 6 and vref.index_bits(65) == 7
  assert vref.index_bits(257) == 9 and vref.index_bits(512) == 9
  assert vref.encode_stream([0], 2) == b'\0\0\0\0'
  assert vref.encode_stream([1], 2) == bytes([0x7F, 0xFF, 0xFC, 0x00])
  assert vref.encode_stream([2], 4) == bytes([0x7F, 0xFF, 0xFC, 0x00])
  assert vref.decode_stream(bytes([0x7F, 0xFF, 0xFC, 0x00]), 1, 4) == ([2], False)
  # interleaving: stream s holds the symbols s, s + S, ...
  assert [vref.stream_count(65, 64, s) for s in (0, 1, 63)] == [2, 1, 1]
  p = vref.encode([1, 0, 0, 0, 1], 2, 2)
  assert vref.split_payload(p, 2) == [vref.encode_stream([1, 0, 1], 2), vref.encode_stream([0, 0], 2)]
  # bytes past the end read as 0, the count is fixed, and a value >= L is clipped to L - 1 and reported
  assert vref.decode_stream(b'', 5, 100) == ([0] * 5, False)
  out, clipped = vref.decode_stream(b'\xff' * 64, 40, 100)
  assert len(out) == 40 and clipped and max(out) == 99 and min(out) >= 0


def test_the_inputs_exercise_carry_propagation():
  total = vref.Counters()
  for shape in cases.SHAPES:
    total.add(cases.reference(shape, 'uniform')[2])
  print('carries %d, longest pending run %d, carries into a run >= 2: %d' % (total.carries, total.longest_run,
                                                                         total.carries_into_run2))
  assert total.carries_into_run2 >= 1 and total.longest_run >= 2 and total.carries >= 100


def test_size_claims_on_the_reference():
  """The bars are the packed size (mode 0) or a fraction of it, never a byte count of the coder.  Device payloads are
  byte-identical to the reference's (tests/test_hip_vq_coder.py), so these hold for the device coder too.  Measured
  (DESIGN.md 4.14): at (4096, 64, 64) geometric 2560 bytes and uniform 3574 against 3072 packed; all-equal at (16384, 64, 4)
  376 bytes (all 0, and all L - 1) against 12288 packed: six decisions per symbol at the floor of log2(2048 / 2017) = 0.022
  bits each."""
  from ctu.utils import vqstream
  shape = (4096, 64, 64)
  M, L, S = shape
  packed = vqstream.packed_bytes(M, L)
  assert packed == 3072
  for kind in ('geometric', 'uniform'):
    v, payload, _ = cases.reference(shape, kind)
    h = cases.entropy_bits(v, L) / 8
    print('%s %s: coded %d bytes, packed %d, zero-order entropy %.1f bytes, coded / entropy %.3f'
          % (cases.shape_id(shape), kind, len(payload), packed, h, len(payload) / h))
    blob = vqstream.build_blob((64, 64), L, S, payload, v)
    mode = struct.unpack_from('<I', blob, 24)[0]
    if kind == 'geometric':
      assert len(payload) < packed and mode == vqstream.MODE_CODED and len(blob) == vqstream.HEADER_BYTES + len(payload)
    else:
      assert len(payload) >= packed and mode == vqstream.MODE_PACKED and len(blob) == vqstream.HEADER_BYTES + packed
  shape = (16384, 64, 4)
  for kind in ('zeros', 'top'):
    _, payload, _ = cases.reference(shape, kind)
    print('%s %s: coded %d bytes, packed %d' % (cases.shape_id(shape), kind, len(payload), vqstream.packed_bytes(16384, 64)))
    assert len(payload) < vqstream.packed_bytes(16384, 64) / 4


# ---- mode 0 packing -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nb,M', [(1, 13), (7, 5), (9, 7)])
def test_pack_and_unpack(nb, M):
  from ctu.utils import vqstream
  assert (M * nb) % 8 != 0
  rng = np.random.default_rng(nb)
  v = rng.integers(0, 1 << nb, size=M)
  v[0], v[-1] = (1 << nb) - 1, 1 << (nb - 1)
  data = vqstream.pack_indices(v, nb)
  assert len(data) == (M * nb + 7) // 8
  # bit j of the string is bit j % 8 of byte j // 8, an index's least significant bit first
  for i, value in enumerate(v.tolist()):
    for k in range(nb):
      j = i * nb + k
      assert (data[j // 8] >> (j % 8)) & 1 == (value >> k) & 1
  assert data[-1] >> ((M * nb) % 8) == 0
  assert vqstream.unpack_indices(data, M, nb).tolist() == v.tolist()
  with pytest.raises(ValueError, match='bytes'):
    vqstream.unpack_indices(data + b'\0', M, nb)
  with pytest.raises(ValueError, match='padding'):
    vqstream.unpack_indices(data[:-1] + bytes([data[-1] | 0x80]), M, nb)
  with pytest.raises(ValueError, match='outside'):
    vqstream.pack_indices([1 << nb], nb)


# ---- the container --------------------------------------------------------------------------------------------------------------
def _blobs():
  """(a mode-1 blob, a mode-0 blob, the indices of each) at (3000, 100, 7) as a 60 x 50 code.  Mode 1: build_blob on the
  reference coder's payload.  Mode 0: put together by hand from the format text -- at L = 100 even uniform indices (6.64 bits
  each) code below their 7 packed bits, so the writer would not pick it (test_size_claims_on_the_reference has the writer
  choose mode 0, at L = 64)."""
  from ctu.utils import vqstream
  shape = (3000, 100, 7)
  v1, payload, _ = cases.reference(shape, 'geometric')
  b1 = vqstream.build_blob((60, 50), 100, 7, payload, v1)
  v0 = cases.reference(shape, 'uniform')[0]
  b0 = struct.pack('<4sIIIIII', b'JPDV', 1, 60, 50, 100, 0, 0) + vqstream.pack_indices(v0, 7)
  assert struct.unpack_from('<4sIIIIII', b1) == (b'JPDV', 1, 60, 50, 100, 7, 1) and b1[28:] == payload
  assert len(b0) == 28 + (3000 * 7 + 7) // 8
  return b1, b0, v1, v0


def _word(v):
  return struct.pack('<I', v)


def test_container_round_trip_on_the_host(tmp_path):
  from ctu.utils import vqstream
  b1, b0, v1, v0 = _blobs()
  n, code_len, L, S, mode, body = vqstream.parse_blob(b1)
  assert (n, code_len, L, S, mode) == (60, 50, 100, 7, 1) and body == cases.reference((3000, 100, 7), 'geometric')[1]
  assert vref.decode(body, 3000, 100, 7) == v1.tolist()
  n, code_len, L, S, mode, body = vqstream.parse_blob(b0)
  assert (n, code_len, L, S, mode) == (60, 50, 100, 0, 0) and body.tolist() == v0.tolist()
  # a packed file needs no device call: read_indices answers on the CPU, from bytes and from a path
  path = str(tmp_path / ('c' + vqstream.SUFFIX))
  with open(path, 'wb') as fh:
    fh.write(b0)
  for src in (b0, path):
    code = vqstream.read_indices(src, 'cpu')
    assert code.dtype.is_floating_point is False and tuple(code.shape) == (60, 50) and code.view(-1).tolist() == v0.tolist()
  assert vqstream.coded_bits(b0) == 8 * len(b0) == 8 * (28 + (3000 * 7 + 7) // 8)
  assert vqstream.coded_bits(b1) == 8 * len(b1)


def _refused(blob, match):
  from ctu.utils import vqstream
  touched = lambda *a, **k: (_ for _ in ()).throw(AssertionError('device call'))
  saved = vqstream.ops.vq_index_decode
  vqstream.ops.vq_index_decode = touched
  try:
    with pytest.raises(ValueError, match=match):
      vqstream.read_indices(blob, 'cpu')
    with pytest.raises(ValueError, match=match):
      vqstream.parse_blob(blob)
  finally:
    vqstream.ops.vq_index_decode = saved


@pytest.mark.parametrize('mode', [1, 0])
def test_reader_refuses_a_wrong_magic(mode):
  blob = _blobs()[1 - mode]
  _refused(b'JPDA' + blob[4:], 'magic')


@pytest.mark.parametrize('mode', [1, 0])
def test_reader_refuses_an_unknown_version(mode):
  blob = _blobs()[1 - mode]
  _refused(blob[:4] + _word(2) + blob[8:], 'version')


@pytest.mark.parametrize('mode', [1, 0])
def test_reader_refuses_an_unknown_mode(mode):
  blob = _blobs()[1 - mode]
  _refused(blob[:24] + _word(2) + blob[28:], 'unknown mode')


@pytest.mark.parametrize('mode', [1, 0])
def test_reader_refuses_L_out_of_range(mode):
  blob = _blobs()[1 - mode]
  for L in (0, 1, 513, 1 << 31):
    _refused(blob[:16] + _word(L) + blob[20:], 'n_center')


def test_reader_refuses_S_out_of_range():
  b1, b0 = _blobs()[:2]
  for S in (0, 3001, 65536):
    _refused(b1[:20] + _word(S) + b1[24:], 'streams')
  _refused(b0[:20] + _word(7) + b0[24:], 'streams in mode 0')
  # S is bounded by M as well as by 65535: a one-row code of 3 indices cannot hold 7 streams
  _refused(b1[:8] + _word(1) + _word(3) + b1[16:], 'streams')


@pytest.mark.parametrize('mode', [1, 0])
def test_reader_refuses_an_empty_shape(mode):
  blob = _blobs()[1 - mode]
  _refused(blob[:8] + _word(0) + blob[12:], 'empty code shape')
  _refused(blob[:12] + _word(0) + blob[16:], 'empty code shape')


def test_reader_refuses_truncated_data():
  b1, b0 = _blobs()[:2]
  _refused(b1[:27], 'header')
  _refused(b0[:10], 'header')
  _refused(b0[:-1], 'truncated')
  _refused(b1[:28 + 4 * 7 - 1], 'truncated')                      # the blob ends inside the length table
  _refused(b1[:-1], 'length table sums to')


def test_reader_refuses_trailing_bytes():
  b1, b0 = _blobs()[:2]
  _refused(b0 + b'\0', 'trailing')
  _refused(b1 + b'\0', 'length table sums to')


def test_reader_refuses_a_length_table_that_does_not_add_up():
  b1 = _blobs()[0]
  first = struct.unpack_from('<I', b1, 28)[0]
  _refused(b1[:28] + _word(first + 1) + b1[32:], 'length table sums to')
  _refused(b1[:28] + _word(0xFFFFFFFF) + b1[32:], 'length table sums to')


def test_reader_refuses_a_packed_value_beyond_L():
  from ctu.utils import vqstream
  b0, v0 = _blobs()[1], _blobs()[3]
  v = v0.copy()
  v[1234] = 100                                                    # 7 bits hold it, the alphabet does not
  _refused(b0[:28] + vqstream.pack_indices(v, 7), 'packed value 100')
  v[1234] = 99
  assert vqstream.read_indices(b0[:28] + vqstream.pack_indices(v, 7), 'cpu').view(-1).tolist() == v.tolist()


def test_writer_refuses_what_the_reader_would():
  from ctu.utils import vqstream
  v, payload, _ = cases.reference((3000, 100, 7), 'uniform')
  with pytest.raises(ValueError, match='length table sums to'):
    vqstream.build_blob((60, 50), 100, 7, payload[:-1], v)
  with pytest.raises(ValueError, match='bytes'):
    vqstream.build_blob((60, 50), 100, 7, np.frombuffer(payload, dtype=np.uint8), v)
  with pytest.raises(ValueError, match='3000 indices'):
    vqstream.build_blob((60, 51), 100, 7, payload, v)
  with pytest.raises(ValueError, match='empty code shape'):
    vqstream.build_blob((0, 50), 100, 7, payload, v)
  with pytest.raises(ValueError, match='n_center'):
    vqstream.build_blob((60, 50), 513, 7, payload, v)
  with pytest.raises(ValueError, match='streams'):
    vqstream.build_blob((60, 50), 100, 0, payload, v)
  bad = v.copy()
  bad[7] = 100
  with pytest.raises(ValueError, match='outside'):
    vqstream.build_blob((60, 50), 100, 7, payload, bad)
  import torch
  with pytest.raises(ValueError, match='int64'):
    vqstream.write_indices(None, torch.zeros((4, 4), dtype=torch.int32), 64)


def test_vqstream_surface():
  from ctu.utils import vqstream
  from jpdse_hip import ops
  assert vqstream.MAGIC == b'JPDV' and vqstream.VERSION == 1 and vqstream.SUFFIX == '.jpdv' and vqstream.HEADER_BYTES == 28
  assert list(inspect.signature(vqstream.write_indices).parameters) == ['path', 'code', 'n_center', 'n_streams']
  assert inspect.signature(vqstream.write_indices).parameters['n_streams'].default == 64
  assert list(inspect.signature(vqstream.read_indices).parameters) == ['blob_or_path', 'device']
  assert list(inspect.signature(vqstream.coded_bits).parameters) == ['blob']
  assert list(inspect.signature(vqstream.reconstruct).parameters) == ['s2h', 'blob_or_path']
  assert list(inspect.signature(ops.vq_index_encode).parameters) == ['index', 'L', 'S']
  assert list(inspect.signature(ops.vq_index_decode).parameters) == ['payload', 'M', 'L', 'S', 'device']
  assert [ops.vq_index_bits(L) for L in (2, 3, 4, 5, 64, 65, 100, 256, 257, 512)] == [1, 2, 2, 3, 6, 7, 7, 8, 9, 9]


def test_ops_decode_refuses_bad_payloads_without_the_library(monkeypatch):
  import jpdse_hip.ops as ops
  touched = lambda: (_ for _ in ()).throw(AssertionError('library touched'))
  monkeypatch.setattr(jpdse_hip, 'lib', touched)
  monkeypatch.setattr(ops, 'lib', touched)
  monkeypatch.setattr(jpdse_hip.streams, 'lib', touched)
  M, L, S = 3000, 100, 7
  good = cases.reference((M, L, S), 'uniform')[1]
  bump = bytearray(good)
  bump[0] ^= 1
  for bad in (good[:-1], good + b'\0', bytes(bump), good[:4 * S - 1], b'', None, np.frombuffer(good, dtype=np.uint8), 'text'):
    with pytest.raises(ValueError, match='vq_index_decode'):
      ops.vq_index_decode(bad, M, L, S)
  for kw in (dict(L=1), dict(L=513), dict(S=0), dict(S=M + 1), dict(M=0), dict(M=1 << 30, L=512)):
    with pytest.raises(ValueError, match='vq_index_decode'):
      a = dict(M=M, L=L, S=S)
      a.update(kw)
      ops.vq_index_decode(good, a['M'], a['L'], a['S'])
  with pytest.raises(ValueError, match='vq_index_decode'):
    ops.vq_index_decode(good, 70000, L, 65536)


# ---- the ABI --------------------------------------------------------------------------------------------------------------------
NAMES = ('jpdse_vq_index_capacity', 'jpdse_vq_index_workspace_size', 'jpdse_vq_index_encode', 'jpdse_vq_index_decode')


def test_entry_points_are_declared_and_exported():
  header = open(os.path.join(ROOT, 'include', 'jpdse.h')).read()
  declared = set(re.findall(r'\b(jpdse_[a-zA-Z0-9_]+)\s*\(', header))
  L, dev = jpdse_hip.lib(), ctypes.CDLL(jpdse_hip.DEV_LIB_PATH)
  for name in NAMES:
    assert name in declared and name in jpdse_hip.SIGNATURES and hasattr(L, name) and hasattr(dev, name), name
  assert declared == set(jpdse_hip.SIGNATURES.keys())
  # the argument structs against the header's: the same fields in the same order
  for cname, cls in (('jpdse_vq_index_encode_args', VqIndexEncodeArgs), ('jpdse_vq_index_decode_args', VqIndexDecodeArgs)):
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (cname, cname), header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = re.findall(r'(\w+)\s*[,;]', body)
    assert names == [f[0].rstrip('_') for f in cls._fields_], (names, cls._fields_)
  assert L.jpdse_version() == 2


def test_host_queries_against_the_closed_forms():
  L = jpdse_hip.lib()
  cap, ws = L.jpdse_vq_index_capacity, L.jpdse_vq_index_workspace_size
  for M, n_center, S in cases.SHAPES + [(1048576, 64, 64), (1048576, 64, 4096), (1 << 20, 512, 65535)]:
    nb = vref.index_bits(n_center)
    assert cap(M, n_center, S) == vref.capacity(M, n_center, S) == nb * M + 12 * S
    assert ws(M, n_center, S) == (nb * M + 8 * S + 15) // 16 * 16 + 8 * S
  # outside the limits: 0, never a wrapped size
  for M, n_center, S in ((0, 64, 1), (-1, 64, 1), (8, 1, 1), (8, 513, 1), (8, 0, 1), (8, 64, 0), (8, 64, -2), (8, 64, 9),
                         (70000, 64, 65536), ((1 << 31) - 1, 4, 1), (1 << 29, 16, 1), ((1 << 31) - 64, 2, 65535)):
    assert cap(M, n_center, S) == 0 and ws(M, n_center, S) == 0, (M, n_center, S)
  assert cap((1 << 31) - 64, 2, 1) == (1 << 31) - 64 + 12                      # nb = 1: just inside
  assert cap(65535, 2, 65535) == 65535 * 13 and cap(8, 64, 8) == 48 + 96


def test_bad_arguments_are_refused_before_any_launch():
  """No device exists here: a call that got as far as a launch could not return JPDSE_EINVAL."""
  lb = jpdse_hip.lib()
  P = 4096                                 # never dereferenced: every call below is refused on its arguments
  M, L, S = 3000, 100, 7
  cap, ws = lb.jpdse_vq_index_capacity(M, L, S), lb.jpdse_vq_index_workspace_size(M, L, S)

  def enc(M=M, L=L, S=S, index=P, out=P, out_bytes=cap, size=P, status=P, wsp=P, ws_bytes=ws):
    return lb.jpdse_vq_index_encode(ctypes.byref(VqIndexEncodeArgs(M, L, S, index, out, out_bytes, size, status, wsp, ws_bytes, None)))

  def dec(M=M, L=L, S=S, src=P, in_bytes=cap, index=P, status=P):
    return lb.jpdse_vq_index_decode(ctypes.byref(VqIndexDecodeArgs(M, L, S, src, in_bytes, index, status, None)))
  null = 'null pointer'
  limits = [(dict(L=1), 'n_center L = 1'), (dict(L=513), 'n_center L = 513'), (dict(M=0), 'M = 0'), (dict(M=-5), 'M = -5'),
            (dict(S=0), 'S = 0 streams'), (dict(S=M + 1), 'S = 3001 streams'), (dict(M=70000, S=65536), 'S = 65536 streams'),
            (dict(M=1 << 29, L=16), 'below 2^31'), (dict(M=(1 << 31) - 64, L=2, S=65535), 'below 2^31')]
  for who, call, cases_ in (
      ('vq_index_encode', enc, limits + [(dict(index=None), null), (dict(out=None), null), (dict(size=None), null),
                                         (dict(status=None), null), (dict(out_bytes=cap - 1), 'below the payload capacity'),
                                         (dict(wsp=None), 'workspace too small'), (dict(ws_bytes=ws - 1), 'workspace too small')]),
      ('vq_index_decode', dec, limits + [(dict(src=None), null), (dict(index=None), null), (dict(status=None), null),
                                         (dict(in_bytes=4 * S - 1), 'length table'), (dict(in_bytes=-1), 'length table'),
                                         (dict(in_bytes=1 << 31), '2^31')])):
    for kw, want in cases_:
      lb.jpdse_code_export(7, 0, 0, 0, 0, None, 0, None, None)      # leaves another call's message behind
      assert call(**kw) == -1, (who, kw)                            # JPDSE_EINVAL
      msg = jpdse_hip.last_error()
      assert msg.startswith(who + ': ') and want in msg, (who, kw, msg)
  for fn, name in ((lb.jpdse_vq_index_encode, 'vq_index_encode'), (lb.jpdse_vq_index_decode, 'vq_index_decode')):
    assert fn(None) == -1 and jpdse_hip.last_error().startswith(name + ': null argument struct')
  with pytest.raises(jpdse_hip.JpdseError):
    jpdse_hip.check(enc(S=0), 'vq_index_encode')
