"""Context-coded index planes of the vector quantizer, host only (no GPU): the pure-Python coder tests/vq_plane_ref.py inverts
itself on every shape and source of the GPU tests and its inputs exercise the carry path; the two size conditions of DESIGN.md
4.19 hold between the two reference coders; the .jpdw container (ctu.utils.vqplane) round-trips and refuses malformed blobs,
one test per refusal; the four C entry points are declared, exported, answer their host queries with the closed forms and
refuse bad arguments before any launch; the model's flag parses, is refused without s2hvq, and the receiver tells the two
containers by their magic."""
import argparse
import ctypes
import inspect
import os
import re
import struct
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'jpd-se_amd'), os.path.dirname(os.path.abspath(__file__))):
  if _p not in sys.path:
    sys.path.insert(0, _p)

import jpdse_hip  # noqa: E402
from jpdse_hip import VqPlaneEncodeArgs, VqPlaneDecodeArgs  # noqa: E402

import vq_coder_ref as vref  # noqa: E402
import vq_plane_cases as cases  # noqa: E402
import vq_plane_ref as pref  # noqa: E402
from test_vq_bottleneck_host import _codec_opts, _hide_device  # noqa: E402

_shape = dict(argnames='shape', argvalues=cases.SHAPES, ids=cases.shape_id)


# ---- the yardstick ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize(**_shape)
def test_reference_round_trip(shape, kind):
  h, w, G, L, strip_rows = shape
  v, payload, _ = cases.reference(shape, kind)
  assert v.shape == (h * w * G,) and v.min() >= 0 and v.max() < L
  assert pref.decode(payload, *shape) == v.tolist()
  K = pref.strips(h, strip_rows)
  streams = pref.split_payload(payload, K * G)
  for s, data in enumerate(streams):
    assert 4 <= len(data) <= pref.stream_capacity(h, w, L, strip_rows, s // G), (s, len(data))
  assert len(payload) <= pref.capacity(*shape) == (pref.index_bits(L) + 2) * h * w * G + 12 * K * G


def test_sources_are_what_they_are_called():
  shape = (16, 8, 5, 100, 3)
  h, w, G, L, _ = shape
  cell = lambda v: v.reshape(h, w, G)
  s = cell(cases.indices(shape, 'stripes'))
  assert (s[1:] == s[:-1]).all() and (s[:, 1:] != s[:, :-1]).all()
  r = cell(cases.indices(shape, 'ramp'))
  assert r[3, 2, 4] == (3 * w + 2 + 4) % L
  assert set(cases.indices(shape, 'zeros')) == {0} and set(cases.indices(shape, 'top')) == {L - 1}
  big = cases.indices(cases.WORKLOAD, 'correlated').reshape(32, 64, 16)
  left = float((big[:, 1:] == big[:, :-1]).mean())
  assert 0.55 < left < 0.70, left              # 0.6, and the few chance matches of the other two branches


def test_reference_on_hand_checked_streams():
  """By hand from the format text.  One symbol without neighbours is 4.14's: the literal alone, tree node 1 at entry 11.  Two
  equal symbols in a row at L = 2: the literal of the first, then the left flag, bit 1, with entry 0 (no upper cell: every
  comparison false) -- the same two decisions, each with an untouched probability of 1024, as the order-0 coder makes for the
  symbols (first, 1) with its one tree node... but in two different table entries, so the bytes are those of two decisions with
  p = 1024.  A column of two equal symbols: the upper flag, bit 1, with entry 10."""
  assert pref.encode_stream([[0]], 2) == vref.encode_stream([0], 2) == b'\0\0\0\0'
  assert pref.encode_stream([[1]], 2) == vref.encode_stream([1], 2)
  assert pref.encode_stream([[2]], 4) == vref.encode_stream([2], 4)

  class Spy(object):
    """The decisions an encoder is asked to make."""

    def __init__(self):
      self.seen = []

    def encode(self, probs, ctx, bit):
      self.seen.append((ctx, bit))

    def finish(self):
      return b''

  def decisions(rows, L):
    spy, saved = Spy(), pref.Encoder
    pref.Encoder = lambda counters=None: spy
    try:
      pref.encode_stream(rows, L)
    finally:
      pref.Encoder = saved
    return spy.seen

  # L = 4, nb = 2: a literal is the nodes 1 and 2 | bit at the entries 11 and 12 / 13
  assert decisions([[2]], 4) == [(11, 1), (13, 0)]
  assert decisions([[2, 2]], 4) == [(11, 1), (13, 0), (0, 1)]
  assert decisions([[2, 1]], 4) == [(11, 1), (13, 0), (0, 0), (11, 0), (12, 1)]
  assert decisions([[2], [2]], 4) == [(11, 1), (13, 0), (10, 1)]
  assert decisions([[2], [3]], 4) == [(11, 1), (13, 0), (10, 0), (11, 1), (13, 1)]
  # second row of [[1, 2], [1, 2]]: (1, 0) has only an upper cell; (1, 1): Lf = 1, U = 2, UL = 1 -> entry 0 | 2 | 0, miss, then
  # the upper flag with entry 8 + (UL == Lf) = 9, hit
  assert decisions([[1, 2], [1, 2]], 4)[-3:] == [(10, 1), (2, 0), (9, 1)]
  # second row of [[1, 1], [3, 1]]: at (1, 1) Lf = 3, U = 1, UL = 1 -> entry 4 (UL == U), miss; upper flag entry 8, hit
  assert decisions([[1, 1], [3, 1]], 4)[-2:] == [(4, 0), (8, 1)]
  # second row of [[1, 1], [1, 0]]: at (1, 1) Lf = U = UL = 1 -> entry 7, miss; U == Lf: no upper flag, the literal follows
  assert decisions([[1, 1], [1, 0]], 4)[-3:] == [(7, 0), (11, 0), (12, 0)]
  # streams: s = k * G + g, strips never look above their first row
  p = pref.encode([0, 1, 0, 1, 0, 1], 3, 1, 2, 2, 2)
  assert pref.split_payload(p, 4) == [pref.encode_stream([[0], [0]], 2), pref.encode_stream([[1], [1]], 2),
                                      pref.encode_stream([[0]], 2), pref.encode_stream([[1]], 2)]
  # bytes past the end read as 0, the count is fixed, a value >= L is clipped to L - 1, reported, and seen by its neighbours
  assert pref.decode_stream(b'', 2, 3, 100) == ([[0] * 3] * 2, False)
  rows, clipped = pref.decode_stream(b'\xff' * 64, 5, 8, 100)
  assert len(rows) == 5 and clipped and max(max(r) for r in rows) == 99 and min(min(r) for r in rows) >= 0


def test_the_inputs_exercise_carry_propagation():
  total = cases.carry_counters()
  print('carries %d, longest pending run %d, carries into a run >= 2: %d' % (total.carries, total.longest_run,
                                                                         total.carries_into_run2))
  assert total.carries_into_run2 >= 1 and total.longest_run >= 2 and total.carries >= 100


def test_size_conditions_between_the_two_reference_coders():
  """At the workload's code (32, 64, 16, 64, 8), 32768 indices, against the order-0 coder of 4.14 in 64 streams; device
  payloads are byte-identical to the references' (tests/test_hip_vq_plane.py, tests/test_hip_vq_coder.py), so both hold for
  the device coders.
  1. correlated source: the context payload is smaller than the order-0 payload of the same indices (measured: 10807 against
     24524 bytes; packed 24576).
  2. uniform source: the context payload is larger by no more than the margin.  Measured with the two reference coders:
     26020 against 25271 bytes, an excess of 749 (the two flags, 2 * log2(64 / 63) bits per symbol = 186 bytes; 128 streams
     against 64, each with its table entry, flush and adaptation).  Margin = 749 + 749 // 4 = 936 bytes."""
  h, w, G, L, strip_rows = cases.WORKLOAD
  sizes = {}
  for kind in ('correlated', 'uniform'):
    v = cases.indices(cases.WORKLOAD, kind).tolist()
    sizes[kind] = (len(pref.encode(v, *cases.WORKLOAD)), len(vref.encode(v, L, cases.ORDER0_STREAMS)))
    print('%s: context %d bytes, order 0 %d bytes, packed %d' % ((kind,) + sizes[kind] + (h * w * G * 6 // 8,)))
  assert sizes['correlated'][0] < sizes['correlated'][1]
  assert sizes['uniform'][0] - sizes['uniform'][1] <= 936


# ---- the container --------------------------------------------------------------------------------------------------------------
BLOB_SHAPE = (16, 8, 5, 100, 3)               # 6 strips x 5 groups = 30 streams


def _blob():
  from ctu.utils import vqplane
  v, payload, _ = cases.reference(BLOB_SHAPE, 'correlated')
  blob = vqplane.build_blob(BLOB_SHAPE[:3], 100, 3, payload)
  assert struct.unpack_from('<4sIIIIIII', blob) == (b'JPDW', 1, 16, 8, 5, 100, 3, 1) and blob[32:] == payload
  return blob, v


def _word(v):
  return struct.pack('<I', v)


def _patched(blob, field, value):
  """The blob with header word `field` (0 = magic) replaced."""
  return blob[:4 * field] + _word(value) + blob[4 * field + 4:]


def test_container_round_trip_on_the_host():
  from ctu.utils import vqplane
  blob, v = _blob()
  h, w, G, L, strip_rows, body = vqplane.parse_blob(blob)
  assert (h, w, G, L, strip_rows) == BLOB_SHAPE and body == cases.reference(BLOB_SHAPE, 'correlated')[1]
  assert pref.decode(body, *BLOB_SHAPE) == v.tolist()
  assert vqplane.coded_bits(blob) == 8 * len(blob) == 8 * (32 + len(body))


def _refused(blob, match):
  from ctu.utils import vqplane
  touched = lambda *a, **k: (_ for _ in ()).throw(AssertionError('device call'))
  saved = vqplane.ops.vq_plane_decode
  vqplane.ops.vq_plane_decode = touched
  try:
    with pytest.raises(ValueError, match=match):
      vqplane.read_planes(blob, 'cpu')
    with pytest.raises(ValueError, match=match):
      vqplane.parse_blob(blob)
  finally:
    vqplane.ops.vq_plane_decode = saved


def test_reader_refuses_a_wrong_magic():
  _refused(b'JPDV' + _blob()[0][4:], 'magic')


def test_reader_refuses_an_unknown_version():
  _refused(_patched(_blob()[0], 1, 2), 'version')


def test_reader_refuses_an_unknown_mode():
  for mode in (0, 2):
    _refused(_patched(_blob()[0], 7, mode), 'unknown mode')


def test_reader_refuses_fields_out_of_range():
  blob = _blob()[0]
  for L in (0, 1, 513, 1 << 31):
    _refused(_patched(blob, 5, L), 'L = ')
  _refused(_patched(blob, 6, 0), 'strip_rows')
  _refused(_patched(_patched(blob, 2, 70000), 6, 1), 'streams')          # 70000 strips of 5 groups
  _refused(_patched(blob, 3, 1 << 30), 'limits')


def test_reader_refuses_an_empty_shape():
  blob = _blob()[0]
  for field in (2, 3, 4):
    _refused(_patched(blob, field, 0), 'empty plane shape')


def test_reader_refuses_truncated_data():
  blob = _blob()[0]
  _refused(blob[:31], 'header')
  _refused(blob[:32 + 4 * 30 - 1], 'truncated')                      # the blob ends inside the length table
  _refused(blob[:-1], 'length table sums to')
  # another strip height is another stream count: the table no longer adds up
  _refused(_patched(blob, 6, 4), 'length table sums to')


def test_reader_refuses_trailing_bytes():
  _refused(_blob()[0] + b'\0', 'length table sums to')


def test_reader_refuses_a_length_table_that_does_not_add_up():
  blob = _blob()[0]
  first = struct.unpack_from('<I', blob, 32)[0]
  _refused(blob[:32] + _word(first + 1) + blob[36:], 'length table sums to')
  _refused(blob[:32] + _word(0xFFFFFFFF) + blob[36:], 'length table sums to')


def test_reader_refuses_what_is_not_bytes():
  from ctu.utils import vqplane
  with pytest.raises(ValueError, match='bytes'):
    vqplane.parse_blob(np.frombuffer(_blob()[0], dtype=np.uint8))


def test_writer_refuses_what_the_reader_would():
  from ctu.utils import vqplane
  payload = cases.reference(BLOB_SHAPE, 'correlated')[1]
  with pytest.raises(ValueError, match='length table sums to'):
    vqplane.build_blob((16, 8, 5), 100, 3, payload[:-1])
  with pytest.raises(ValueError, match='bytes'):
    vqplane.build_blob((16, 8, 5), 100, 3, np.frombuffer(payload, dtype=np.uint8))
  with pytest.raises(ValueError, match='empty plane shape'):
    vqplane.build_blob((0, 8, 5), 100, 3, payload)
  with pytest.raises(ValueError, match='L = 513'):
    vqplane.build_blob((16, 8, 5), 513, 3, payload)
  with pytest.raises(ValueError, match='strip_rows'):
    vqplane.build_blob((16, 8, 5), 100, 0, payload)
  with pytest.raises(ValueError, match='int64'):
    vqplane.write_planes(None, torch.zeros(16, dtype=torch.int32), (4, 4, 1), 64)
  with pytest.raises(ValueError, match='17 indices'):
    vqplane.write_planes(None, torch.zeros(17, dtype=torch.int64), (4, 4, 1), 64)
  with pytest.raises(ValueError, match='outside'):
    vqplane.write_planes(None, torch.full((16,), 64, dtype=torch.int64), (4, 4, 1), 64)


def test_surface():
  from ctu.utils import vqplane
  from jpdse_hip import ops, streams
  assert vqplane.MAGIC == b'JPDW' and vqplane.VERSION == 1 and vqplane.SUFFIX == '.jpdw' and vqplane.HEADER_BYTES == 32
  assert list(inspect.signature(vqplane.write_planes).parameters) == ['path', 'code', 'shape', 'n_center', 'strip_rows']
  assert inspect.signature(vqplane.write_planes).parameters['strip_rows'].default == 8
  assert list(inspect.signature(vqplane.read_planes).parameters) == ['blob_or_path', 'device']
  assert list(inspect.signature(vqplane.coded_bits).parameters) == ['blob']
  assert list(inspect.signature(ops.vq_plane_encode).parameters) == ['index', 'h', 'w', 'G', 'L', 'strip_rows']
  assert list(inspect.signature(ops.vq_plane_decode).parameters) == ['payload', 'h', 'w', 'G', 'L', 'strip_rows', 'device']
  assert ops.vq_plane_encode is streams.vq_plane_encode and ops.vq_plane_decode is streams.vq_plane_decode
  assert inspect.signature(ops.vq_plane_encode).parameters['strip_rows'].default == 8


def test_ops_decode_refuses_bad_payloads_without_the_library(monkeypatch):
  import jpdse_hip.ops as ops
  touched = lambda: (_ for _ in ()).throw(AssertionError('library touched'))
  monkeypatch.setattr(jpdse_hip, 'lib', touched)
  monkeypatch.setattr(ops, 'lib', touched)
  monkeypatch.setattr(jpdse_hip.streams, 'lib', touched)
  good = cases.reference(BLOB_SHAPE, 'uniform')[1]
  bump = bytearray(good)
  bump[0] ^= 1
  for bad in (good[:-1], good + b'\0', bytes(bump), good[:4 * 30 - 1], b'', None, np.frombuffer(good, dtype=np.uint8), 'text'):
    with pytest.raises(ValueError, match='vq_plane_decode'):
      ops.vq_plane_decode(bad, *BLOB_SHAPE)
  for kw in (dict(L=1), dict(L=513), dict(h=0), dict(w=0), dict(G=0), dict(strip_rows=0), dict(h=70000, strip_rows=1),
             dict(w=1 << 28)):
    a = dict(zip(('h', 'w', 'G', 'L', 'strip_rows'), BLOB_SHAPE))
    a.update(kw)
    with pytest.raises(ValueError, match='vq_plane_decode'):
      ops.vq_plane_decode(good, **a)


# ---- the ABI --------------------------------------------------------------------------------------------------------------------
NAMES = ('jpdse_vq_plane_capacity', 'jpdse_vq_plane_workspace_size', 'jpdse_vq_plane_encode', 'jpdse_vq_plane_decode')


def test_entry_points_are_declared_and_exported():
  header = open(os.path.join(ROOT, 'include', 'jpdse.h')).read()
  declared = set(re.findall(r'\b(jpdse_[a-zA-Z0-9_]+)\s*\(', header))
  L, dev = jpdse_hip.lib(), ctypes.CDLL(jpdse_hip.DEV_LIB_PATH)
  for name in NAMES:
    assert name in declared and name in jpdse_hip.SIGNATURES and hasattr(L, name) and hasattr(dev, name), name
  assert declared == set(jpdse_hip.SIGNATURES.keys())
  for cname, cls in (('jpdse_vq_plane_encode_args', VqPlaneEncodeArgs), ('jpdse_vq_plane_decode_args', VqPlaneDecodeArgs)):
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (cname, cname), header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = re.findall(r'(\w+)\s*[,;]', body)
    assert names == [f[0].rstrip('_') for f in cls._fields_], (names, cls._fields_)
  assert L.jpdse_version() == 2


def test_host_queries_against_the_closed_forms():
  L = jpdse_hip.lib()
  cap, ws = L.jpdse_vq_plane_capacity, L.jpdse_vq_plane_workspace_size
  for shape in cases.SHAPES + [cases.WORKLOAD, (32, 64, 16, 64, 4), (32, 64, 16, 64, 32), (4096, 16, 15, 512, 1),
                               (1024, 1024, 64, 2, 1024)]:
    h, w, G, n_center, strip_rows = shape
    nb, S = pref.index_bits(n_center), pref.strips(h, strip_rows) * G
    assert cap(*shape) == pref.capacity(*shape) == (nb + 2) * h * w * G + 12 * S, shape
    assert ws(*shape) == ((nb + 2) * h * w * G + 8 * S + 15) // 16 * 16 + 8 * S, shape
  # outside the limits: 0, never a wrapped size
  for shape in ((0, 8, 1, 64, 8), (-1, 8, 1, 64, 8), (8, 0, 1, 64, 8), (8, 8, 0, 64, 8), (8, 8, -3, 64, 8), (8, 8, 1, 1, 8),
                (8, 8, 1, 513, 8), (8, 8, 1, 0, 8), (8, 8, 1, 64, 0), (8, 8, 1, 64, -1), (65536, 1, 1, 64, 1), (4096, 1, 16, 64, 1),
                (1 << 16, 1 << 16, 1, 64, 1 << 16), (1 << 15, 1 << 15, 2, 2, 1 << 15), (1 << 14, 1 << 14, 1, 512, 1 << 14),
                ((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1, 2, (1 << 31) - 1)):
    assert cap(*shape) == 0 and ws(*shape) == 0, shape
  assert cap(65535, 1, 1, 2, 1) == 65535 * 15 and cap(8, 8, 1, 64, 100) == 8 * 64 + 12


def test_bad_arguments_are_refused_before_any_launch():
  """No device exists here: a call that got as far as a launch could not return JPDSE_EINVAL."""
  lb = jpdse_hip.lib()
  P = 4096                                 # never dereferenced: every call below is refused on its arguments
  shape = dict(zip(('h', 'w', 'G', 'L', 'strip_rows'), BLOB_SHAPE))
  cap, ws = lb.jpdse_vq_plane_capacity(*BLOB_SHAPE), lb.jpdse_vq_plane_workspace_size(*BLOB_SHAPE)

  def enc(index=P, out=P, out_bytes=cap, size=P, status=P, wsp=P, ws_bytes=ws, **kw):
    a = dict(shape)
    a.update(kw)
    return lb.jpdse_vq_plane_encode(ctypes.byref(VqPlaneEncodeArgs(a['h'], a['w'], a['G'], a['L'], a['strip_rows'], index, out,
                                                                   out_bytes, size, status, wsp, ws_bytes, None)))

  def dec(src=P, in_bytes=cap, index=P, status=P, **kw):
    a = dict(shape)
    a.update(kw)
    return lb.jpdse_vq_plane_decode(ctypes.byref(VqPlaneDecodeArgs(a['h'], a['w'], a['G'], a['L'], a['strip_rows'], src, in_bytes,
                                                                   index, status, None)))
  null = 'null pointer'
  limits = [(dict(L=1), 'n_center L = 1'), (dict(L=513), 'n_center L = 513'), (dict(h=0), 'h = 0'), (dict(w=-2), 'w = -2'),
            (dict(G=0), 'G = 0'), (dict(strip_rows=0), 'strip_rows = 0'), (dict(h=70000, strip_rows=1), 'S = 350000 streams'),
            (dict(h=1 << 15, w=1 << 15, strip_rows=1 << 15), 'below 2^31'), (dict(h=1 << 14, w=1 << 14, G=1, strip_rows=1 << 14), 'below 2^31')]      # 2^28 indices of 9 bytes
  for who, call, cases_ in (
      ('vq_plane_encode', enc, limits + [(dict(index=None), null), (dict(out=None), null), (dict(size=None), null),
                                         (dict(status=None), null), (dict(out_bytes=cap - 1), 'below the payload capacity'),
                                         (dict(wsp=None), 'workspace too small'), (dict(ws_bytes=ws - 1), 'workspace too small')]),
      ('vq_plane_decode', dec, limits + [(dict(src=None), null), (dict(index=None), null), (dict(status=None), null),
                                         (dict(in_bytes=4 * 30 - 1), 'length table'), (dict(in_bytes=-1), 'length table'),
                                         (dict(in_bytes=1 << 31), '2^31')])):
    for kw, want in cases_:
      lb.jpdse_code_export(7, 0, 0, 0, 0, None, 0, None, None)      # leaves another call's message behind
      assert call(**kw) == -1, (who, kw)                            # JPDSE_EINVAL
      msg = jpdse_hip.last_error()
      assert msg.startswith(who + ': ') and want in msg, (who, kw, msg)
  for fn, name in ((lb.jpdse_vq_plane_encode, 'vq_plane_encode'), (lb.jpdse_vq_plane_decode, 'vq_plane_decode')):
    assert fn(None) == -1 and jpdse_hip.last_error().startswith(name + ': null argument struct')
  with pytest.raises(jpdse_hip.JpdseError):
    jpdse_hip.check(enc(strip_rows=0), 'vq_plane_encode')


# ---- the model's flag and the receiver's dispatch -----------------------------------------------------------------------------
def test_flag_parses_and_defaults_to_off():
  from ctu.models import get_option_setter
  parser = argparse.ArgumentParser()
  get_option_setter('pix2pixHD')(parser, True)
  assert parser.parse_args([]).vq_context_coder is False
  assert parser.parse_args(['--encoder_quantizer', 's2hvq', '--vq_context_coder']).vq_context_coder is True


@pytest.mark.parametrize('over', [dict(encoder_quantizer='binarizer'), dict(encoder_quantizer='binarizer', no_feat_encoding=True)],
                         ids=str)
def test_model_constructor_refuses_the_flag_without_s2hvq(over, monkeypatch):
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  _hide_device(monkeypatch)
  with pytest.raises(ValueError, match='vq_context_coder'):
    Pix2PixHDModel(_codec_opts(vq_context_coder=True, **over))


def test_model_constructor_passes_its_checks_with_the_flag(monkeypatch):
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  with pytest.raises(jpdse_hip.JpdseError, match='no GPU visible'):
    Pix2PixHDModel(_codec_opts(vq_context_coder=True))


def _bare_codec():
  """VQIndexCodec on a stand-in encoder: 64 x 32 images, two down-samplings, 16 channels in vectors of 4, 8 centres -- planes
  of 16 x 8 x 4 indices."""
  from ctu.models.codec import VQIndexCodec
  vq = types.SimpleNamespace(n_center=8, cout=16, center_size=4)
  netE = types.SimpleNamespace(n_downsampling=2, _vq=vq, vq_code_len=lambda H, W: (H >> 2) * (W >> 2) * 4)
  return VQIndexCodec(netE, 0)


def test_receiver_tells_the_containers_by_their_magic(monkeypatch):
  """Hand-built blobs of both kinds, reference payloads inside; no flag is set on the codec.  check_payloads verifies each
  header against the label map and the code book on the host; features_of_payloads routes each blob to its own reader."""
  from ctu.utils import vqplane, vqstream
  codec = _bare_codec()
  assert codec.context_coder is False
  shape, code_len = (16, 8, 4, 8, 8), 16 * 8 * 4
  v = cases.indices(shape, 'correlated')
  plane = vqplane.build_blob(shape[:3], 8, 8, pref.encode(v.tolist(), *shape))
  flat = vqstream.build_blob((1, code_len), 8, 32, vref.encode(v.tolist(), 8, 32), v)
  assert plane[:4] == b'JPDW' and flat[:4] == b'JPDV'
  xd = {'label': torch.zeros(2, 1, 64, 32)}
  geo = codec.check_payloads([plane, flat], xd, 'decode_coded')
  assert geo == (2, 64, 32, code_len, 8, 4)
  assert codec.check_payloads([flat, bytearray(plane)], xd, 'decode_coded') == geo
  # the .jpdw header against the geometry and the code book, in the .jpdv messages' style
  with pytest.raises(ValueError, match='blob 1 was coded for n_center 16, the code book has 8'):
    codec.check_payloads([flat, vqplane.build_blob(shape[:3], 16, 8, pref.encode(v.tolist(), 16, 8, 4, 16, 8))], xd, 'decode_coded')
  other = cases.indices((8, 16, 4, 8, 8), 'correlated')
  with pytest.raises(ValueError, match='blob 0 holds planes of 8 x 16 x 4 indices, a 64 x 32 label map carries 16 x 8 x 4'):
    codec.check_payloads([vqplane.build_blob((8, 16, 4), 8, 8, pref.encode(other.tolist(), 8, 16, 4, 8, 8)), flat], xd, 'decode_coded')
  with pytest.raises(ValueError, match='decode_coded: blob 0: the length table sums to'):
    codec.check_payloads([plane[:-1], flat], xd, 'decode_coded')
  with pytest.raises(ValueError, match='not a coded index file'):
    codec.check_payloads([b'JPDX' + plane[4:], flat], xd, 'decode_coded')
  # the readers: each blob goes to its own, and the rows come back in order
  seen = []
  monkeypatch.setattr(vqplane, 'read_planes', lambda b, dev: (seen.append(('jpdw', b[:4])), (torch.from_numpy(v.astype(np.int64)), shape[:3], 8))[1])
  monkeypatch.setattr(vqstream, 'read_indices', lambda b, dev: (seen.append(('jpdv', b[:4])), torch.from_numpy(v.astype(np.int64)).view(1, -1))[1])
  got = {}
  monkeypatch.setattr(codec, 'features_of_code', lambda code, geo_, device, who: got.setdefault('code', code))
  codec.features_of_payloads([plane, flat, bytearray(plane)], geo, lambda: 'cpu', 'decode_coded')
  assert seen == [('jpdw', b'JPDW'), ('jpdv', b'JPDV'), ('jpdw', b'JPDW')]
  assert tuple(got['code'].shape) == (3, code_len) and got['code'][2].tolist() == v.tolist()


def test_payloads_keep_the_smaller_blob_and_the_jpdv_one_on_a_tie(monkeypatch):
  from ctu.utils import vqplane, vqstream
  codec = _bare_codec()
  xd = {'label': torch.zeros(3, 1, 64, 32)}
  code = torch.zeros(3, 16 * 8 * 4, dtype=torch.int64)
  plane_sizes, calls = [39, 40, 41], []

  def write_indices(path, c, L, n_streams):
    calls.append('v')
    return b'V' * 40

  def write_planes(path, c, shape, L):
    calls.append(('w', shape, L))
    return b'W' * plane_sizes[len(calls) - 4]                        # the three .jpdv blobs are made first

  monkeypatch.setattr(vqstream, 'write_indices', write_indices)
  monkeypatch.setattr(vqplane, 'write_planes', write_planes)
  assert [len(b) for b in codec.payloads(code, xd)] == [40, 40, 40] and calls == ['v'] * 3      # flag off: no .jpdw is made
  del calls[:]
  codec.context_coder = True
  blobs = codec.payloads(code, xd)
  assert [b[:1] for b in blobs] == [b'W', b'V', b'V'] and [len(b) for b in blobs] == [39, 40, 40]
  assert calls == ['v'] * 3 + [('w', (16, 8, 4), 8)] * 3
  assert codec.file_rates(blobs, 64, 32)[0] == sum(8.0 * len(b) / (64 * 32) for b in blobs) / 3
