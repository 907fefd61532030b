"""Coded label and instance maps, host only (no GPU): the pure-Python coder tests/semantics_ref.py (written from DESIGN.md
4.9) inverts itself on every shape and input kind of the GPU tests; the .jpds container (ctu.utils.semantics) round-trips,
refuses malformed files and is never larger than the raw file; the recorded Cityscapes pair decodes to itself and its
coded size is the figure 4.9 records; the four C entry points are declared, exported, answer their host queries by the
formula of 4.9 and refuse bad arguments before any launch."""
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

import semantics_cases as cases  # noqa: E402
import semantics_ref as sref  # noqa: E402

_shape = dict(argnames='shape', argvalues=cases.SHAPES, ids=cases.shape_id)
# DESIGN.md 4.9, "Measured sizes": the recorded 1024x512 pair at strip_rows 8, payload bytes of the label / instance plane
GOLDEN_CODED = (7448, 14150)


# ---- the yardstick ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize(**_shape)
def test_reference_round_trip(shape, kind):
  N, H, W, sr = shape
  label, inst, coded, _ = cases.reference(shape, kind)
  S = len(sref.strips(H, sr))
  for n in range(N):
    for plane, a in ((0, label), (1, inst)):
      payload, cut = coded[n][plane]
      streams = sref.split_payload(payload, S)
      caps = [sref.stream_capacity(plane, r, W) for _, r in sref.strips(H, sr)]
      assert all(len(s) <= c for s, c in zip(streams, caps)) and len(payload) <= sref.plane_capacity(plane, H, W, sr)
      assert cut == any(len(s) == c and len(sref.encode_stream(a[n, y0:y0 + r].reshape(-1).tolist(), r, W, plane)) > c
                        for s, c, (y0, r) in zip(streams, caps, sref.strips(H, sr)))
      if not cut:
        assert np.array_equal(sref.decode_plane(payload, plane, H, W, sr), a[n])
      mode, stored = sref.entry(a[n], plane, sr)
      assert mode == (0 if cut or len(payload) >= sref.raw_size(plane, H, W) else 1)
      assert stored == (payload if mode else sref.raw_plane(a[n], plane))


def test_reference_on_hand_checked_streams():
  """By hand from the format text.  One label pixel 0: no neighbour, so 8 literal bits 0 at p = 1024: bound =
  (range >> 11) << 10 halves the range eight times from 0xFFFFFFFF to 0x00FFFFF8 < 2^24: one normalisation (a shiftLow that
  emits the unstored first byte), low stays 0; the flush emits 0 five times: 5 stored bytes of 0."""
  assert sref.encode_stream([0], 1, 1, 0) == b'\0' * 5
  assert sref.decode_stream(b'\0' * 5, 1, 1, 0) == [0]
  # bytes past the end read as 0 and the pixel count is fixed whatever the bytes are
  assert sref.decode_stream(b'', 2, 3, 0) == [0] * 6 and len(sref.decode_stream(b'\xff' * 3, 2, 3, 1)) == 6
  # the second pixel of a row equal to the first is ONE decision (v == L, context 0), not a literal: both streams differ
  # only in that bit, and the unequal one carries a second literal
  same, other = sref.encode_stream([5, 5], 1, 2, 0), sref.encode_stream([5, 6], 1, 2, 0)
  assert sref.decode_stream(same, 1, 2, 0) == [5, 5] and sref.decode_stream(other, 1, 2, 0) == [5, 6]
  assert len(other) > len(same)
  # below the first row of a strip, a pixel equal to the upper one but not to the left one takes the second decision
  assert sref.decode_stream(sref.encode_stream([1, 2, 3, 2], 2, 2, 1), 2, 2, 1) == [1, 2, 3, 2]
  # a strip never looks above its first row: two strips of one row are two independent one-row streams
  a = np.array([[4, 4, 9], [4, 4, 9]])
  payload, cut = sref.encode_plane(a, 0, 1)
  one = sref.encode_stream([4, 4, 9], 1, 3, 0)
  assert not cut and payload == struct.pack('<II', len(one), len(one)) + one + one


def test_the_inputs_show_a_cut_stream_and_a_carry_through_pending_bytes():
  _, _, coded, _ = cases.reference(cases.CUT_SHAPE, cases.CUT_KIND)
  assert coded[0][0][1] and coded[0][1][1], 'the i.i.d. input was chosen so that streams outgrow their slots'
  _, _, carry_coded, c = cases.reference(cases.CARRY_SHAPE, cases.CARRY_KIND)
  assert not any(cut for image in carry_coded for _, cut in image), 'the carry must lie in bytes the device comparison covers'
  print('carries %d, longest pending run %d, carries into a run >= 2: %d' % (c.carries, c.longest_run, c.carries_into_run2))
  assert c.carries >= 100 and c.longest_run >= 2 and c.carries_into_run2 >= 1


# ---- the recorded map -----------------------------------------------------------------------------------------------------------
def test_golden_pair_decodes_to_itself_at_the_recorded_size():
  label, inst, coded = cases.golden()
  assert label.shape == (512, 1024) and label.dtype == np.uint8 and inst.shape == (512, 1024)
  assert os.path.getsize(cases.GOLDEN) < 100 * 1024
  sizes = tuple(len(p) for p, _ in coded)
  print('label / instance payload at strip_rows 8: %d / %d bytes (raw %d / %d)' % (sizes + (512 * 1024, 4 * 512 * 1024)))
  assert not coded[0][1] and not coded[1][1]
  assert sizes == GOLDEN_CODED                 # a determinism check: the figure of DESIGN.md 4.9, exactly
  assert np.array_equal(sref.decode_plane(coded[0][0], 0, 512, 1024, 8), label)
  assert np.array_equal(sref.decode_plane(coded[1][0], 1, 512, 1024, 8), inst)
  design = open(os.path.join(ROOT, 'DESIGN.md')).read()
  assert '| 8 | 7448 | 14150 |' in design


# ---- the container --------------------------------------------------------------------------------------------------------------
def _blob(shape, kind, n=0, mask=3):
  from ctu.utils import semantics
  _, H, W, sr = shape
  label, inst, _, _ = cases.reference(shape, kind)
  planes = [sref.entry(label[n], 0, sr), sref.entry(inst[n], 1, sr) if mask & 2 else None]
  return semantics.pack(H, W, sr, planes), planes


@pytest.mark.parametrize('mask', [1, 3], ids=['label', 'both'])
@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize(**_shape)
def test_jpds_round_trip_and_the_raw_bound(shape, kind, mask, tmp_path):
  from ctu.utils import semantics
  N, H, W, sr = shape
  for n in range(N):
    blob, planes = _blob(shape, kind, n, mask)
    assert blob[:4] == b'JPDS'
    assert struct.unpack('<IIIIIII', blob[4:32]) == (1, H, W, sr, mask, planes[0][0], planes[1][0] if mask & 2 else 0)
    # the raw-fallback rule: never larger than the file that stores the same planes raw
    assert len(blob) <= semantics.raw_file_bytes(H, W, mask) == 32 + H * W * (1 + (4 if mask & 2 else 0))
    path = str(tmp_path / ('i%d%s' % (n, semantics.SUFFIX)))
    assert semantics.write(path, blob) == os.path.getsize(path) == len(blob)
    back = semantics.read(path)
    assert back == blob
    gH, gW, gsr, gmask, gplanes = semantics.unpack(back)
    assert (gH, gW, gsr, gmask) == (H, W, sr, mask) and gplanes == [tuple(p) if p else None for p in planes]


def test_both_modes_occur_and_pack_refuses_a_coded_plane_that_does_not_pay():
  from ctu.utils import semantics
  modes = {p[0] for s in cases.SHAPES for k in cases.KINDS for p in _blob(s, k)[1]}
  assert modes == {0, 1}
  N, H, W, sr = cases.CUT_SHAPE
  label, _, coded, _ = cases.reference(cases.CUT_SHAPE, cases.CUT_KIND)
  assert len(coded[0][0][0]) >= H * W
  with pytest.raises(ValueError, match='store it raw'):
    semantics.pack(H, W, sr, [(1, coded[0][0][0]), None])


def test_jpds_reader_refuses_malformed_files(tmp_path):
  from ctu.utils import semantics
  shape = (3, 19, 33, 8)
  coded, cplanes = _blob(shape, 'rects')
  raw, rplanes = _blob(shape, 'iid19', 1)
  assert [p[0] for p in cplanes] == [1, 1] and [p[0] for p in rplanes] == [0, 0]
  S = 3

  def refused(name, data, match):
    path = str(tmp_path / name)
    with open(path, 'wb') as fh:
      fh.write(data)
    with pytest.raises(ValueError, match=match):
      semantics.read(path)
    with pytest.raises(ValueError, match=match):
      semantics.unpack(data)
  word = lambda v: struct.pack('<I', v)
  for tag, b in (('c', coded), ('r', raw)):
    refused(tag + 'magic', b'JPDA' + b[4:], 'magic')
    refused(tag + 'version', b[:4] + word(2) + b[8:], 'version')
    refused(tag + 'emptyH', b[:8] + word(0) + b[12:], 'empty map shape')
    refused(tag + 'emptyW', b[:12] + word(0) + b[16:], 'empty map shape')
    refused(tag + 'strip', b[:16] + word(0) + b[20:], 'strip_rows 0')
    refused(tag + 'mask0', b[:20] + word(0) + b[24:], 'unknown plane mask 0')
    refused(tag + 'mask2', b[:20] + word(2) + b[24:], 'unknown plane mask 2')
    refused(tag + 'mask4', b[:20] + word(4) + b[24:], 'unknown plane mask 4')
    refused(tag + 'mode0', b[:24] + word(2) + b[28:], 'unknown mode')
    refused(tag + 'mode1', b[:28] + word(7) + b[32:], 'unknown mode')
    refused(tag + 'header', b[:31], 'header')
    refused(tag + 'short', b[:-1], 'truncated')
    refused(tag + 'long', b + b'\0', 'trailing')
  refused('absentmode', coded[:20] + word(1) + coded[24:28] + word(1) + coded[32:32 + len(cplanes[0][1])], 'unknown mode')
  refused('ctable', coded[:32 + 4 * S - 1], 'truncated')                          # the file ends inside the length table
  first = struct.unpack('<I', coded[32:36])[0]
  refused('csum+', coded[:32] + word(first + 1) + coded[36:], 'truncated|trailing|length table')   # a table that does not add up
  refused('csum-', coded[:32] + word(first - 1) + coded[36:], 'truncated|trailing|length table')
  refused('chuge', coded[:32] + word(0xFFFFFFFF) + coded[36:], 'length table sums to')
  with pytest.raises(ValueError, match='bytes'):
    semantics.unpack(np.frombuffer(coded, dtype=np.uint8))
  # the writer refuses what the reader would
  with pytest.raises(ValueError, match='truncated'):
    semantics.write(str(tmp_path / 'w'), coded[:-1])
  with pytest.raises(ValueError, match='length table sums to'):
    semantics.pack(19, 33, 8, [(1, cplanes[0][1][:-1]), None])
  with pytest.raises(ValueError, match='raw plane'):
    semantics.pack(19, 33, 8, [(0, rplanes[0][1][:-1]), None])
  with pytest.raises(ValueError, match='unknown mode'):
    semantics.pack(19, 33, 8, [(2, rplanes[0][1]), None])
  with pytest.raises(ValueError, match='strip_rows'):
    semantics.pack(19, 33, 0, [rplanes[0], None])
  with pytest.raises(ValueError, match='shape'):
    semantics.pack(0, 33, 8, [rplanes[0], None])


def test_the_other_containers_are_untouched():
  from ctu.utils import bitstream, entropy, semantics
  assert (bitstream.MAGIC, bitstream.VERSION, bitstream.HEADER_BYTES) == (b'JPDC', 1, 20)
  assert (entropy.MAGIC, entropy.VERSION, entropy.HEADER_BYTES, entropy.SUFFIX) == (b'JPDA', 1, 24, '.jpda')
  assert (semantics.MAGIC, semantics.VERSION, semantics.HEADER_BYTES, semantics.SUFFIX) == (b'JPDS', 1, 32, '.jpds')


# ---- the ABI --------------------------------------------------------------------------------------------------------------------
NAMES = ('jpdse_semantics_capacity', 'jpdse_semantics_workspace_size', 'jpdse_semantics_encode', 'jpdse_semantics_decode')


def test_entry_points_are_declared_and_exported_under_version_2():
  header = open(os.path.join(ROOT, 'include', 'jpdse.h')).read()
  declared = set(re.findall(r'\b(jpdse_[a-zA-Z0-9_]+)\s*\(', header))
  L, dev = jpdse_hip.lib(), ctypes.CDLL(jpdse_hip.DEV_LIB_PATH)
  for name in NAMES:
    assert name in declared and name in jpdse_hip.SIGNATURES and hasattr(L, name) and hasattr(dev, name), name
    args = re.search(r'\b%s\s*\(([^)]*)\)\s*;' % name, header).group(1)
    assert len(args.split(',')) == len(jpdse_hip.SIGNATURES[name][1]), name
  assert declared == set(jpdse_hip.SIGNATURES.keys())
  for name in NAMES[2:]:
    assert re.search(r'\b%s\s*\([^)]*void\*\s*/\* hipStream_t \*/\s*stream\)\s*;' % name, header), name
  assert L.jpdse_version() == 2 and re.search(r'#define\s+JPDSE_ABI_VERSION\s+2\b', header)
  assert 'semantics' in open(os.path.join(ROOT, 'jpd-se_amd', 'csrc', 'Makefile')).read()


def _formula(N, H, W, sr, mask):
  """capacity and workspace."""
  S = -(-H // sr)
  up = lambda v: (v + 15) // 16 * 16
  cap = sum(H * W * raw + 12 * S for p, raw in ((0, 1), (1, 4)) if mask >> p & 1)
  ws = up(8 * N * S) + sum(up(N * S * (min(sr, H) * W * raw + 8)) + up(4 * N * S) for p, raw in ((0, 1), (1, 4)) if mask >> p & 1)
  return cap, ws


def test_host_queries_equal_the_formula():
  L = jpdse_hip.lib()
  cap, ws = L.jpdse_semantics_capacity, L.jpdse_semantics_workspace_size
  for N, H, W, sr in cases.SHAPES + [(4, 512, 1024, 8), (2, 512, 1024, 1000)]:
    for mask in (1, 2, 3):
      want = _formula(N, H, W, sr, mask)
      assert (cap(H, W, sr, mask), ws(N, H, W, sr, mask)) == want, (N, H, W, sr, mask)
      if mask & 1:
        assert sref.plane_capacity(0, H, W, sr) == _formula(N, H, W, sr, 1)[0]
      if mask & 2:
        assert sref.plane_capacity(1, H, W, sr) == _formula(N, H, W, sr, 2)[0]
  # outside the limits: 0, never a wrapped size
  for H, W, sr, mask in ((0, 8, 8, 3), (4, 0, 8, 3), (4, 8, 0, 3), (-1, 8, 8, 1), (4, 8, -2, 1), (4, 8, 8, 0), (4, 8, 8, 4),
                         (65536, 4, 1, 1), (1 << 15, 1 << 15, 8, 3), (1 << 14, 1 << 15, 8, 2), (1 << 20, 1 << 11, 64, 1)):
    assert cap(H, W, sr, mask) == 0 and ws(1, H, W, sr, mask) == 0, (H, W, sr, mask)
  assert cap(65535, 4, 1, 1) == 65535 * 4 + 12 * 65535 and cap(65536, 4, 2, 1) > 0
  assert ws(0, 4, 8, 8, 3) == 0 and ws(65536, 4, 8, 8, 3) == 0 and ws(65535, 1, 1, 8, 1) > 0


def test_bad_arguments_are_refused_before_any_launch():
  """No device exists here: a call that got as far as a launch could not return JPDSE_EINVAL."""
  L = jpdse_hip.lib()
  P = ctypes.c_void_p(4096)            # never dereferenced: every call below is refused on its arguments
  N, H, W, sr, mask = 2, 19, 33, 8, 3
  S = 3
  cap, ws = L.jpdse_semantics_capacity(H, W, sr, mask), L.jpdse_semantics_workspace_size(N, H, W, sr, mask)

  def enc(N=N, H=H, W=W, sr=sr, mask=mask, label=P, inst=P, out=P, stride=cap, sizes=P, status=P, wsp=P, ws_bytes=ws):
    return L.jpdse_semantics_encode(N, H, W, sr, mask, label, inst, out, stride, sizes, status, wsp, ws_bytes, None)

  def dec(N=N, H=H, W=W, sr=sr, mask=mask, num_labels=19, src=P, stride=cap, off=4 * S, sizes=P, label=P, inst=P, bad=P):
    return L.jpdse_semantics_decode(N, H, W, sr, mask, num_labels, src, stride, off, sizes, label, inst, bad, None)
  null, extent, limits = 'null pointer', 'non-positive extent', 'beyond the coder\'s limits'
  for who, call, cases_ in (
      ('semantics_encode', enc, [(dict(out=None), null), (dict(sizes=None), null), (dict(status=None), null),
                                 (dict(label=None), 'label is NULL'), (dict(inst=None), 'inst is NULL'),
                                 (dict(N=0), extent), (dict(H=-1), extent), (dict(W=0), extent),
                                 (dict(sr=0), 'non-positive strip_rows'), (dict(sr=-8), 'non-positive strip_rows'),
                                 (dict(mask=0), 'plane mask 0'), (dict(mask=4), 'plane mask 4'), (dict(N=65536), limits),
                                 (dict(H=65536, sr=1), limits), (dict(H=1 << 15, W=1 << 15), limits),
                                 (dict(stride=cap - 1), 'below the payload capacity')]),
      ('semantics_decode', dec, [(dict(src=None), null), (dict(sizes=None), null), (dict(bad=None), null),
                                 (dict(label=None), 'label is NULL'), (dict(inst=None), 'inst is NULL'),
                                 (dict(N=0), extent), (dict(W=-3), extent), (dict(sr=0), 'non-positive strip_rows'),
                                 (dict(mask=0), 'plane mask 0'), (dict(mask=8), 'plane mask 8'), (dict(N=65536), limits),
                                 (dict(H=65536, sr=1), limits), (dict(num_labels=0), 'num_labels 0'),
                                 (dict(num_labels=257), 'num_labels 257'), (dict(off=4 * S - 1), 'length table'),
                                 (dict(off=cap - 4 * S + 1), 'length table'), (dict(stride=8 * S - 1), 'length table'),
                                 (dict(mask=1, stride=4 * S - 1), 'length table'),
                                 (dict(mask=2, stride=4 * S - 1), 'length table')])):
    for kw, want in cases_:
      L.jpdse_code_export(7, 0, 0, 0, 0, None, 0, None, None)      # leaves another call's message behind
      assert call(**kw) == -1, (who, kw)                            # JPDSE_EINVAL
      msg = jpdse_hip.last_error()
      assert msg.startswith(who + ': ') and want in msg, (who, kw, msg)
  # a plane the mask does not name needs no buffer: these get past the pointer checks and fail on the next one
  assert enc(mask=1, inst=None, stride=0) == -1 and 'below the payload capacity' in jpdse_hip.last_error()
  assert enc(mask=2, label=None, stride=0) == -1 and 'below the payload capacity' in jpdse_hip.last_error()
  for kw in (dict(wsp=None), dict(ws_bytes=ws - 1), dict(ws_bytes=0)):
    assert enc(**kw) == -2 and 'workspace too small' in jpdse_hip.last_error()      # JPDSE_EWORKSPACE
  with pytest.raises(jpdse_hip.JpdseError):
    jpdse_hip.check(enc(N=0), 'semantics_encode')


def test_ops_and_model_refuse_bad_input_without_the_library(monkeypatch):
  import torch
  import jpdse_hip.ops as ops
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  touched = lambda: (_ for _ in ()).throw(AssertionError('library touched'))
  monkeypatch.setattr(jpdse_hip, 'lib', touched)
  monkeypatch.setattr(ops, 'lib', touched)
  monkeypatch.setattr(jpdse_hip.streams, 'lib', touched)
  shape = (3, 19, 33, 8)
  _, H, W, sr = shape
  good = [list(_blob(shape, 'rects', n)[1]) for n in range(2)]
  lab, ins = good[0]
  bump = bytearray(lab[1])
  bump[0] ^= 1
  for bad in (None, [], good[0], [good[0], [lab]], [good[0], [None, ins]], [good[0], [lab, None]], [[(1, 'text'), ins]],
              [[(3, lab[1]), ins]], [[(1, bytes(bump)), ins]], [[(1, lab[1][:-1]), ins]], [[(1, lab[1] + b'\0'), ins]],
              [[(1, b'\0' * 11), ins]], [[(0, b'\0' * (H * W - 1)), ins]], [[lab, (0, b'\0' * (H * W))]]):
    with pytest.raises(ValueError, match='semantics_decode'):
      ops.semantics_decode(bad, H, W, sr, 19)
  # raw planes are checked on the host as well: a label outside the set, a negative instance id
  with pytest.raises(ValueError, match='holds label 200'):
    ops.semantics_decode([[(0, bytes([200]) * (H * W)), ins]], H, W, sr, 19)
  with pytest.raises(ValueError, match='negative'):
    ops.semantics_decode([[lab, (0, struct.pack('<i', -1) * (H * W))]], H, W, sr, 19)
  with pytest.raises(ValueError, match='num_labels'):
    ops.semantics_decode(good, H, W, sr, 257)
  for l, i, kw in ((torch.zeros(1, 1, 4, 4, dtype=torch.float64), None, {}), (torch.zeros(1, 4, 4), None, {}),
                   (torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4, dtype=torch.int32), {}),
                   (torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 5, dtype=torch.int64), {}),
                   (torch.zeros(1, 1, 4, 4), None, dict(strip_rows=0))):
    with pytest.raises(ValueError, match='semantics_encode'):
      ops.semantics_encode(l, i, **kw)
  # the model's receiver refuses malformed blobs before it needs a device (self is never used that far)
  blob = _blob(shape, 'rects')[0]
  for bad in (None, [], [blob[:-1]], [blob, _blob((2, 16, 33, 8), 'rects')[0]], [np.frombuffer(blob, dtype=np.uint8)]):
    with pytest.raises(ValueError, match='decode_semantics'):
      Pix2PixHDModel.decode_semantics(None, bad)


def test_trainer_and_model_have_the_semantics_calls():
  from jpdse_hip import ops
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  from ctu.trainers.pix2pixHD_trainer import Pix2PixHDTrainer
  for cls in (Pix2PixHDModel, Pix2PixHDTrainer):
    assert list(inspect.signature(cls.get_coded_semantics).parameters)[:2] == ['self', 'x_dict']
    assert list(inspect.signature(cls.decode_semantics).parameters) == ['self', 'blobs']
    assert list(inspect.signature(cls.decode_from_files).parameters) == ['self', 'coded_payloads', 'semantics_blobs']
    assert list(inspect.signature(cls.get_total_rate).parameters)[:2] == ['self', 'x_dict']
    # the calls of 4.8 keep their signatures
    assert list(inspect.signature(cls.get_coded).parameters) == ['self', 'x_dict']
    assert list(inspect.signature(cls.decode_coded).parameters) == ['self', 'payloads', 'x_dict']
  sig = inspect.signature(ops.semantics_encode)
  assert list(sig.parameters) == ['label', 'inst', 'strip_rows'] and sig.parameters['strip_rows'].default == 8
  assert inspect.signature(Pix2PixHDModel.get_coded_semantics).parameters['strip_rows'].default == 8
