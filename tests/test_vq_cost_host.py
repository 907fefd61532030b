"""Code-length maps of the two S2HVQ index coders, host side (no GPU): the entry points in the header, the
library and the ctypes table; the host-only size queries; every refusal answered before any launch; the Python restatement
(tests/vq_cost_ref.py) -- its decision sequence is the reference coders' own, its sum identities, and the per-stream bound
between the model's code length and the bytes the Python CODERS write, on the case lists of tests/vq_coder_cases.py and
tests/vq_plane_cases.py; the `coder=` validation and the refusals of the two new trainer calls on a bare model; and the two
binarizer calls still refusing s2hvq with their pinned text."""
import ctypes
import json
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
from jpdse_hip import VqIndexCostArgs, VqPlaneCostArgs  # noqa: E402
import vq_coder_cases as icases  # noqa: E402
import vq_plane_cases as pcases  # noqa: E402
import vq_coder_ref as vref  # noqa: E402
import vq_plane_ref as pref  # noqa: E402
import vq_cost_ref as cref  # noqa: E402

NAMES = ('jpdse_vq_index_cost_workspace_size', 'jpdse_vq_index_cost', 'jpdse_vq_plane_cost_workspace_size', 'jpdse_vq_plane_cost')
TABLE_BYTES = (2049 * 4 + 255) // 256 * 256


# ---- the ABI ----------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_exported_under_version_2():
  header = open(os.path.join(ROOT, 'include', 'jpdse.h')).read()
  declared = set(re.findall(r'\b(jpdse_[a-zA-Z0-9_]+)\s*\(', header))
  L, dev = jpdse_hip.lib(), ctypes.CDLL(jpdse_hip.DEV_LIB_PATH)
  for name in NAMES:
    assert name in declared and name in jpdse_hip.SIGNATURES and hasattr(L, name) and hasattr(dev, name), name
  assert declared == set(jpdse_hip.SIGNATURES.keys())
  for cname, cls in (('jpdse_vq_index_cost_args', VqIndexCostArgs), ('jpdse_vq_plane_cost_args', VqPlaneCostArgs)):
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (cname, cname), header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = re.findall(r'(\w+)\s*[,;]', body)
    assert names == [f[0] for f in cls._fields_], (names, cls._fields_)
  assert L.jpdse_version() == 2


def test_size_queries_are_host_only_zero_outside_the_limits_and_monotone_inside():
  L = jpdse_hip.lib()
  iq, pq = L.jpdse_vq_index_cost_workspace_size, L.jpdse_vq_plane_cost_workspace_size
  # the table and one uint32 per symbol
  for M, n_center, S in icases.SHAPES:
    for G in (1, 4):
      if M % G == 0:
        assert iq(M, n_center, S, G, 0) == iq(M, n_center, S, G, 19) == TABLE_BYTES + 4 * M, (M, n_center, S, G)
  for shape in pcases.SHAPES + [pcases.WORKLOAD]:
    h, w, G, n_center, rows = shape
    assert pq(h, w, G, n_center, rows, 0) == pq(h, w, G, n_center, rows, 256) == TABLE_BYTES + 4 * h * w * G, shape
  # outside the limits of the matching encode call, of the groups, of the classes: 0, never a wrapped size
  for a in ((0, 64, 1, 1, 0), (-4, 64, 1, 1, 0), (64, 1, 1, 1, 0), (64, 513, 1, 1, 0), (64, 64, 0, 1, 0), (64, 64, 65, 1, 0),
            (1 << 20, 64, 65536, 1, 0), (64, 64, 8, 0, 0), (64, 64, 8, -1, 0), (64, 64, 8, 3, 0), (64, 64, 8, 128, 0),
            (64, 64, 8, 1, -1), (64, 64, 8, 1, 257), ((1 << 31) - 1, 512, 1, 1, 0), (1 << 28, 512, 1, 1, 0)):
    assert iq(*a) == 0, a
  for a in ((0, 8, 1, 64, 8, 0), (8, 0, 1, 64, 8, 0), (8, 8, 0, 64, 8, 0), (8, 8, 1, 1, 8, 0), (8, 8, 1, 513, 8, 0),
            (8, 8, 1, 64, 0, 0), (70000, 1, 1, 64, 1, 0), (1 << 15, 1 << 15, 2, 2, 1 << 15, 0), (8, 8, 1, 64, 8, -1),
            (8, 8, 1, 64, 8, 257), ((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1, 2, (1 << 31) - 1, 0)):
    assert pq(*a) == 0, a
  sizes = [iq(M, 64, 1, 1, 0) for M in (1, 2, 63, 64, 65, 1000, 1 << 20)]
  assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
  sizes = [pq(h, 7, 3, 64, 8, 19) for h in (1, 2, 8, 9, 100, 4096)]
  assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
  assert iq(4096, 64, 64, 16, 19) == iq(4096, 64, 64, 16, 19)


def test_bad_arguments_are_refused_before_any_launch():
  """No device exists here: a call that got as far as a launch could not return JPDSE_EINVAL or JPDSE_EWORKSPACE."""
  lb = jpdse_hip.lib()
  P = 4096                                 # 16-byte aligned and never dereferenced: every call below is refused on its arguments
  EINVAL, EWORKSPACE = -1, -2

  def index_call(M=64, L=64, S=8, G=4, index=P, h=0, w=0, H=0, W=0, label=None, n_classes=0, symbol=None, cell=P, group=P,
                 units=P, decisions=P, status=P, cu=None, cp=None, wsp=P, ws_bytes=None):
    if ws_bytes is None:
      ws_bytes = max(lb.jpdse_vq_index_cost_workspace_size(64, 64, 8, 4, 0), 1)
    return lb.jpdse_vq_index_cost(ctypes.byref(VqIndexCostArgs(M, L, S, G, index, h, w, H, W, label, n_classes, symbol, cell, group,
                                                               units, decisions, status, cu, cp, wsp, ws_bytes, None)))

  def plane_call(h=4, w=4, G=4, L=64, strip_rows=2, index=P, H=0, W=0, label=None, n_classes=0, symbol=None, cell=P, group=P,
                 units=P, decisions=P, status=P, cu=None, cp=None, wsp=P, ws_bytes=None):
    if ws_bytes is None:
      ws_bytes = max(lb.jpdse_vq_plane_cost_workspace_size(4, 4, 4, 64, 2, 0), 1)
    return lb.jpdse_vq_plane_cost(ctypes.byref(VqPlaneCostArgs(h, w, G, L, strip_rows, index, H, W, label, n_classes, symbol, cell,
                                                               group, units, decisions, status, cu, cp, wsp, ws_bytes, None)))

  null = 'null pointer'
  pointers = [(dict(index=None), null), (dict(cell=None), null), (dict(group=None), null), (dict(units=None), null),
              (dict(decisions=None), null), (dict(status=None), null)]
  label = dict(label=P, cu=P, cp=P, n_classes=19)
  label_cases = [(dict(label, H=16, W=16, cu=None), 'class_units or class_pixels'), (dict(label, H=16, W=16, cp=None), 'class_units or class_pixels'),
                 (dict(label, H=0, W=16), 'non-positive extent'), (dict(label, H=16, W=8), 'power-of-two multiple'),
                 (dict(label, H=12, W=12), 'power-of-two multiple'), (dict(label, H=16, W=16, n_classes=0), 'n_classes 0 outside [1, 256]'),
                 (dict(label, H=16, W=16, n_classes=257), 'n_classes 257 outside [1, 256]')]
  index_cases = [(dict(L=1), 'n_center L = 1'), (dict(L=513), 'n_center L = 513'), (dict(M=0), 'M = 0'), (dict(S=0), 'S = 0 streams'),
                 (dict(S=65), 'S = 65 streams'), (dict(G=0), 'G = 0 groups'), (dict(G=3), 'G = 3 groups'), (dict(G=-4), 'G = -4 groups')]
  index_cases += pointers + [(dict(kw, h=4, w=4), want) for kw, want in label_cases]
  index_cases += [(dict(label, H=16, W=16, h=4, w=3), 'does not hold M = 64'), (dict(label, H=16, W=16, h=0, w=0), 'does not hold M = 64'),
                  (dict(wsp=4100), 'not 16-byte aligned')]
  plane_cases = [(dict(L=1), 'n_center L = 1'), (dict(L=513), 'n_center L = 513'), (dict(h=0), 'h = 0'), (dict(w=-2), 'w = -2'),
                 (dict(G=0), 'G = 0'), (dict(strip_rows=0), 'strip_rows = 0'), (dict(h=70000, strip_rows=1), 'S = 280000 streams')]
  plane_cases += pointers + label_cases + [(dict(wsp=4100), 'not 16-byte aligned')]
  for who, call, cases_ in (('vq_index_cost', index_call, index_cases), ('vq_plane_cost', plane_call, plane_cases)):
    for kw, want in cases_:
      lb.jpdse_code_export(7, 0, 0, 0, 0, None, 0, None, None)      # leaves another call's message behind
      assert call(**kw) == EINVAL, (who, kw)
      msg = jpdse_hip.last_error()
      assert msg.startswith(who + ': ') and want in msg, (who, kw, msg)
    for kw in (dict(wsp=None), dict(ws_bytes=TABLE_BYTES + 4 * 64 - 1), dict(ws_bytes=0)):
      assert call(**kw) == EWORKSPACE, (who, kw)
      assert jpdse_hip.last_error().startswith(who + ': workspace too small'), jpdse_hip.last_error()
  for fn, name in ((lb.jpdse_vq_index_cost, 'vq_index_cost'), (lb.jpdse_vq_plane_cost, 'vq_plane_cost')):
    assert fn(None) == EINVAL and jpdse_hip.last_error().startswith(name + ': null argument struct')


def test_stream_module_refuses_before_the_library(monkeypatch):
  from jpdse_hip import ops, streams
  assert ops.vq_index_cost is streams.vq_index_cost and ops.vq_plane_cost is streams.vq_plane_cost
  touched = lambda: (_ for _ in ()).throw(AssertionError('library touched'))
  monkeypatch.setattr(streams, 'lib', touched)

  class FakeIndex(object):                 # what the checks read of a device tensor
    is_cuda, device, dtype = True, 'dev', torch.int32

    def __init__(self, M):
      self.M, self.shape = M, (M,)

    def dim(self):
      return 1

    def numel(self):
      return self.M

    def is_contiguous(self):
      return True

  with pytest.raises(ValueError, match='L = 513'):
    streams.vq_index_cost(FakeIndex(64), 513, 8)
  with pytest.raises(ValueError, match='S = 65 streams'):
    streams.vq_index_cost(FakeIndex(64), 64, 65)
  with pytest.raises(ValueError, match='groups = 3 does not divide'):
    streams.vq_index_cost(FakeIndex(64), 64, 8, groups=3)
  with pytest.raises(ValueError, match='hw = '):
    streams.vq_index_cost(FakeIndex(64), 64, 8, groups=4, label=torch.zeros(1, 1, 16, 16), n_classes=19, hw=(4, 3))
  with pytest.raises(ValueError, match='shape is'):
    streams.vq_plane_cost(FakeIndex(64), (4, 4), 64)
  with pytest.raises(ValueError, match='strip_rows 0'):
    streams.vq_plane_cost(FakeIndex(64), (4, 4, 4), 64, strip_rows=0)
  with pytest.raises(ValueError, match='n_classes without a label map'):
    streams.vq_plane_cost(FakeIndex(64), (4, 4, 4), 64, n_classes=19)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_reference_on_hand_worked_streams():
  T = cref.table()
  assert T[1024] == 65536 and T[0] == T[2048] == 0
  # one symbol of L = 2: one decision at q = 1024, one bit
  r = cref.index_cost([1], 2, 1)
  assert r['symbol'].tolist() == [65536] and r['stream_decisions'].tolist() == [1] and r['status'] == 0
  # two zeros of L = 4 in one stream: nodes 1 and 2 at 1024, then both at 1024 + (1024 >> 5) = 1056
  r = cref.index_cost([0, 0], 4, 1)
  assert r['symbol'].tolist() == [2 * 65536, 2 * T[1056]] and r['stream_decisions'].tolist() == [4]
  # the same two symbols in two streams: both tables fresh
  assert cref.index_cost([0, 0], 4, 2)['symbol'].tolist() == [2 * 65536, 2 * 65536]
  # a 1 x 3 plane of L = 4, values 2 2 1: literal | left flag hit (entry 0) | flag missed, then the literal
  r = cref.plane_cost([2, 2, 1], 1, 3, 1, 4, 8)
  q_miss = 1024 - (1024 >> 5)                   # entry 0 after one bit 1
  # the literal of 1 = 01b walks node 1 (seen once, bit 1: 992) with bit 0, then node 2, untouched by the literal of 2 = 10b
  assert r['symbol'].tolist() == [2 * 65536, T[2048 - 1024], T[q_miss] + T[992] + T[2048 - 1024]]
  assert r['stream_decisions'].tolist() == [2 + 1 + 3]
  # a 2 x 1 plane: no left cell ever; the second symbol codes the upper flag at entry 10
  r = cref.plane_cost([3, 3], 2, 1, 1, 4, 8)
  assert r['symbol'].tolist() == [2 * 65536, 65536] and r['stream_decisions'].tolist() == [3]
  # strips of one row: no upper cell, two streams
  r = cref.plane_cost([3, 3], 2, 1, 1, 4, 1)
  assert r['symbol'].tolist() == [2 * 65536, 2 * 65536] and r['stream_decisions'].tolist() == [2, 2]
  # a bad index is priced as 0 and reported
  bad, good = cref.index_cost([5, -1, 1, 4], 4, 2), cref.index_cost([0, 0, 1, 0], 4, 2)
  assert bad['status'] == 2 and good['status'] == 0
  assert all(np.array_equal(bad[k], good[k]) for k in ('symbol', 'cell', 'group', 'stream_units', 'stream_decisions'))


def _check_identities(r, M, G, S):
  total = int(r['symbol'].sum())
  assert r['symbol'].shape == (M,) and r['cell'].shape == (M // G,) and r['group'].shape == (G,)
  assert r['stream_units'].shape == (S,) and r['stream_decisions'].shape == (S,)
  assert int(r['cell'].sum()) == int(r['group'].sum()) == int(r['stream_units'].sum()) == total
  assert int(r['symbol'].min()) > 0 and r['status'] == 0


def test_index_walk_prices_the_decisions_the_reference_coder_codes():
  """Stream by stream: the (entry, q, bit) sequence of the cost walk is the one the coder's own Encoder saw; the identities; and
  the bound against the coder's bytes -- the CPU check of the bound, before any device run."""
  worst_lo, worst_hi, checked = 0.0, 0.0, 0
  for shape in icases.SHAPES:
    M, L, S = shape
    for kind in icases.KINDS:
      v, payload, _ = icases.reference(shape, kind)
      flat = v.tolist()
      streams = vref.split_payload(payload, S)
      for G in (1, 4) if M % 4 == 0 else (1,):
        r = cref.index_cost(flat, L, S, G)
        _check_identities(r, M, G, S)
      for s in range(S) if S <= 8 or kind == 'uniform' else (0, S - 1):
        priced = []
        costs, decisions = cref.index_stream_costs(flat[s::S], L, priced)
        coded, data = cref.coder_trace(vref, vref.encode_stream, flat[s::S], L)
        assert coded == priced and data == streams[s], (shape, kind, s)
        assert sum(costs) == int(r['stream_units'][s]) and decisions == int(r['stream_decisions'][s]) == vref.index_bits(L) * len(flat[s::S])
      for s in range(S):                       # no stream is left out
        gap = cref.gap_bits(len(streams[s]), int(r['stream_units'][s]))
        assert abs(gap) <= cref.bound_bits(int(r['stream_decisions'][s])), (shape, kind, s, gap)
        worst_lo, worst_hi, checked = min(worst_lo, gap) if checked else gap, max(worst_hi, gap), checked + 1
  print('index coder: 8 * bytes - bits per stream between %+.2f and %+.2f over %d streams' % (worst_lo, worst_hi, checked))
  assert checked == sum(S for _, _, S in icases.SHAPES) * len(icases.KINDS)


def test_plane_walk_prices_the_decisions_the_reference_coder_codes():
  worst_lo, worst_hi, checked, flags_seen = 0.0, 0.0, 0, set()
  for shape in pcases.SHAPES:
    h, w, G, L, strip_rows = shape
    S = pref.strips(h, strip_rows) * G
    for kind in pcases.KINDS:
      v, payload, _ = pcases.reference(shape, kind)
      flat = v.tolist()
      streams = pref.split_payload(payload, S)
      r = cref.plane_cost(flat, h, w, G, L, strip_rows)
      _check_identities(r, h * w * G, G, S)
      for s in range(S):
        k, g = divmod(s, G)
        rows = pref._strip_rows_of(flat, h, w, G, strip_rows, k, g)
        priced = []
        costs, decisions = cref.plane_stream_costs(rows, L, priced)
        coded, data = cref.coder_trace(pref, pref.encode_stream, rows, L)
        assert coded == priced and data == streams[s], (shape, kind, s)
        assert sum(sum(row) for row in costs) == int(r['stream_units'][s]) and decisions == int(r['stream_decisions'][s]) == len(priced)
        flags_seen.update((e, bit) for e, _, bit in priced if e <= 10)
        gap = cref.gap_bits(len(streams[s]), int(r['stream_units'][s]))
        assert abs(gap) <= cref.bound_bits(decisions), (shape, kind, s, gap)
        worst_lo, worst_hi, checked = min(worst_lo, gap) if checked else gap, max(worst_hi, gap), checked + 1
  print('plane coder: 8 * bytes - bits per stream between %+.2f and %+.2f over %d streams' % (worst_lo, worst_hi, checked))
  # every flag entry a stream can reach, with both outcomes, was priced somewhere: equality is transitive, so of the three
  # comparisons behind the left flag's entry exactly two cannot hold (3, 5 and 6 never occur)
  assert flags_seen == {(e, bit) for e in (0, 1, 2, 4, 7, 8, 9, 10) for bit in (0, 1)}, sorted(flags_seen)


# ---- the model's calls ------------------------------------------------------------------------------------------------------------
def _bare_model(codec):
  """A Pix2PixHDModel that never ran its constructor: only what the refusals read.  Anything that would touch the device raises."""
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  m = Pix2PixHDModel.__new__(Pix2PixHDModel)
  boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError('device work before the refusal'))
  m.__dict__.update(codec=codec, preprocess=boom, _device=boom, _encoder_eval=boom, _semantics=boom)
  return m


def _bare_trainer(model):
  from ctu.trainers.pix2pixHD_trainer import Pix2PixHDTrainer
  tr = Pix2PixHDTrainer.__new__(Pix2PixHDTrainer)
  tr.__dict__.update(model=model, eval=lambda: None)
  return tr


X_DICT = {'label': torch.zeros(2, 1, 64, 32), 'instance': torch.zeros(2, 1, 64, 32, dtype=torch.int64), 'image': torch.zeros(2, 3, 64, 32)}


@pytest.mark.parametrize('call', ['get_vq_rate_map', 'get_vq_class_rates'])
def test_new_calls_validate_coder_before_device_work(call):
  from ctu.models.codec import VQIndexCodec
  m = _bare_model(VQIndexCodec.__new__(VQIndexCodec))
  for target in (m, _bare_trainer(m)):
    for coder in ('jpdv', 'order0', '', 0, 'Index', ('index',)):
      with pytest.raises(ValueError, match='coder') as err:
        getattr(target, call)(X_DICT, coder=coder)
      assert call in str(err.value)
    for coder in (None, 'index', 'plane'):     # a good value gets as far as the device
      with pytest.raises(AssertionError, match='device work'):
        getattr(target, call)(X_DICT, coder=coder)
  with pytest.raises(AssertionError, match='device work'):
    getattr(m, call)(X_DICT)


@pytest.mark.parametrize('call', ['get_vq_rate_map', 'get_vq_class_rates'])
def test_new_calls_need_the_vq_encoder(call):
  from ctu.models.codec import BinaryCodec
  for codec in (None, BinaryCodec.__new__(BinaryCodec)):
    m = _bare_model(codec)
    for target in (m, _bare_trainer(m)):
      with pytest.raises(ValueError, match='the vector-quantised code needs --encoder_quantizer s2hvq') as err:
        getattr(target, call)(X_DICT, coder='bogus')       # the quantizer's refusal comes first
      assert str(err.value).startswith(call + ': ')


@pytest.mark.parametrize('call', ['get_rate_map', 'get_class_rates'])
def test_binarizer_calls_still_refuse_s2hvq_with_the_pinned_text(call):
  from ctu.models.codec import VQIndexCodec
  m = _bare_model(VQIndexCodec.__new__(VQIndexCodec))
  want = ('%s: a call of the one-bit binarizer\'s code, not available with --encoder_quantizer s2hvq (its code: '
          'get_vq_code / get_coded / get_coded_rate)' % call)
  with pytest.raises(ValueError) as err:
    getattr(m, call)(X_DICT)
  assert str(err.value) == want
  pinned = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'codec_refusals.json')))
  assert want in json.dumps(pinned)


def test_codec_cost_doc_says_what_a_packed_jpdv_is_priced_as():
  from ctu.models.codec import VQIndexCodec
  from ctu.utils import vqstream
  assert 'packed' in VQIndexCodec.cost.__doc__ and 'index' in VQIndexCodec.cost.__doc__
  assert VQIndexCodec.COST_CODERS == (None, 'index', 'plane')
  # the stream count of the index model is the one payloads() hands write_indices, clamped as write_indices clamps it
  assert vqstream.clamp_streams(16 * 8, 32768) == 128 and vqstream.clamp_streams(16 * 8, 100) == 100
  assert vqstream.clamp_streams(0, 5) == 1 and vqstream.clamp_streams(1 << 20, 1 << 20) == vqstream.MAX_STREAMS
