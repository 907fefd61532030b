"""CPU-only: when a conv layer rebuilds its two GEMM panels, and by which call (jpdse_hip/panels.py).

The layers live on the CPU, the two launching wrappers (ops.conv_pack, ops.conv_pack_into) are replaced by recorders, and the
library is used for its host-only queries alone (jpdse_conv_dgrad_pack_size, jpdse_conv_pack_entries): nothing is launched.
The expected sequences of the event tests were read off the code before panels.py existed: HipConv2d.packs(),
batched_pack_entries() and bwd_input_slice() of that code pass test_events_* and test_slice_panels as they stand, with one
exception -- an fp32 PACKED layer answered batched_pack_entries() with None, not [], when nothing had moved (PackBatcher treats
both as "skip this layer")."""
import ctypes

import pytest
import torch

from jpdse_hip import lib, ops, layers, F32, BF16, ACT_NONE, PAD_ZERO, JpdseError, PackEntry
from jpdse_hip.layers import HipConv2d, Ctx

LAYERS = {      # the smallest shapes that reach each kind ...
    'cast': lambda: HipConv2d(64, 16, 3, 1, 1, dtype=BF16),
    'cast_T': lambda: HipConv2d(128, 64, 3, 2, 1, apply_bias=False, transposed=True, dtype=BF16),
    'packed_bf16': lambda: HipConv2d(39, 64, 3, 1, 1, dtype=BF16),
    'alias': lambda: HipConv2d(16, 8, 3, 1, 1, dtype=F32),
    'packed_f32': lambda: HipConv2d(39, 64, 3, 1, 1, dtype=F32),
    # ... and the smallest at which jpdse_conv_pack_entries has rows for a stride-1 layer: it answers -1 below 64 x 64 padded
    # channels (csrc/conv_gemm.hip: those phases take the padded-K pack kernel), which leaves such a layer to the lazy path
    # whatever the rule says -- 'cast' and 'alias' above are such layers, and the None they answer is the library's
    'cast_64': lambda: HipConv2d(64, 64, 3, 1, 1, dtype=BF16),
    'alias_64': lambda: HipConv2d(64, 64, 3, 1, 1, dtype=F32),
}
KIND = {'cast': 'cast', 'cast_T': 'cast', 'packed_bf16': 'packed', 'alias': 'alias', 'packed_f32': 'packed', 'cast_64': 'cast',
        'alias_64': 'alias'}
NO_ROWS = ('cast', 'alias')


class Recorder(object):
  """Stands in for the two pack launches.  calls: 'alloc' = conv_pack (new buffers, both panels), 'both' / 'dgrad' =
  conv_pack_into with / without a forward panel; `into` holds the buffers of the conv_pack_into calls."""

  def __init__(self, monkeypatch):
    self.calls, self.into, self.sources = [], [], []
    monkeypatch.setattr(ops, 'conv_pack', self.pack)
    monkeypatch.setattr(ops, 'conv_pack_into', self.pack_into)

  def pack(self, d, w, device):
    self.calls.append('alloc')
    self.sources.append(w)
    return torch.zeros(8, dtype=torch.uint8, device=device), torch.zeros(8, dtype=torch.uint8, device=device)

  def pack_into(self, d, w, fwd, dgr):
    assert dgr is not None and dgr.dtype == torch.uint8
    self.calls.append('dgrad' if fwd is None else 'both')
    self.into.append((fwd, dgr))
    self.sources.append(w)

  def take(self):
    calls, self.calls = self.calls, []
    return calls


# ---- the events -------------------------------------------------------------------------------------------------------------
def optimizer_step(w, cast_written=True):
  """What FusedAdam.step() says through the protocol after its kernel updated w."""
  w._jpdse_wver = getattr(w, '_jpdse_wver', 0) + 1
  if cast_written and getattr(w, '_jpdse_cast_out', None) is not None:
    w._jpdse_cast_wver = w._jpdse_wver


def ev_step(layer):
  optimizer_step(layer.weight)


def ev_step_cast_stale(layer):
  optimizer_step(layer.weight, cast_written=False)


def ev_inplace(layer):
  with torch.no_grad():
    layer.weight.mul_(0.5)


def ev_epoch(layer):
  layers.bump_weights_epoch()


def ev_storage(layer):
  layer.weight.data = layer.weight.data.clone(memory_format=torch.preserve_format)


#  event                   ->  kind: (batched_pack_entries() right after it, what the next packs() records)
E, N_ = 'entries', None
EVENTS = [
    (ev_step,            {'cast': (E, ['dgrad']),  'packed': (N_, ['both']), 'alias': (E, ['dgrad'])}),
    (ev_step_cast_stale, {'cast': (N_, ['both']),  'packed': (N_, ['both']), 'alias': (E, ['dgrad'])}),      # ALIAS has no cast to lag
    (ev_inplace,         {'cast': (N_, ['both']),  'packed': (N_, ['both']), 'alias': (N_, ['dgrad'])}),
    (ev_epoch,           {'cast': (N_, ['both']),  'packed': (N_, ['both']), 'alias': (N_, ['dgrad'])}),
    (ev_storage,         {'cast': (N_, ['both']),  'packed': (N_, ['both']), 'alias': (N_, ['dgrad'])}),     # ALIAS: a NEW buffer
]
FIRST = {'cast': ['alloc'], 'packed': ['alloc'], 'alias': ['dgrad']}     # ALIAS: the master is the forward panel, torch.empty the other


def first_use(layer, rec, kind):
  assert layer.batched_pack_entries() is None                    # no panels yet: the lazy path allocates
  fwd, dgrad = layer.packs()
  assert rec.take() == FIRST[kind]
  if kind == 'alias':
    assert fwd.data_ptr() == layer.weight.data_ptr() and rec.into[-1][1] is dgrad
    assert dgrad.numel() == lib().jpdse_conv_dgrad_pack_size(ctypes.byref(layer._desc(1, 64, 64))) > 0
  assert getattr(layer.weight, '_jpdse_cast_out', None) is (fwd if kind == 'cast' else None)
  quiet(layer, rec, (fwd, dgrad))
  return fwd, dgrad


def quiet(layer, rec, bufs):
  """Nothing moved: nothing for the batcher, nothing recorded, the same buffers."""
  assert layer.batched_pack_entries() == []
  again = layer.packs()
  assert again[0] is bufs[0] and again[1] is bufs[1] and rec.take() == []


def apply_event(layer, rec, name, bufs, event, expect):
  kind = KIND[name]
  want_entries, want_calls = expect[kind]
  event(layer)
  e = layer.batched_pack_entries()
  if want_entries is None or name in NO_ROWS:
    assert e is None
  else:
    assert isinstance(e, list) and len(e) >= 1
    assert all(x.w == layer.weight.data_ptr() for x in e)
    assert layer.batched_pack_entries() is e                     # the table rows are built once per (master, panel) pair
  assert rec.take() == []                                        # asking launches nothing
  fwd, dgrad = layer.packs()
  assert rec.take() == want_calls
  if kind == 'alias':
    assert fwd.data_ptr() == layer.weight.data_ptr()
    assert (dgrad is bufs[1]) == (event is not ev_storage), 'ALIAS re-allocates its data-gradient panel with the storage, only then'
  else:
    assert fwd is bufs[0] and dgrad is bufs[1]
    assert rec.into[-1][0] is (fwd if want_calls == ['both'] else None) and rec.into[-1][1] is dgrad
  assert rec.sources[-1] is layer.weight
  quiet(layer, rec, (fwd, dgrad))
  return fwd, dgrad


@pytest.mark.parametrize('name', sorted(LAYERS))
def test_events_in_sequence(name, monkeypatch):
  rec = Recorder(monkeypatch)
  layer = LAYERS[name]()
  bufs = first_use(layer, rec, KIND[name])
  for event, expect in EVENTS + EVENTS[:1]:                      # ... and a clean optimizer step heals a lagging cast
    bufs = apply_event(layer, rec, name, bufs, event, expect)


@pytest.mark.parametrize('event,expect', EVENTS, ids=[e.__name__ for e, _ in EVENTS])
@pytest.mark.parametrize('name', sorted(LAYERS))
def test_events_from_a_fresh_state(name, event, expect, monkeypatch):
  rec = Recorder(monkeypatch)
  layer = LAYERS[name]()
  apply_event(layer, rec, name, first_use(layer, rec, KIND[name]), event, expect)


def test_slice_panels(monkeypatch):
  """bwd_input_slice: panels of the sliced master -- allocated per channel range, re-packed in place when the master moved."""
  rec = Recorder(monkeypatch)
  used = []
  monkeypatch.setattr(ops, 'conv_dgrad', lambda d, dz, pack, **kw: used.append((d.C, pack)))
  layer = HipConv2d(39, 64, 4, 2, 2, PAD_ZERO, act=ACT_NONE, dtype=BF16)
  x = ops.Act.empty(1, 8, 8, 39, BF16, 'cpu')
  dy = ops.Act.empty(1, 5, 5, 64, BF16, 'cpu')
  ctx = Ctx(x, None)
  layer.bwd_input_slice(ctx, dy, 36, 39)
  assert rec.take() == ['alloc'] and tuple(rec.sources[-1].shape) == (64, 3, 4, 4)
  assert torch.equal(rec.sources[-1], layer.weight.detach()[:, 36:39])
  layer.bwd_input_slice(ctx, dy, 36, 39)
  assert rec.take() == [] and used[1][1] is used[0][1]
  optimizer_step(layer.weight)
  layer.bwd_input_slice(ctx, dy, 36, 39)
  assert rec.take() == ['both'] and rec.into[-1][1] is used[0][1] and used[2][1] is used[0][1]
  assert rec.into[-1][0].data_ptr() != rec.into[-1][1].data_ptr()
  layer.bwd_input_slice(ctx, dy, 35, 38)
  assert rec.take() == ['alloc'] and used[3][1] is not used[0][1]
  assert torch.equal(rec.sources[-1], layer.weight.detach()[:, 35:38])
  assert [c for c, _ in used] == [3, 3, 3, 3]
  assert getattr(layer.weight, '_jpdse_cast_out', None) is None  # the slice panels publish nothing to the optimizer
  assert layer.batched_pack_entries() is None                    # and are not the layer's own panels


# ---- what only the new structure has ----------------------------------------------------------------------------------------
def test_decision_table():
  """panels.decide, the rule itself: every kind x {no panels, stamp equal, only the optimizer counter moved (cast fresh / stale),
  anything else moved}."""
  from jpdse_hip.panels import decide, ALIAS, CAST, PACKED, ALLOC_AND_PACK, PACK_BOTH, PACK_DGRAD_ONLY, NONE
  old = (3, 1, 0x1000, 5)
  stepped = (3, 1, 0x1000, 6)
  moved = [(4, 1, 0x1000, 5), (3, 2, 0x1000, 5), (4, 1, 0x1000, 6)]       # torch version, weights epoch, version + counter
  storage = [(3, 1, 0x2000, 5), (0, 1, 0x2000, 6)]
  for kind in (ALIAS, CAST, PACKED):
    for fresh in (False, True):
      for now in [old, stepped] + moved + storage:
        assert decide(kind, False, None, now, fresh) == (ALLOC_AND_PACK, False)
      assert decide(kind, True, old, old, fresh) == (NONE, True)
  for fresh in (False, True):
    assert decide(ALIAS, True, old, stepped, fresh) == (PACK_DGRAD_ONLY, True)
    assert decide(PACKED, True, old, stepped, fresh) == (PACK_BOTH, False)
    for now in moved:
      assert decide(ALIAS, True, old, now, fresh) == (PACK_DGRAD_ONLY, False)
      assert decide(CAST, True, old, now, fresh) == (PACK_BOTH, False)
      assert decide(PACKED, True, old, now, fresh) == (PACK_BOTH, False)
    for now in storage:
      assert decide(ALIAS, True, old, now, fresh) == (ALLOC_AND_PACK, False)
      assert decide(CAST, True, old, now, fresh) == (PACK_BOTH, False)
      assert decide(PACKED, True, old, now, fresh) == (PACK_BOTH, False)
  assert decide(CAST, True, old, stepped, True) == (PACK_DGRAD_ONLY, True)
  assert decide(CAST, True, old, stepped, False) == (PACK_BOTH, False)


def test_kinds_and_stamp():
  from jpdse_hip import panels
  for name, make in LAYERS.items():
    assert make()._panels.kind == KIND[name], name
  w = LAYERS['alias']().weight
  assert panels.stamp(w) == (w._version, panels._weights_epoch[0], w.data_ptr(), 0)
  panels.optimizer_stepped(w)
  assert panels.stamp(w)[3] == 1 and not hasattr(w, '_jpdse_cast_wver')
  panels.publish_cast(w, torch.zeros(1))
  panels.optimizer_stepped(w)
  assert (w._jpdse_wver, w._jpdse_cast_wver) == (2, 2) and panels.cast_target(w) is w._jpdse_cast_out


def test_batcher_covers_and_marks(monkeypatch):
  """PackBatcher.run() with its launch recorded: one table over the layers that answer with entries, block0 running over its
  rows; the covered layers are fresh afterwards, the others keep their lazy pack; an unchanged table is not uploaded again."""
  rec = Recorder(monkeypatch)
  runs = []
  monkeypatch.setattr(ops, 'conv_pack_run', lambda table, n, total: runs.append((table, n, total)))
  net = torch.nn.ModuleDict({name: make() for name, make in LAYERS.items()})
  batcher = layers.PackBatcher(net)
  for name, m in net.items():
    first_use(m, rec, KIND[name])
  assert batcher.run() == 0 and runs == []
  for round_ in range(2):
    for m in net.values():
      ev_step(m)
    covered = [name for name in LAYERS if KIND[name] != 'packed' and name not in NO_ROWS]
    rows = [e for name in covered for e in net[name].batched_pack_entries()]
    assert batcher.run() == len(covered) == 3 and len(runs) == round_ + 1
    table, n, total = runs[-1]
    assert n == len(rows) and total == sum(e.blocks for e in rows) and table.numel() == n * 96 and table.dtype == torch.uint8
    got = (PackEntry * n).from_buffer_copy(bytes(table.numpy()))
    assert [(g.w, g.out, g.blocks) for g in got] == [(e.w, e.out, e.blocks) for e in rows]
    assert [g.block0 for g in got] == [sum(e.blocks for e in rows[:i]) for i in range(n)]
    assert all(e.block0 == 0 for e in rows)                      # the layers' cached rows stay as the library made them
    for name, m in net.items():
      m.packs()
      assert rec.take() == ([] if name in covered else ['dgrad'] if name in NO_ROWS else ['both']), name
  assert runs[1][0] is runs[0][0]


def test_moved_master_device_is_refused(monkeypatch):
  """Packing into buffers that live on another device than the master is refused (it used to pack across devices silently)."""
  rec = Recorder(monkeypatch)
  layer = LAYERS['packed_bf16']()
  layer.packs()
  layer.weight = torch.nn.Parameter(torch.empty(layer.weight.shape, device='meta').contiguous(memory_format=torch.channels_last))
  with pytest.raises(JpdseError, match='device|moved'):
    layer.packs()
  assert rec.take() == ['alloc']
