"""Pure-Python restatement of the code-length maps of the two S2HVQ index coders, jpdse_vq_index_cost and jpdse_vq_plane_cost
(TEST INFRASTRUCTURE), written from the definitions of DESIGN.md 4.20 and from nothing else.  The cost table and the update of
a probability are tests/code_cost_ref.py's (`table`, `adapted`), the stream geometry and the flag entries are those of the
reference coders tests/vq_coder_ref.py and tests/vq_plane_ref.py (imported, not edited).  Integer arithmetic throughout.

  decision  coded with the probability q of bit 0 (before its update): T[q] for bit 0, T[2048 - q] for bit 1
  symbol    the sum over the decisions its coder spends on it
  index     symbol m in stream m % S: the nb bit-tree decisions, most significant bit first, node m at entry m
  plane     symbol (y, x, g) in stream k * G + g: the left flag (if coded), the upper flag (if coded), the literal at the
            entries 10 + m (if neither matched)
  bad       an index outside [0, L) counts as 0, for itself and as a neighbour; status bit 1

Every walk can record the (entry, q, bit) sequence it prices (`trace`); `coder_trace` replays a reference *coder* with a hook
on its Encoder and returns the sequence it coded: tests/test_vq_cost_host.py asserts the two are the same.
"""
import numpy as np

import rc_ref
import vq_coder_ref as vref
import vq_plane_ref as pref
from code_cost_ref import UNIT, adapted, class_tables, table  # noqa: F401  (UNIT, class_tables: re-exported)
from rc_ref import PROB_INIT, PROB_ONE

index_bits = vref.index_bits


def _decide(probs, entry, bit, trace):
  q = probs[entry]
  probs[entry] = adapted(q, bit)
  if trace is not None:
    trace.append((entry, q, bit))
  return table()[PROB_ONE - q] if bit else table()[q]


def _literal(probs, base, v, nb, trace):
  m, units = 1, 0
  for k in range(nb - 1, -1, -1):
    bit = (v >> k) & 1
    units += _decide(probs, base + m, bit, trace)
    m = m << 1 | bit
  return units


def _clean(values, L):
  """(the values as the coders see them, status)."""
  flat = [int(v) for v in values]
  bad = any(not 0 <= v < L for v in flat)
  return [v if 0 <= v < L else 0 for v in flat], (2 if bad else 0)


def index_stream_costs(symbols, L, trace=None):
  """symbols: the values of one stream, each in [0, L) -> (the cost of each, the decisions coded)."""
  nb = index_bits(L)
  probs = [PROB_INIT] * (1 << nb)
  return [_literal(probs, 0, v, nb, trace) for v in symbols], nb * len(symbols)


def plane_stream_costs(rows, L, trace=None):
  """rows: the strip of one group as a list of rows of values in [0, L) -> (the costs in the same shape, the decisions coded)."""
  nb = index_bits(L)
  probs = [PROB_INIT] * (10 + (1 << nb))
  out, decisions = [], 0
  for y, row in enumerate(rows):
    costs = []
    for x, v in enumerate(row):
      lf = row[x - 1] if x > 0 else None
      u = rows[y - 1][x] if y > 0 else None
      ul = rows[y - 1][x - 1] if x > 0 and y > 0 else None
      left, up = pref._flag_entries(lf, u, ul)
      units, hit = 0, False
      if lf is not None:
        hit = v == lf
        units += _decide(probs, left, int(hit), trace)
        decisions += 1
      if not hit and u is not None and u != lf:
        hit = v == u
        units += _decide(probs, up, int(hit), trace)
        decisions += 1
      if not hit:
        units += _literal(probs, 10, v, nb, trace)
        decisions += nb
      costs.append(units)
    out.append(costs)
  return out, decisions


def _sums(symbol, G, stream_units, stream_decisions, status):
  symbol = np.asarray(symbol, dtype=np.int64)
  by_cell = symbol.reshape(-1, G)
  return dict(symbol=symbol, cell=by_cell.sum(axis=1), group=by_cell.sum(axis=0),
              stream_units=np.asarray(stream_units, dtype=np.int64), stream_decisions=np.asarray(stream_decisions, dtype=np.int64),
              status=status)


def index_cost(indices, L, S, G=1):
  """indices: M integers (any value: one outside [0, L) is priced as 0) -> dict of int64 numpy arrays: symbol [M], cell [M / G],
  group [G], stream_units [S], stream_decisions [S]; status: 2 when an index was outside [0, L)."""
  flat, status = _clean(indices, L)
  M = len(flat)
  assert 1 <= S <= M and G >= 1 and M % G == 0
  symbol, units, decisions = [0] * M, [], []
  for s in range(S):
    costs, n = index_stream_costs(flat[s::S], L)
    symbol[s::S] = costs
    units.append(sum(costs))
    decisions.append(n)
  return _sums(symbol, G, units, decisions, status)


def plane_cost(indices, h, w, G, L, strip_rows):
  """The same for the index planes: cell (y, x, g) at (y * w + x) * G + g; cell [h * w]; S = ceil(h / strip_rows) * G."""
  flat, status = _clean(indices, L)
  assert len(flat) == h * w * G
  symbol, units, decisions = [0] * (h * w * G), [], []
  for k in range(pref.strips(h, strip_rows)):
    y0 = k * strip_rows
    for g in range(G):
      costs, n = plane_stream_costs(pref._strip_rows_of(flat, h, w, G, strip_rows, k, g), L)
      for dy, row in enumerate(costs):
        for x, c in enumerate(row):
          symbol[((y0 + dy) * w + x) * G + g] = c
      units.append(sum(sum(row) for row in costs))
      decisions.append(n)
  return _sums(symbol, G, units, decisions, status)


def bound_bits(decisions):
  """|8 * stream bytes - stream units / 65536| <= 48 + decisions / 64."""
  return 48.0 + decisions / 64.0


def gap_bits(stream_bytes, units):
  """8 * stream bytes - units / 65536: what the bound is about."""
  return 8.0 * stream_bytes - units / float(UNIT)


class _Recorder(rc_ref.Encoder):
  """rc_ref.Encoder that notes (entry, q, bit) of every adaptive decision before it codes it."""
  traces = None

  def encode(self, probs, ctx, bit):
    _Recorder.traces[-1].append((ctx, probs[ctx], bit))
    rc_ref.Encoder.encode(self, probs, ctx, bit)

  def __init__(self, counters=None):
    rc_ref.Encoder.__init__(self, counters)
    _Recorder.traces.append([])


def coder_trace(module, encode_stream, *args):
  """The (entry, q, bit) sequence the reference coder `module`.`encode_stream`(*args) codes, and its bytes: the coder itself
  runs, with the recording Encoder in the place of the one it imported."""
  saved, _Recorder.traces = module.Encoder, []
  module.Encoder = _Recorder
  try:
    data = encode_stream(*args)
  finally:
    module.Encoder = saved
  (trace,) = _Recorder.traces
  return trace, data
