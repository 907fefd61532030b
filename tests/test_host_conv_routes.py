"""CPU-only guard of the conv dispatch itself: for every layer of scripts/make_conv_host_queries.py the developer build names the
route (jpd-se_amd/csrc/conv_route.h: the kernel family) its forward, data gradient and weight gradient take
(jpdse_debug_conv_route; nothing is launched).  Under the shipped dispatch the names must equal tests/golden/conv_routes.json
(written by scripts/make_conv_routes.py); the slot queries must answer for the route the launch will select; a developer mode
must not select what it switches off."""
import ctypes
import json
import os
import sys

import pytest

import jpdse_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

import make_conv_host_queries as gen      # noqa: E402
import make_conv_routes as mr             # noqa: E402

DESCRIPTORS = gen.all_descriptors()
MOMENT_ROUTES = {'thin_fwd', 'rows', 'halo'}      # forward routes whose kernels have a moment epilogue
RING = {'ring_taps9_frame', 'ring_halo_frame', 'ring_taps9_strips', 'ring_halo_strips'}
ROWS_FWD = {'rows', 'thin_in_rows', 'thin_rows', 'head_rows'}                         # the row-streaming family (g_rows_enabled)
ROWS_DGRAD = {'rows', 'dgrad2_rows', 'thin_dgrad2_rows', 'thin_in_rows'}
# mode -> the routes it switches off, per direction (include/jpdse_dev.h, jpdse_debug_set_fast_path)
SWITCHED_OFF = {
    3: (ROWS_FWD | {'halo'}, ROWS_DGRAD | RING | {'halo'}, set()),
    6: ({'taps4', 'taps9', 'head_fwd', 'head_rows'},
        {'taps9', 'taps4', 'taps_dgrad2', 'thin1', 'head', 'ring_taps9_frame', 'ring_halo_frame', 'ring_taps9_strips'}, {'thin1'}),
    7: (set(), RING, set()),
    29: (ROWS_FWD, ROWS_DGRAD, set()),
    35: (set(), {'taps_dgrad2'}, set()),
    40: (set(), {'ring_taps9_frame', 'ring_halo_frame'}, set()),
}


@pytest.fixture(scope='module')
def dev():
  with jpdse_hip.dev_mode(1) as lib:
    yield lib
    assert lib.jpdse_debug_set_fast_path(1) == 0


def test_route_names_cover_every_route(dev):
  names = [[], [], []]
  for direction in range(3):
    while dev.jpdse_debug_route_name(direction, len(names[direction])) is not None:
      names[direction].append(dev.jpdse_debug_route_name(direction, len(names[direction])).decode())
    assert len(set(names[direction])) == len(names[direction]) and names[direction][-1] == 'generic'
    assert dev.jpdse_debug_route_name(direction, -1) is None
  assert (len(names[0]), len(names[1]), len(names[2])) == (13, 16, 8)
  assert dev.jpdse_debug_route_name(3, 0) is None
  for sets in SWITCHED_OFF.values():
    assert all(s <= set(n) for s, n in zip(sets, names))      # the tables above name routes that exist
  assert MOMENT_ROUTES <= set(names[0]) and RING <= set(names[1])


def test_shipped_dispatch_takes_the_recorded_routes(dev):
  fix = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'conv_routes.json')))
  assert fix['descriptor_fields'] == gen.DESC_FIELDS and fix['route_fields'] == ['fwd', 'dgrad', 'wgrad']
  assert [tuple(c[0]) for c in fix['cases']] == DESCRIPTORS
  wrong = ['%s: %s, recorded %s' % (dict(zip(gen.DESC_FIELDS, key)), got, want)
           for key, want in fix['cases'] for got in [mr.routes(dev, tuple(key))] if got != want]
  assert not wrong, '%d of %d layers moved to another kernel:\n%s' % (len(wrong), len(fix['cases']), '\n'.join(wrong[:20]))


def cpad(c):
  return (c + 7) & ~7


def test_slot_queries_answer_for_the_selected_route(dev):
  """A slot count > 0 promises that the launch writes that many slots, so it must come from the route the launch selects with
  the same wants, and asking for moments must not move the layer (the invariant the queries used to rely on silently).

  Conversely a moment-writing route answers > 0 except where its own slot formula says its epilogue does not serve the layer,
  and each exception is asserted for what it is: an activation in the descriptor (moments are asked of a bare conv: 80 of the
  672 layers), the halo kernel's single-buffered form (<= 64 input channels: 7 layers), thin_fwd tiles that do not divide
  the output (18 layers); for the norm-backward sums, a tile other than 128 dense channels (9 layers)."""
  for key in DESCRIPTORS:
    d = jpdse_hip.ConvDesc(*key, gen.SLOPE)
    what = dict(zip(gen.DESC_FIELDS, key))
    plan = gen.query(dev, key)[1:55]
    OH, OW = plan[4], plan[5]
    plain = mr.routes(dev, key)
    fwd_m = mr.routes(dev, key, mr.FWD_MOMENTS)[0]
    slots = dev.jpdse_conv_moment_slots(ctypes.byref(d))
    if what['act'] != 0 or fwd_m not in MOMENT_ROUTES:
      assert slots == 0, (what, slots, fwd_m)
    elif fwd_m == 'rows':
      assert slots > 0, what
    elif fwd_m == 'halo':
      assert (slots > 0) == (cpad(what['C']) > 64) and slots in (0, (OH // 4) * (OW // 64)), (what, slots)
    else:      # thin_fwd: tiles of 8 | 4 rows x 64 | 32 pixels, one slot each when they divide the output
      assert slots in [0] + [(OH // th) * (OW // tw) for th, tw in ((8, 64), (4, 64), (4, 32)) if OH % th == 0 and OW % tw == 0], (what, slots)
      assert slots > 0 or not (OH % 8 == 0 and OW % 64 == 0), (what, slots)
    if slots > 0:
      assert fwd_m == plain[0], (what, fwd_m, plain)
    dgrad_m = mr.routes(dev, key, mr.DGRAD_MOMENTS)[1]
    assert (dev.jpdse_convT_moment_slots(ctypes.byref(d)) > 0) == (dgrad_m == 'dgrad2_rows'), (what, dgrad_m)
    assert dgrad_m == plain[1] or dgrad_m != 'dgrad2_rows', (what, dgrad_m, plain)
    nsum = dev.jpdse_conv_dgrad_nsum_slots(ctypes.byref(d))
    for extra in (0, mr.DGRAD_MASK, mr.DGRAD_MASK | mr.DGRAD_ADDEND):      # jpdse_conv_dgrad_fused_nsums launches with mask and addend
      dgrad_n = mr.routes(dev, key, mr.DGRAD_NSUMS | extra)[1]
      serves = dgrad_n == 'ring_halo_frame' and cpad(what['K']) >= 128 and what['C'] % 128 == 0
      assert (nsum > 0) == serves and nsum in (0, (what['H'] // 4) * (what['W'] // 64)), (what, nsum, dgrad_n, extra)
      assert nsum == 0 or dgrad_n == plain[1], (what, dgrad_n, plain)


def test_developer_modes_select_nothing_they_switch_off(dev):
  try:
    assert dev.jpdse_debug_set_fast_path(0) == 0
    for key in DESCRIPTORS:
      assert mr.routes(dev, key) == ['generic'] * 3, key
    for mode, off in SWITCHED_OFF.items():
      assert dev.jpdse_debug_set_fast_path(mode) == 0
      for key in DESCRIPTORS:
        for flags in (0, mr.FWD_MOMENTS | mr.DGRAD_MASK | mr.DGRAD_ADDEND):
          got = mr.routes(dev, key, flags)
          assert not any(r in s for r, s in zip(got, off)), (mode, key, flags, got)
  finally:
    assert dev.jpdse_debug_set_fast_path(1) == 0
  assert mr.routes(dev, DESCRIPTORS[0]) == ['thin_fwd', 'fast', 'thin']      # mode 1 is back
