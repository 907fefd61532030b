"""The InstanceNorm kernels of csrc/norm.hip against their fp64 contract (tests/norm_contract.py; the criteria themselves are checked
on the CPU by tests/test_norm_contract_host.py), form by form: the two register-held kernels, moment -> finalize -> apply
(developer mode 27), PHASE 3 from producer slots, the two slot-finalize kernels + apply, and the aliased backward -- statistics
against fp64 within the derived bound, forward and backward against fp64 given the device's own statistics, pad lanes, and the
integer-operand plumbing check, at the smallest shapes that reach each path.  Which form and how many splits a case reaches is
asserted from the Python restatement of the geometry, not assumed."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import jpdse_hip
from jpdse_hip import ops, F32, BF16, ACT_NONE, ACT_RELU, ACT_LRELU
from jpdse_hip.ops import Act
import hip_util
from hip_util import DEV, DTYPES, record
from ew_contract import VE, cpad, tdtype, assert_bits_equal
import norm_contract as nc

ACTS = (ACT_NONE, ACT_RELU, ACT_LRELU)


@pytest.fixture(scope='module', autouse=True)
def _gpu():
  jpdse_hip.require_gpu(0)


def dev(t, C, dtype):
  """[N, HW, Cs] fp32 CPU storage values -> Act [N, 1, HW, Cs] on the device (exact: the values are representable)."""
  return Act(t.to(tdtype(dtype)).view(t.shape[0], 1, t.shape[1], t.shape[2]).to(DEV).contiguous(), C)


def host(a):
  torch.cuda.synchronize()
  t = a.t if isinstance(a, Act) else a
  return nc.flat(t.detach().cpu().float()) if t.dim() == 4 else t.detach().cpu()


def label(case, form):
  """`case form`: the case goes into the parity report's note (hip_util.record strips it from the comparison's name), so that the
  report keeps one line per form and criterion with its worst case."""
  hip_util.CASE[0] = case
  return case + ' ' + form


def mode(three_kernel):
  return jpdse_hip.dev_mode(27) if three_kernel else contextlib.nullcontext()


def fwd_bwd(x, dy, res, C, dtype, act, three_kernel, slope=nc.SLOPE32, stats=None):
  """(y, stats, dx) on the host; with `stats` given, the backward alone."""
  X, DY = dev(x, C, dtype), dev(dy, C, dtype)
  with mode(three_kernel):
    y = None
    if stats is None:
      y, stats = ops.inorm_fwd(X, act, slope, nc.EPS, dev(res, C, dtype) if res is not None else None)
    else:
      stats = stats.to(DEV)
    dx = ops.inorm_bwd(X, stats, DY, act, slope, nc.EPS)
    return (host(y) if y is not None else None), host(stats), host(dx)


def check_shift_forms(x, dy, res, C, dtype, what, combos, want=None):
  """Contracts a, b, c in the shipped build's form and in the three-kernel form; `want`: the form the shipped build must reach."""
  N, HW = x.shape[0], x.shape[1]
  for three in (False, True):
    form, g = nc.norm_form(dtype, N, HW, C, three_kernel=three)
    assert form == ('moment' if three else (want or form)), (form, want)
    for i, (act, with_res) in enumerate(combos):
      r = res if with_res else None
      y, stats, dx = fwd_bwd(x, dy, r, C, dtype, act, three)
      if i == 0:
        nc.assert_stats(stats, x, label(what, form))
      w = label('%s act %d%s' % (what, act, ' +res' if with_res else ''), form)
      nc.assert_fwd(y, x, stats, act, r, C, dtype, w)
      nc.assert_bwd(dx, x, dy, stats, act, C, dtype, w)
    if form == 'moment' and not three:
      break                                    # the shipped build is on the three-kernel form already


def check_plumbing(N, HW, C, dtype, what):
  """Integer operands: exact mean in every form, bit-equal across forms; dx == dz in every form."""
  xi = nc.int_fwd_case(N, HW, C, 5)
  bx, bdy = nc.int_bwd_case(N, HW, C, 6)
  unit = nc.unit_stats(N, cpad(C))
  means = []
  for three in (False, True):
    form = nc.norm_form(dtype, N, HW, C, three_kernel=three)[0]
    _, stats, _ = fwd_bwd(xi, bdy, None, C, dtype, ACT_NONE, three)
    nc.assert_int_stats(stats, xi, label(what, form))
    means.append(stats[..., 0].contiguous())
    for act in ACTS:
      _, _, dx = fwd_bwd(bx, bdy, None, C, dtype, act, three, slope=nc.PLUMB_SLOPE, stats=unit)
      nc.assert_int_bwd(dx, bx, bdy, act, label('%s act %d' % (what, act), form))
  assert_bits_equal(means[1], means[0], label(what, 'integer operands: mean, three-kernel form vs shipped form'))


# ---- rsqrtf ---------------------------------------------------------------------------------------------------------------------
def test_rsqrtf_allowance():
  """The device's rsqrtf against fp64 1 / sqrt at known fp32 arguments: PHASE 3 with one slot of one pixel hands M2 + eps to
  rsqrtf unchanged.  Arguments: var + eps of this suite's own inputs, and a log sweep of [eps, 4096]."""
  vs = [torch.logspace(-5, 3.612, 16384, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)]
  for dtype in DTYPES:
    C = nc.main_c(dtype)
    for HW in nc.HW_EDGES:
      vs.append(nc.norm_inputs(nc.images_for(HW), HW, C, dtype, 11 + HW)[0].double().var(dim=1, unbiased=False).flatten())
    for kind in nc.CONDITIONING:
      vs.append(nc.conditioning_inputs(kind, 2, 2049, C, dtype, 21)[0].double().var(dim=1, unbiased=False).flatten())
  var = torch.cat(vs).float()
  n, Cs = var.numel(), 1024
  N = -(-n // Cs)
  m2 = torch.zeros(N * Cs, dtype=torch.float32)
  m2[:n] = var
  mom = torch.stack([torch.zeros_like(m2), m2], dim=-1).view(N, Cs, 1, 2).contiguous()
  X = dev(torch.zeros((N, 1, Cs)), Cs, F32)
  assert nc.norm_form(F32, N, 1, Cs, slots=1)[0] == 'phase3'
  _, stats = ops.inorm_fwd_from_moments(X, mom.to(DEV), 1, ACT_NONE, nc.SLOPE32, nc.EPS)
  got = host(stats)[..., 1].reshape(-1)
  arg = m2 + nc.f32(nc.EPS)
  worst = nc.rsqrt_ulp_error(got, arg)
  print('rsqrtf: worst error %.4f ulp over %d arguments' % (worst, n))
  record('rsqrtf: worst error vs fp64 1 / sqrt, ulps (allowance RSQRT_ULPS = twice this, rounded up)', worst, nc.RSQRT_ULPS / 2.0,
         '%d arguments' % n)
  assert 2.0 * worst <= nc.RSQRT_ULPS, 'rsqrtf errs by %.3f ulp: RSQRT_ULPS = %d is no longer twice the measurement' % (worst, nc.RSQRT_ULPS)


# ---- the shift forms -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('HW', nc.HW_EDGES)
def test_pixel_edges(HW, dtype):
  """C = 16 vectors (TX 16, span 128): one and two pixels, rows past the end, one span, a ragged split of one pixel, 16 and 17
  splits (the 16-row chunks of sum_rows), 64 splits, and 65 (the shipped build's moment form); each also in mode 27."""
  C, N = nc.main_c(dtype), nc.images_for(HW)
  form, g = nc.norm_form(dtype, N, HW, C)
  if HW == 8193:
    assert form == 'moment' and g['splits'] == 64
  else:
    assert form == 'rows' and (g['TX'], g['span'], g['splits']) == (16, 128, nc.ROWS_SPLITS[HW])
  x, dy, res = nc.norm_inputs(N, HW, C, dtype, 11 + HW)
  combos = nc.ACT_RES if HW <= 2049 else [(ACT_LRELU, True), (ACT_RELU, False)]
  check_shift_forms(x, dy, res, C, dtype, 'HW %d' % HW, combos, want=form)
  check_plumbing(N, HW, C, dtype, 'HW %d' % HW)


@pytest.mark.parametrize('dtype', DTYPES)
def test_small_c(dtype):
  """C = 8: bf16 TX 1, TY 256 (span 2048); fp32 TX 2, TY 128 (span 1024).  Rows past the end, and a second split of one pixel."""
  g = nc.fused_geom(2, 100, 8, VE[dtype])
  assert (g['TX'], g['TY']) == ((1, 256) if dtype == BF16 else (2, 128))
  for HW in (100, g['span'] + 1):
    assert nc.norm_form(dtype, 2, HW, 8)[1]['splits'] == (1 if HW == 100 else 2)
    x, dy, res = nc.norm_inputs(2, HW, 8, dtype, 24 + HW)
    check_shift_forms(x, dy, res, 8, dtype, 'C 8 HW %d' % HW, [(ACT_LRELU, True), (ACT_RELU, False)], want='rows')
    check_plumbing(2, HW, 8, dtype, 'C 8 HW %d' % HW)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('ci', range(5))
def test_channel_edges(ci, dtype):
  """Padded channels, idle column lanes, a second column block with one vector: pad lanes of y and dx stay zero."""
  C, N, HW = nc.CHANNELS[dtype][ci], 2, 300
  x, dy, res = nc.norm_inputs(N, HW, C, dtype, 3 * C + HW)
  check_shift_forms(x, dy, res, C, dtype, 'C %d' % C, [(ACT_LRELU, True), (ACT_RELU, False), (ACT_NONE, True)], want='rows')
  check_plumbing(N, HW, C, dtype, 'C %d' % C)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C,HW', nc.MOMENT_EXTRA)
def test_moment_form_split_loops(C, HW, dtype):
  """Mode 27: more than 24 splits, so that the four-at-a-time loop of reduce_splits runs and leaves a tail; exactly one split."""
  N = 1 if HW > 2049 else 2
  form, g = nc.norm_form(dtype, N, HW, C, three_kernel=True)
  assert form == 'moment'
  if HW > 2049:
    assert g['splits'] > 24 and nc.loop_and_tail(nc.reduce_splits_trips(g['splits'])), g
  else:
    assert g['splits'] == 1
  x, dy, res = nc.norm_inputs(N, HW, C, dtype, 3 * C + HW)
  check_shift_forms(x, dy, res, C, dtype, 'C %d HW %d' % (C, HW), [(ACT_LRELU, True), (ACT_RELU, False)])
  check_plumbing(N, HW, C, dtype, 'C %d HW %d' % (C, HW))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', nc.CONDITIONING)
def test_conditioning(kind, dtype):
  """Mean >> sigma, an outlier first pixel (the kernels' shift), a constant channel, a channel constant but for one pixel: each
  held to the derived bound; the report's note quotes the error against the shift-free bound."""
  C, N, HW = nc.main_c(dtype), 2, 2049
  x, dy, res = nc.conditioning_inputs(kind, N, HW, C, dtype, 21)
  check_shift_forms(x, dy, res, C, dtype, kind, [(ACT_NONE, True), (ACT_RELU, False)], want='rows')
  if kind == 'constant':
    for three in (False, True):
      y, stats, _ = fwd_bwd(x, dy, res, C, dtype, ACT_NONE, three)
      assert_bits_equal(stats[..., :C, 0].contiguous(), torch.full((N, C), 1.5), 'constant channel: mean')
      assert_bits_equal(y, res, 'constant channel: y == res', dtype)
      y, _, _ = fwd_bwd(x, dy, None, C, dtype, ACT_LRELU, three)
      assert_bits_equal(y, torch.zeros_like(y), 'constant channel: y == 0', dtype)


# ---- the slot forms ------------------------------------------------------------------------------------------------------------
def slot_fwd_bwd(x, dy, res, C, dtype, act, slots, three_kernel, slope=nc.SLOPE32, stats=None, mom=None):
  X, DY = dev(x, C, dtype), dev(dy, C, dtype)
  with mode(three_kernel):
    y = None
    if stats is None:
      y, st = ops.inorm_fwd_from_moments(X, mom.to(DEV), slots, act, slope, nc.EPS, dev(res, C, dtype) if res is not None else None)
      stats = host(st)
    sums = nc.sum_slots_of(x, dy, stats, act, slots, slope)
    DY.nsums = (sums.to(DEV), slots, X.t.data_ptr())
    dx = ops.inorm_bwd(X, stats.to(DEV), DY, act, slope, nc.EPS)
    return (host(y) if y is not None else None), stats, host(dx)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('slots,HW', nc.SLOT_CASES)
def test_slot_forms(slots, HW, dtype):
  """Slots built on the CPU, equal pixel counts: 1, 2 and 64 slots reach PHASE 3, 65 and 260 the slot-finalize kernels + apply
  (260: the four-at-a-time loop of finalize_slots_kernel and its tail); every case again in mode 27, where all of them take the
  finalize kernels.  C = 72: a ragged channel block."""
  N = 2
  assert nc.loop_and_tail(nc.finalize_slots_trips(slots)) == (slots == 260)
  for C, combos in ((nc.main_c(dtype), [(ACT_NONE, True), (ACT_RELU, False), (ACT_LRELU, True)]), (72, [(ACT_LRELU, True)])):
    x, dy, res = nc.norm_inputs(N, HW, C, dtype, 41 + slots)
    mom = nc.slots_of(x, slots)
    xi = nc.int_slot_case(N, HW, C, slots, 8)
    bx, bdy = nc.int_bwd_case(N, HW, C, 6)
    for three in (False, True):
      form = nc.norm_form(dtype, N, HW, C, three_kernel=three, slots=slots)[0]
      assert form == ('phase3' if slots <= 64 and not three else 'slots')
      for i, (act, with_res) in enumerate(combos):
        r = res if with_res else None
        y, stats, dx = slot_fwd_bwd(x, dy, r, C, dtype, act, slots, three, mom=mom)
        if i == 0:
          nc.assert_slot_stats(stats, mom, HW, label('%d slots C %d' % (slots, C), form))
        w = label('%d slots C %d act %d%s' % (slots, C, act, ' +res' if with_res else ''), form)
        nc.assert_fwd(y, x, stats, act, r, C, dtype, w)
        nc.assert_bwd(dx, x, dy, stats, act, C, dtype, w)
      _, stats, _ = slot_fwd_bwd(xi, bdy, None, C, dtype, ACT_NONE, slots, three, mom=nc.slots_of(xi, slots))
      nc.assert_int_slot_stats(stats, xi, C, label('%d slots C %d' % (slots, C), form))
      for act in ACTS:
        _, _, dx = slot_fwd_bwd(bx, bdy, None, C, dtype, act, slots, three, slope=nc.PLUMB_SLOPE, stats=nc.unit_stats(N, cpad(C)))
        nc.assert_int_bwd(dx, bx, bdy, act, label('%d slots C %d act %d' % (slots, C, act), form))


# ---- the aliased backward --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B', [1, 2])
def test_aliased_backward(B, dtype):
  """3B gradient images over 2B saved ones (alias = B): each gradient image against the fp64 reference of ITS saved image."""
  C, HW = nc.main_c(dtype), 2049
  x, _, _ = nc.norm_inputs(2 * B, HW, C, dtype, 52)
  _, dy, _ = nc.norm_inputs(3 * B, HW, C, dtype, 53)
  bx, bdy = nc.int_bwd_case(3 * B, HW, C, 6)
  bx = bx[:2 * B].contiguous()
  X, DY, BX, BDY = dev(x, C, dtype), dev(dy, C, dtype), dev(bx, C, dtype), dev(bdy, C, dtype)
  unit = nc.unit_stats(2 * B, cpad(C)).to(DEV)
  for three in (False, True):
    form, g = nc.norm_form(dtype, 3 * B, HW, C, three_kernel=three, alias=B)
    assert form == ('moment' if three else 'rows') and g['splits'] == (16 if three else 17)     # 2049 // (16 * 8) = 16 moment splits
    with mode(three):
      _, stats = ops.inorm_fwd(X, ACT_NONE, nc.SLOPE32, nc.EPS)
      for act in (ACT_RELU, ACT_LRELU):
        dx = host(ops.inorm_bwd_aliased(X, stats, DY, B, act, nc.SLOPE32, nc.EPS))
        nc.assert_bwd(dx, x, dy, host(stats), act, C, dtype, label('B %d act %d' % (B, act), 'aliased ' + form), alias=B)
        dx = host(ops.inorm_bwd_aliased(BX, unit, BDY, B, act, nc.PLUMB_SLOPE, nc.EPS))
        nc.assert_int_bwd(dx, bx, bdy, act, label('B %d act %d' % (B, act), 'aliased ' + form), alias=B)
