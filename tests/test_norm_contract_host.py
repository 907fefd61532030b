"""The InstanceNorm contracts (tests/norm_contract.py) on the CPU: each criterion accepts a faithful fp32 emulation of each form of
csrc/norm.hip at the shapes tests/test_hip_norm_contract.py runs on the device, and rejects the defects it exists to catch,
planted into that emulation.  On integer operands a defect must change the stored bits; on randn operands it must exceed the
bound 10x wherever the statistics criterion is the one meant to catch it.  torch-CPU only."""
import pytest
import torch

from jpdse_hip import F32, BF16, ACT_NONE, ACT_RELU, ACT_LRELU
from bf16_contract import CAP, Cand, contract_figures
from ew_contract import VE, cpad, ulp_f32
import norm_contract as nc

DTYPES = [F32, BF16]


def forms_at(dtype, N, HW, C):
  """[(form, geometry)] the device test reaches at this shape: the shipped build's form, and the three-kernel form."""
  out = [nc.norm_form(dtype, N, HW, C)]
  if out[0][0] != 'moment':
    out.append(nc.norm_form(dtype, N, HW, C, three_kernel=True))
  return out


def test_geometry_restatements():
  for dtype in DTYPES:
    C = nc.main_c(dtype)
    for HW in nc.HW_EDGES:
      form, g = nc.norm_form(dtype, nc.images_for(HW), HW, C)
      if HW == 8193:
        assert form == 'moment' and nc.fused_geom(1, HW, cpad(C), VE[dtype])['splits'] == 65
      else:
        assert form == 'rows' and (g['TX'], g['span'], g['col_blocks'], g['splits']) == (16, 128, 1, nc.ROWS_SPLITS[HW]), (dtype, HW, g)
    # the 16-row chunks of sum_rows: 17 rows are one full chunk and a chunk of one
    assert -(-nc.ROWS_SPLITS[2049] // 16) == 2 and nc.ROWS_SPLITS[2049] % 16 == 1
    g = nc.fused_geom(2, 100, 8, VE[dtype])
    assert (g['TX'], g['TY']) == ((1, 256) if dtype == BF16 else (2, 128))
    assert nc.fused_geom(2, g['span'] + 1, 8, VE[dtype])['splits'] == 2
    seen = set()
    for Cc in nc.CHANNELS[dtype]:
      g = nc.fused_geom(2, 300, cpad(Cc), VE[dtype])
      if g['cv'] < g['TX']:
        seen.add('idle_lanes')
      if g['col_blocks'] == 2 and g['cv'] - g['TX'] == 8 // VE[dtype]:        # one lane (fp32: Cs is a multiple of 8, so two)
        seen.add('second_block_one_lane')
      if cpad(Cc) != Cc:
        seen.add('pad_lanes')
    assert seen == {'idle_lanes', 'second_block_one_lane', 'pad_lanes'}, (dtype, seen)
    (c4, hw4), (c1, hw1) = nc.MOMENT_EXTRA
    form, g = nc.norm_form(dtype, 1, hw4, c4, three_kernel=True)
    assert form == 'moment' and g['splits'] > 24 and nc.loop_and_tail(nc.reduce_splits_trips(g['splits'])), g
    assert nc.norm_form(dtype, 2, hw1, c1, three_kernel=True)[1]['splits'] == 1
    # 64 splits: the four-at-a-time loop alone
    assert not nc.loop_and_tail(nc.reduce_splits_trips(nc.norm_form(dtype, 1, 8193, C)[1]['splits']))
    for slots, HW in nc.SLOT_CASES:
      assert nc.norm_form(dtype, 2, HW, C, slots=slots)[0] == ('phase3' if slots <= 64 else 'slots')
      assert nc.norm_form(dtype, 2, HW, C, slots=slots, three_kernel=True)[0] == 'slots'
      assert HW % slots == 0 and nc.is_pow2(HW // slots)
  assert nc.loop_and_tail(nc.finalize_slots_trips(260)) and not nc.loop_and_tail(nc.finalize_slots_trips(65))
  assert nc.finalize_slots_trips(65)[0] == (0, 2) and nc.finalize_slots_trips(260)[3] == (1, 1) and nc.finalize_slots_trips(260)[4] == (1, 0)


def not_single_rounding(y, x, stats, act, res):
  """Share of the elements of an fp32-emulated bf16 output that are not the single rounding of the fp64 value."""
  cands, exact, S, n = nc.fwd_reference(x, stats, act, res)
  return contract_figures(y.double(), [Cand(exact)], S, n)[1]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('HW', nc.HW_EDGES)
def test_clean_emulation_of_each_form_passes(HW, dtype):
  C, N = nc.main_c(dtype), nc.images_for(HW)
  x, dy, res = nc.norm_inputs(N, HW, C, dtype, 11 + HW)
  xi = nc.flat(nc.int_fwd_case(N, HW, C, 5))
  bx, bdy = nc.int_bwd_case(N, HW, C, 6)
  means = []
  for form, g in forms_at(dtype, N, HW, C):
    what = '%s HW %d' % (form, HW)
    stats = nc.emu_stats(x, form, g)
    nc.assert_stats(stats, x, what)
    for act, with_res in (nc.ACT_RES if HW <= 2049 else nc.ACT_RES[:1]):
      r = res if with_res else None
      y = nc.emu_apply_fwd(x, stats, act, r, dtype)
      nc.assert_fwd(y, x, stats, act, r, C, dtype, what)
      if dtype == BF16:
        # the reference arithmetic alone leaves the single rounding far less often than the cap allows
        assert not_single_rounding(y, x, stats, act, r) <= CAP / 10
      nc.assert_bwd(nc.emu_bwd(x, dy, stats, act, dtype, form, g), x, dy, stats, act, C, dtype, what)
    si = nc.emu_stats(xi, form, g)
    nc.assert_int_stats(si, xi, what)
    means.append(si[..., 0])
    for act in (ACT_NONE, ACT_RELU, ACT_LRELU):
      dx = nc.emu_bwd(bx, bdy, nc.unit_stats(N, bx.shape[-1]), act, dtype, form, g, slope=nc.PLUMB_SLOPE)
      nc.assert_int_bwd(dx, bx, bdy, act, what)
  assert all(torch.equal(m, means[0]) for m in means), 'integer operands: the forms disagree on the mean'


@pytest.mark.parametrize('dtype', DTYPES)
def test_clean_emulation_other_shapes(dtype):
  """The channel shapes, the small-C shapes and the moment form's extra shapes."""
  shapes = [(2, 300, c) for c in nc.CHANNELS[dtype]] + [(2, 100, 8), (2, nc.fused_geom(2, 100, 8, VE[dtype])['span'] + 1, 8)]
  shapes += [(1 if hw > 2049 else 2, hw, c) for c, hw in nc.MOMENT_EXTRA]
  for N, HW, C in shapes:
    x, dy, res = nc.norm_inputs(N, HW, C, dtype, 3 * C + HW)
    xi = nc.flat(nc.int_fwd_case(N, HW, C, 7))
    for form, g in forms_at(dtype, N, HW, C):
      what = '%s C %d HW %d' % (form, C, HW)
      stats = nc.emu_stats(x, form, g)
      nc.assert_stats(stats, x, what)
      nc.assert_fwd(nc.emu_apply_fwd(x, stats, ACT_LRELU, res, dtype), x, stats, ACT_LRELU, res, C, dtype, what)
      nc.assert_bwd(nc.emu_bwd(x, dy, stats, ACT_LRELU, dtype, form, g), x, dy, stats, ACT_LRELU, C, dtype, what)
      nc.assert_int_stats(nc.emu_stats(xi, form, g), xi, what)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', nc.CONDITIONING)
def test_conditioning_cases_pass_for_the_clean_emulation(kind, dtype):
  C, N, HW = nc.main_c(dtype), 2, 2049
  x, dy, res = nc.conditioning_inputs(kind, N, HW, C, dtype, 21)
  for form, g in forms_at(dtype, N, HW, C):
    stats = nc.emu_stats(x, form, g)
    nc.assert_stats(stats, x, kind + ' ' + form)
    y = nc.emu_apply_fwd(x, stats, ACT_NONE, res, dtype)
    nc.assert_fwd(y, x, stats, ACT_NONE, res, C, dtype, kind + ' ' + form)
    if kind == 'constant':
      assert torch.equal(stats[..., :C, 0], torch.full((N, C), 1.5)) and torch.equal(y, res)
    nc.assert_bwd(nc.emu_bwd(x, dy, stats, ACT_RELU, dtype, form, g), x, dy, stats, ACT_RELU, C, dtype, kind + ' ' + form)


# ---- planted defects: the reductions --------------------------------------------------------------------------------------------
def stats_used(stats, x):
  return max(nc.stats_figures(stats, nc.stats_reference(x)))


@pytest.mark.parametrize('dtype', DTYPES)
def test_reduction_defects_are_rejected(dtype):
  C = nc.main_c(dtype)
  # (defect, HW, forms): the last pixel of the ragged second split; partial row 16 of 17; the divisor
  plan = [('drop_last_pixel', 129, ('rows', 'moment')), ('skip_row_16', 2049, ('rows',)), ('dup_row_16', 2049, ('rows',)),
          ('divisor_hw_minus_1', 129, ('rows', 'moment'))]
  for defect, HW, forms in plan:
    x, dy, res = nc.norm_inputs(2, HW, C, dtype, 31)
    xi = nc.flat(nc.int_fwd_case(2, HW, C, 5))
    bx, bdy = nc.int_bwd_case(2, HW, C, 6)
    for form, g in forms_at(dtype, 2, HW, C):
      if form not in forms:
        continue
      assert stats_used(nc.emu_stats(x, form, g), x) <= 1.0
      assert stats_used(nc.emu_stats(x, form, g, defect=defect), x) > 10.0, (defect, form)
      with pytest.raises(AssertionError):
        nc.assert_int_stats(nc.emu_stats(xi, form, g, defect=defect), xi, defect)
      if defect != 'divisor_hw_minus_1':       # both sums are zero: their divisor is out of the plumbing check's sight
        with pytest.raises(AssertionError):
          dx = nc.emu_bwd(bx, bdy, nc.unit_stats(2, bx.shape[-1]), ACT_RELU, dtype, form, g, slope=nc.PLUMB_SLOPE, defect=defect)
          nc.assert_int_bwd(dx, bx, bdy, ACT_RELU, defect)
  # at the largest shapes only the integer operands tell: one pixel of 8192 moves the mean by a hundredth of the bf16 bound
  for HW, form_defects in ((8192, ('drop_last_pixel', 'skip_row_16', 'divisor_hw_minus_1')), (8193, ('drop_last_pixel',))):
    xi = nc.flat(nc.int_fwd_case(1, HW, C, 5))
    form, g = nc.norm_form(dtype, 1, HW, C)
    nc.assert_int_stats(nc.emu_stats(xi, form, g), xi, 'clean')
    for defect in form_defects:
      with pytest.raises(AssertionError):
        nc.assert_int_stats(nc.emu_stats(xi, form, g, defect=defect), xi, defect)


@pytest.mark.parametrize('dtype', DTYPES)
def test_chan_merge(dtype):
  C = nc.main_c(dtype)
  for slots, HW in nc.SLOT_CASES:
    x, dy, res = nc.norm_inputs(2, HW, C, dtype, 41 + slots)
    mom = nc.slots_of(x, slots)
    xi = nc.flat(nc.int_slot_case(2, HW, C, slots, 8))
    momi = nc.slots_of(xi, slots)
    for form in ('phase3', 'slots') if slots <= 64 else ('slots',):
      what = '%s %d slots' % (form, slots)
      stats = nc.emu_slot_stats(mom, HW, form)
      nc.assert_slot_stats(stats, mom, HW, what)
      # the merged statistics are those of the data, up to the slots' own fp32 rounding
      ref = nc.stats_reference(x)
      assert float(((stats[..., 0].double() - ref[0]).abs() / ref[0].abs().clamp_min(1.0)).max()) < 1e-5
      nc.assert_int_slot_stats(nc.emu_slot_stats(momi, HW, form), xi, C, what)
      for defect in ('no_ns_dm2', 'mean_div_slots_minus_1'):
        if slots == 1:
          continue                              # one slot: no dm^2 term, and no slots - 1 to divide by
        bad = nc.emu_slot_stats(mom, HW, form, defect=defect)
        assert max(nc.stats_figures(bad, nc.slot_stats_reference(mom, HW))) > 10.0, (defect, what)
        with pytest.raises(AssertionError):
          nc.assert_int_slot_stats(nc.emu_slot_stats(momi, HW, form, defect=defect), xi, C, what)
      # backward slots: the sums of the slots are the sums of the data
      sl = nc.sum_slots_of(x, dy, stats, ACT_LRELU, slots)
      yh, dz, ss = nc.bwd_terms(x, dy, stats, ACT_LRELU)
      sums = nc.emu_slot_sums(sl, HW, form)
      nc.assert_bwd(nc.emu_apply_bwd(yh, dz, ss, sums, dtype), x, dy, stats, ACT_LRELU, C, dtype, what)


# ---- planted defects: the apply expressions --------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_apply_defects_are_rejected(dtype):
  N, HW, C = 2, 300, 17
  x, dy, res = nc.norm_inputs(N, HW, C, dtype, 51)
  form, g = nc.norm_form(dtype, N, HW, C)
  stats = nc.emu_stats(x, form, g)
  for act, defect in ((ACT_RELU, 'res_before_act'), (ACT_LRELU, 'res_before_act'), (ACT_LRELU, 'slope_on_positive'),
                      (ACT_NONE, 'nonzero_pad')):
    nc.assert_fwd(nc.emu_apply_fwd(x, stats, act, res, dtype), x, stats, act, res, C, dtype, 'clean')
    with pytest.raises(AssertionError):
      nc.assert_fwd(nc.emu_apply_fwd(x, stats, act, res, dtype, C=C, defect=defect), x, stats, act, res, C, dtype, defect)
  y = nc.emu_apply_fwd(x, stats, ACT_RELU, res, dtype)
  for act, defect in ((ACT_RELU, 'mask_from_stored_y'), (ACT_LRELU, 'mask_from_stored_y'), (ACT_NONE, 'yhat_m2_sign'),
                      (ACT_RELU, 'yhat_m2_sign')):
    nc.assert_bwd(nc.emu_bwd(x, dy, stats, act, dtype, form, g), x, dy, stats, act, C, dtype, 'clean')
    with pytest.raises(AssertionError):
      nc.assert_bwd(nc.emu_bwd(x, dy, stats, act, dtype, form, g, defect=defect, y=y), x, dy, stats, act, C, dtype, defect)
  # aliased: 2B saved images, 3B gradient images
  B = 2
  x, _, _ = nc.norm_inputs(2 * B, HW, C, dtype, 52)
  _, dy, _ = nc.norm_inputs(3 * B, HW, C, dtype, 53)
  stats = nc.emu_stats(x, form, g)
  nc.assert_bwd(nc.emu_bwd(x, dy, stats, ACT_RELU, dtype, form, g, alias=B), x, dy, stats, ACT_RELU, C, dtype, 'aliased', alias=B)
  with pytest.raises(AssertionError):
    nc.assert_bwd(nc.emu_bwd(x, dy, stats, ACT_RELU, dtype, form, g, alias=B, defect='alias_off_by_one'), x, dy, stats, ACT_RELU,
                  C, dtype, 'alias_off_by_one', alias=B)


# ---- facts of the bound ------------------------------------------------------------------------------------------------------------
def test_bound_facts():
  HW, C = 2048, 8
  x = nc.flat(nc.randn_nhwc((1, C, 1, HW), F32, 61))
  width = {}
  for k in (0.0, 8.0, 16.0):
    xk = x.clone()
    if k:
      xk[:, 0, :C] = k
    width[k] = nc.stats_reference(xk)[3][0, :C]
  # an outlier first pixel (the kernel's shift) widens the bound, and the bound follows sum d^2 = HW (var + (mean - shift)^2)
  assert bool((width[8.0] > 10 * width[0.0]).all())
  ratio = width[16.0] / width[8.0]
  assert bool(((ratio > 3.0) & (ratio < 4.6)).all()), ratio
  # the shift-free bound does not move with the first pixel (beyond what one pixel does to the variance)
  xk = x.clone()
  xk[:, 0, :C] = 16.0
  free = nc.stats_reference(xk, shift_free=True)[3][0, :C] / nc.stats_reference(x, shift_free=True)[3][0, :C]
  assert bool((free < 1.5).all()), free
  # never below one ulp of the result: a constant channel, a single pixel, the slot merge of one slot
  for t in (torch.full((2, 300, 8), 1.5), nc.flat(nc.randn_nhwc((2, 8, 1, 1), BF16, 62))):
    mean, rstd, bm, br = nc.stats_reference(t)
    assert bool((bm >= ulp_f32(mean)).all()) and bool((br >= ulp_f32(rstd)).all())
  mean, rstd, bm, br = nc.slot_stats_reference(nc.slots_of(torch.full((2, 8, 8), 1.5), 1), 8)
  assert bool((bm >= ulp_f32(mean)).all()) and bool((br >= ulp_f32(rstd)).all())
  assert nc.rsqrt_ulp_error(torch.tensor([0.5]), torch.tensor([4.0])) == 0.0
