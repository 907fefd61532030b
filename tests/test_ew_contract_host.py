"""The elementwise contracts (tests/ew_contract.py) on the CPU: each criterion accepts a faithful fp32 emulation of its kernel
and rejects the defects it exists to catch, planted into that emulation at the shapes tests/test_hip_ew_contract.py runs on the
device.  On the integer inputs a defect must change the result (inequality); on the randn inputs it must exceed the bound at
least 10x wherever that criterion is the one meant to catch it.  torch-CPU only."""
import numpy as np
import pytest
import torch

from jpdse_hip import F32, BF16, ACT_RELU, ACT_LRELU
import ew_contract as ec
from ew_contract import VE, cpad, edge_y, plateau

DTYPES = [F32, BF16]


def test_geometry_restatements():
  assert ec.loss_partial_count(1) == 1 and ec.loss_partial_count(256 * 257) == 257
  assert ec.loss_partial_count(262144) == ec.RED_BLOCKS == ec.loss_partial_count(266240)
  for dtype in DTYPES:
    N, C, H, W = ec.map_shapes(dtype)['cap']
    vecs = N * H * W * cpad(C) // VE[dtype]
    assert vecs == 532480 and ec.grid_stride_sweeps(vecs) == 2 and vecs - ec.EW_CAP < ec.EW_CAP
    # the kernels that enumerate something else than the tensor's vectors, each by its own work items
    npix = N * H * W
    assert npix == 66560
    assert ec.channel_copy_items(npix, 3) == 199680 and ec.insert_channels_items(dtype, npix, C - 5, 3) <= 133120   # one sweep
    wide = [ec.channel_copy_items(npix, ec.WIDE_COPY_NCH), ec.insert_channels_items(dtype, npix, ec.WIDE_INSERT_C0, C)]
    assert wide == [532480, 599040 if dtype == BF16 else 532480]
    layout = [N * cpad(C) * H * W, N * C * H * W]                    # nchw_to_nhwc, nhwc_to_nchw: one item per element
    for items in wide + layout:
      sweeps = ec.grid_stride_sweeps(items)
      assert sweeps >= 2 and 0 < items - (sweeps - 1) * ec.EW_CAP < ec.EW_CAP, items    # the last sweep is partial
    assert ec.grid_stride_sweeps(ec.CAST_N // 8) == 2 and ec.CAST_N // 8 - ec.EW_CAP == 3
    n, c, h, w = ec.MSE_CONST_SHAPES['cap_ragged']
    assert ec.grid_stride_sweeps(n * h * w * 8) == 5                 # mse_const_bwd: one item per storage element, 2129920
    for name, by in ec.LOSS_SHAPES.items():
      N, C, H, W = by[dtype]
      vecs = N * H * W * cpad(C) // VE[dtype]
      want = {'v1': 8 // VE[dtype], 'p255': 256 * 255, 'p256': 256 * 256, 'p257': 256 * 257, 'cap': 262144}.get(name, 266240)
      assert vecs == want, (name, dtype, vecs)
  hit = set()
  for name, dtype, npix, C in ec.CSUM_CASES:
    g = ec.csum_geom(dtype, npix, cpad(C))
    if name.startswith('blocks_'):
      assert g['nblk'] == int(name.split('_')[1])
    hit |= g['cases']
  assert hit >= ec.CSUM_REQUIRED, sorted(ec.CSUM_REQUIRED - hit)
  g = ec.csum_geom(F32, 2051, 1024)
  assert (g['TX'], g['TY']) == (256, 1)
  g = ec.csum_geom(BF16, 5632, 1024)
  assert (g['TX'], g['TY'], g['nblk']) == (128, 2, 512)
  # 9 blocks leave 3 partials per final group: the 8-wide unrolled loop needs a group of 8 or more, which 35 blocks give
  assert 'final_unrolled8_plus_tail' not in ec.csum_geom(BF16, 2304, 24)['cases']
  assert 'final_unrolled8_plus_tail' in ec.csum_geom(F32, 2240, 40)['cases']


def test_helpers():
  assert ec.ulp_f32(torch.tensor([1.0, 1.5, 2.0, 0.0])).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -149]
  assert float(ec.loss_value_exact(7, 3)) == float(np.float32(7) * (np.float32(1) / np.float32(3)))
  a = torch.tensor([0.0, 1.0]); b = torch.tensor([-0.0, 1.0])
  assert torch.equal(a, b) and ec.bits_differ(a, b) == 1          # the stored bits, not the values
  with pytest.raises(AssertionError):
    ec.assert_exact_terms(torch.full((2 ** 22,), 4.0), 'too large')
  with pytest.raises(AssertionError):
    ec.assert_exact_terms(torch.tensor([0.5]), 'not an integer')


# ---- grid-stride maps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_map_defects_change_the_stored_bits(dtype):
  for case, shape in ec.map_shapes(dtype).items():
    a, b = ec.randn_nhwc(shape, dtype, 1), ec.randn_nhwc(shape, dtype, 2)
    want = ec.emu_add(a, b, dtype)
    assert ec.bits_differ(ec.emu_add(a, b, dtype), want, dtype) == 0
    assert ec.bits_differ(ec.plant_map_defect(want, dtype, 'drop_last_vector'), want, dtype) > 0, case
    if case == 'cap':
      n = ec.bits_differ(ec.plant_map_defect(want, dtype, 'skip_second_sweep'), want, dtype)
      assert n >= (532480 - ec.EW_CAP) * VE[dtype] * 0.9


@pytest.mark.parametrize('dtype', DTYPES)
def test_relu_mask_ge_is_rejected(dtype):
  shape = ec.map_shapes(dtype)['ragged']
  y, dy = edge_y(shape, dtype, 3), ec.randn_nhwc(shape, dtype, 4, mean=1.0)
  for act in (ACT_RELU, ACT_LRELU):
    want = ec.emu_act_bwd(y, dy, act, dtype)
    bad = ec.emu_act_bwd(y, dy, act, dtype, defect='mask_ge')
    N, C = shape[0], shape[1]
    diff = ec.bits(bad.to(ec.tdtype(dtype))) != ec.bits(want.to(ec.tdtype(dtype)))
    # exactly the zeros of y among the logical lanes (the padding lanes hold dy = 0: -0 vs +0 products aside, no change)
    assert int(diff[..., :C].sum()) == int((y[..., :C] == 0).sum()) == 4
  g = ec.loss_gscale(1.0, 2.5, y[..., :shape[1]].numel())
  b = ec.randn_nhwc(shape, dtype, 5)
  want = ec.emu_l1_grad(y, b, g, dtype, relu_a=True)
  assert ec.bits_differ(ec.emu_l1_grad(y, b, g, dtype, relu_a=True, defect='mask_ge'), want, dtype) == 4
  assert float(want.view(-1, want.shape[-1])[0, 2]) != 0.0, 'a positive subnormal is alive'


@pytest.mark.parametrize('hw', [(8, 12), (9, 13), (2, 2), (3, 2)])
def test_maxpool_gradient_to_the_last_maximum_is_rejected(hw):
  H, W = hw
  for per_window in (True, False):
    x = plateau((2, 12, H, W), per_window)
    dy = ec.int_nhwc((2, 12, H // 2, W // 2), 1, 5, 9)
    want = ec.emu_maxpool_bwd(x, dy)
    assert torch.equal(want[:, 0:2 * (H // 2):2, 0:2 * (W // 2):2], dy), 'every window is a four-way tie: first element'
    assert float(want.sum()) == float(dy.sum())
    assert ec.bits_differ(ec.emu_maxpool_bwd(x, dy, defect='last_max'), want, F32) > 0
  x = ec.randn_nhwc((2, 12, H, W), BF16, 2)
  xr = x[..., :12].permute(0, 3, 1, 2).clone().requires_grad_(True)
  y = torch.nn.functional.max_pool2d(xr, 2, 2)
  assert torch.equal(ec.emu_maxpool_fwd(x)[..., :12], y.detach().permute(0, 2, 3, 1))
  dy = ec.randn_nhwc((2, 12, H // 2, W // 2), BF16, 3)
  y.backward(dy[..., :12].permute(0, 3, 1, 2))
  assert torch.equal(ec.emu_maxpool_bwd(x, dy)[..., :12], xr.grad.permute(0, 2, 3, 1))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('hw', [(1, 1), (1, 5), (2, 2), (3, 3), (8, 12), (9, 13)])
def test_avgpool_divisor_9_at_a_border_is_rejected(hw, dtype):
  H, W = hw
  x = ec.randn_nhwc((2, 39, H, W), dtype, 11, mean=0.5)
  cands, exact = ec.emu_avgpool_fwd(x, dtype)
  ref = torch.nn.functional.avg_pool2d(x.double().permute(0, 3, 1, 2), 3, 2, 1, count_include_pad=False).permute(0, 2, 3, 1)
  assert (exact - ref).abs().max().item() < 1e-12
  worst, share = ec.candidate_figures(cands[0].float(), cands, exact, dtype)
  assert worst == 0.0 and share == 0.0
  # a correct implementation with another summation order: within one ulp, a small share off the candidates
  other = ec.st(ref.float(), dtype)
  worst, share = ec.candidate_figures(other, cands, exact, dtype)
  assert worst <= 1.0
  bad, _ = ec.emu_avgpool_fwd(ec.int_nhwc((2, 39, H, W), 1, 9, 3), dtype, defect='divisor_9')
  ci, ei = ec.emu_avgpool_fwd(ec.int_nhwc((2, 39, H, W), 1, 9, 3), dtype)
  worst, share = ec.candidate_figures(bad[0].float(), ci, ei, dtype)
  assert worst >= 10.0 and share > ec.CAP, (worst, share)            # most windows of these sizes touch a border
  OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
  dy = ec.randn_nhwc((2, 39, OH, OW), dtype, 12, mean=0.5)
  cb, eb = ec.emu_avgpool_bwd(dy, H, W, dtype)
  xr = torch.zeros((2, 40, H, W), dtype=torch.float64, requires_grad=True)
  torch.nn.functional.avg_pool2d(xr, 3, 2, 1, count_include_pad=False).backward(dy.double().permute(0, 3, 1, 2))
  assert (eb - xr.grad.permute(0, 2, 3, 1)).abs().max().item() < 1e-12
  for c in cb:
    assert ec.candidate_figures(c.float(), cb, eb, dtype) == (0.0, 0.0)
  dyi = ec.int_nhwc((2, 39, OH, OW), 1, 9, 4)
  cb, eb = ec.emu_avgpool_bwd(dyi, H, W, dtype)
  bad, _ = ec.emu_avgpool_bwd(dyi, H, W, dtype, defect='divisor_9')
  worst, share = ec.candidate_figures(bad[0].float(), cb, eb, dtype)
  assert worst >= 10.0 and share > ec.CAP, (worst, share)


# ---- losses ---------------------------------------------------------------------------------------------------------------------
def loss_case(kind, name, dtype, ints):
  if kind == 'mse_const':
    shape = ec.MSE_CONST_SHAPES[name]
    a = ec.int_nhwc(shape, -1, 2, 1) if ints else ec.randn_nhwc(shape, dtype, 3, mean=0.25)
    if ints:
      a.view(-1, 8)[0, 0] = a.view(-1, 8)[-1, 0] = -1.0
    t32, t64 = ec.loss_terms(kind, a, None, 1.0, dtype)
    count = a[..., 0].numel()
  else:
    shape = ec.LOSS_SHAPES[name][dtype]
    a, b = ec.loss_int_pair(shape) if ints else ec.loss_randn_pair(shape, dtype)
    t32, t64 = ec.loss_terms(kind, a, b, 0.0, dtype)
    count = a[..., :shape[1]].numel()
  return t32, t64, count


INT_DEFECTS = {'v1': ['drop_last_vector'],
               'p257': ['drop_last_vector', 'drop_partial', 'dup_partial'],
               'cap': ['drop_last_vector', 'drop_partial', 'dup_partial', 'bf16_acc'],
               'cap_ragged': ['skip_second_sweep', 'drop_partial', 'dup_partial', 'bf16_acc'],
               'cap_ragged_c8': ['drop_last_vector', 'skip_second_sweep', 'drop_partial', 'dup_partial', 'bf16_acc']}


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', ['l1', 'mse'])
@pytest.mark.parametrize('name', list(ec.LOSS_SHAPES))
def test_loss_value_criteria(name, kind, dtype):
  t32, t64, count = loss_case(kind, name, dtype, ints=True)
  ec.assert_exact_terms(t64, name)
  want = ec.loss_value_exact(int(t64.sum().item()), count)
  assert np.float32(ec.emu_loss(t32, count)) == want
  for defect in INT_DEFECTS.get(name, []):
    if defect == 'drop_last_vector' and dtype == F32 and 'c8' not in name and name != 'v1':
      continue                                                       # fp32, C = 3: the last vector holds padding lanes only
    if defect == 'drop_last_vector' and dtype == F32 and name == 'v1':
      continue
    assert np.float32(ec.emu_loss(t32, count, defect)) != want, defect
  t32, t64, count = loss_case(kind, name, dtype, ints=False)
  D = ec.loss_depth(t32.shape[0], t32.shape[1])
  ref, sabs = t64.sum() / count, t64.sum() / count
  used = ec.reduction_used(ec.emu_loss(t32, count), ref, sabs, D)
  assert used <= 0.25, used                                          # a correct fp32 implementation: room to spare
  if name != 'v1':
    assert ec.reduction_used(ec.emu_loss(t32, count, 'bf16_acc'), ref, sabs, D) >= 10.0


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(ec.MSE_CONST_SHAPES))
def test_mse_const_value_criteria(name, dtype):
  t32, t64, count = loss_case('mse_const', name, dtype, ints=True)
  ec.assert_exact_terms(t64, name)
  want = ec.loss_value_exact(int(t64.sum().item()), count)
  assert np.float32(ec.emu_loss(t32, count)) == want
  defects = ['drop_last_vector'] + (['skip_second_sweep', 'drop_partial', 'dup_partial', 'bf16_acc'] if name == 'cap_ragged' else [])
  for defect in defects:
    assert np.float32(ec.emu_loss(t32, count, defect)) != want, defect
  t32, t64, count = loss_case('mse_const', name, dtype, ints=False)
  D = ec.loss_depth(t32.shape[0], 1)
  ref = t64.sum() / count
  assert ec.reduction_used(ec.emu_loss(t32, count), ref, ref, D) <= 0.25
  if name == 'cap_ragged':
    assert ec.reduction_used(ec.emu_loss(t32, count, 'bf16_acc'), ref, ref, D) >= 10.0


@pytest.mark.parametrize('dtype', DTYPES)
def test_loss_gradients_follow_the_fp32_order(dtype):
  shape = ec.LOSS_SHAPES['p257'][dtype]
  a, b = ec.loss_randn_pair(shape, dtype)
  count = a[..., :3].numel()
  g = ec.loss_gscale(0.5, 3.0, count)
  assert float(g) == float(np.float32(0.5) * (np.float32(3.0) / np.float32(count)))
  other = ec.f32(0.5 * 3.0 / count)                                  # the same number formed in double: differs in the last bit
  got = ec.emu_l1_grad(a, b, g, dtype)
  assert set(got[..., :3].unique().tolist()) <= {float(ec.st(g, dtype)), -float(ec.st(g, dtype)), 0.0}
  if float(other) != float(g) and dtype == F32:
    assert ec.bits_differ(ec.emu_l1_grad(a, b, other, dtype), got, dtype) > 0
  m = ec.emu_mse_grad(a, b, g, dtype)
  ref = (2.0 * (a.double() - b.double())) * float(g)
  assert ((m.double() - ref).abs() <= 2.0 * ec.ulp_of(ref, dtype)).all()


# ---- channel_sum ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ec.CSUM_CASES, ids=[c[0] for c in ec.CSUM_CASES])
def test_channel_sum_criteria(case):
  name, dtype, npix, C = case
  Cs = cpad(C)
  geom = ec.csum_geom(dtype, npix, Cs)
  x = ec.csum_inputs(dtype, npix, C, 'int')
  ec.assert_exact_terms(x.abs().sum(0).max(), name)
  want = x.double().sum(0).float()
  assert torch.equal(ec.emu_channel_sum(x, dtype), want)
  defects = ['drop_last_vector'] if Cs - VE[dtype] < C else []       # unless the last vector holds padding lanes only
  if geom['nblk'] >= 5:
    defects.append('drop_group')
  if 'ragged_last_block' in geom['cases']:
    defects.append('drop_ragged_block')
  if npix >= 2000:
    defects.append('bf16_acc')
  for defect in defects:
    got = ec.emu_channel_sum(x, dtype, defect)
    lanes = slice(Cs - VE[dtype], C) if defect == 'drop_last_vector' else slice(0, C)
    assert not torch.equal(got[lanes], want[lanes]), defect
  x = ec.csum_inputs(dtype, npix, C, 'randn')
  D = ec.csum_depth(dtype, npix, Cs)
  ref, sabs = x.double().sum(0)[:C], x.double().abs().sum(0)[:C]
  assert ec.reduction_used(ec.emu_channel_sum(x, dtype)[:C], ref, sabs, D) <= 0.25
  if npix >= 2000:
    assert ec.reduction_used(ec.emu_channel_sum(x, dtype, 'bf16_acc')[:C], ref, sabs, D) >= 10.0


# ---- Adam -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('step', ec.ADAM_STEPS)
def test_adam_criteria(step):
  sc = ec.adam_scalars(step=step, **ec.ADAM_HP)
  for i, n in enumerate(ec.ADAM_SIZES):
    p, g, m, v = ec.adam_inputs(n, 20 + i)
    ref = ec.adam64(p, g, m, v, sc)
    p2, m2, v2 = ec.emu_adam(p, g, m, v, sc)
    used = [ec.adam_used(p2, ref[0], ref[3]), ec.adam_used(m2, ref[1], ref[4]), ec.adam_used(v2, ref[2], ref[5])]
    assert max(used) <= 0.5, (n, used)                               # worst case of every rounding at once is never met
    if n % 4:
      pt, mt, vt = ec.emu_adam(p, g, m, v, sc, defect='drop_tail')
      assert ec.adam_used(pt, ref[0], ref[3]) >= 10.0 and ec.adam_used(mt, ref[1], ref[4]) >= 10.0
      assert ec.adam_used(vt, ref[2], ref[5]) >= 10.0
    if step > 1 and n >= 3:
      bad = ec.adam_scalars(step=step, defect='bias_step_minus_1', **ec.ADAM_HP)
      pb, _, _ = ec.emu_adam(p, g, m, v, bad)
      assert ec.adam_used(pb, ref[0], ref[3]) >= 10.0, (n, step)
  bad = ec.adam_scalars(step=1, defect='bias_step_minus_1', **ec.ADAM_HP)
  assert not np.isfinite(bad['lr1'])                                 # step 1: the defect divides by zero
  # the bf16 panel copy: rn_bf16 of the stored fp32 p, bit for bit -- not of the fp64 p
  p, g, m, v = ec.adam_inputs(4099, 5)
  p2, _, _ = ec.emu_adam(p, g, m, v, sc)
  assert torch.equal(ec.rn_bf16(p2.double()), p2.to(torch.bfloat16).double())


def test_quant_loss_reference_is_the_integer_sum():
  a = (torch.rand(1, 5, 7, 3, generator=ec.G(1)) - 0.5) * 1.3
  b = torch.rand(1, 5, 7, 3, generator=ec.G(2)) - 0.5
  mean, std = [0.5, 0.45, 0.55], [1.0, 0.9, 1.1]
  qa, qb = ec.quant_u8(a, mean, std), ec.quant_u8(b, mean, std)
  assert qa.min() >= 0 and qa.max() <= 255 and qa.min() == 0
  v = ec.quant_loss_value(ec.pad_lanes(a, 3), ec.pad_lanes(b, 3), 3, mean, std, False)
  assert v == np.float32(np.abs(qa - qb).sum() * (1.0 / qa.size))
