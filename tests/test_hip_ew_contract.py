"""The kernels of csrc/elementwise.hip against their contracts (tests/ew_contract.py; the criteria themselves are checked on the
CPU by tests/test_ew_contract_host.py): bit-exact maps, fused / unfused candidates, reductions that are exact on integer inputs
and within D u sum|terms| of fp64 on randn inputs, Adam within k u (|value| + |update terms|) of fp64 -- at the smallest shapes
that reach each path: one vector, a ragged block, a partial second grid-stride sweep counted in each kernel's own work items, the 1024-partial cap of the loss first
stage, every branch of the channel_sum geometry, and the block-ownership search and scalar path of the Adam kernel."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jpdse_hip
from jpdse_hip import ops, F32, BF16, ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH
from jpdse_hip.ops import Act
from jpdse_hip.optim import FusedAdam
from hip_util import DEV, DTYPES, record
import ew_contract as ec
from ew_contract import cpad, tdtype, edge_y, plateau, SUB, MAP_CASES


@pytest.fixture(scope='module', autouse=True)
def _gpu():
  jpdse_hip.require_gpu(0)


def dev(t, C, dtype):
  """fp32 CPU NHWC storage values -> Act on the device (exact: the values are representable)."""
  return Act(t.to(tdtype(dtype)).to(DEV).contiguous(), C)


def host(t):
  torch.cuda.synchronize()
  return t.detach().cpu()


def check_map(got, want, C, dtype, what):
  g = host(got.t if isinstance(got, Act) else got)
  ec.assert_bits_equal(g, want, what, dtype)
  ec.assert_pad_zero(g, C, what)


# ---- grid-stride maps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', MAP_CASES)
def test_add_and_act_bwd(case, dtype):
  shape = ec.map_shapes(dtype)[case]
  C = shape[1]
  y, dy = edge_y(shape, dtype, 1), ec.randn_nhwc(shape, dtype, 2)
  Y, DY = dev(y, C, dtype), dev(dy, C, dtype)
  check_map(ops.add(Y, DY), ec.emu_add(y, dy, dtype), C, dtype, 'add')
  for act, name in ((ACT_RELU, 'relu'), (ACT_LRELU, 'lrelu'), (ACT_NONE, 'none')):
    check_map(ops.act_bwd(Y, DY, act, ec.SLOPE), ec.emu_act_bwd(y, dy, act, dtype), C, dtype, 'act_bwd ' + name)
  yt = edge_y(shape, dtype, 3, tanh=True)
  got = host(ops.act_bwd(dev(yt, C, dtype), DY, ACT_TANH).t)
  cands, exact = ec.tanh_bwd_candidates(yt, dy, dtype)
  ec.assert_candidates(got, cands, exact, dtype, 'act_bwd tanh')
  ec.assert_pad_zero(got, C, 'act_bwd tanh')
  n = got.view(-1, got.shape[-1]).shape[0]
  assert (got.view(-1, got.shape[-1])[n - 1, :2] == 0).all(), '|y| = 1: the gradient vanishes exactly'


def pool_in_shape(out_shape, odd):
  N, C, H, W = out_shape
  return (N, C, 2 * H - (1 if odd else 0), 2 * W - (1 if odd else 0))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', MAP_CASES)
def test_avgpool_grid_stride(case, dtype):
  """Forward: the enumerated tensor is the output; backward: the input gradient."""
  shape = ec.map_shapes(dtype)[case]
  N, C, H, W = shape
  x = ec.randn_nhwc(pool_in_shape(shape, odd=(case != 'cap')), dtype, 4, mean=0.5)
  got = ops.avgpool3s2_fwd(dev(x, C, dtype))
  assert tuple(got.t.shape[1:3]) == (H, W)
  cands, exact = ec.emu_avgpool_fwd(x, dtype)
  ec.assert_candidates(host(got.t), cands, exact, dtype, 'avgpool3s2_fwd')
  ec.assert_pad_zero(host(got.t), C, 'avgpool3s2_fwd')
  dy = ec.randn_nhwc((N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype, 5, mean=0.5)
  got = host(ops.avgpool3s2_bwd(dev(dy, C, dtype), H, W).t)
  cands, exact = ec.emu_avgpool_bwd(dy, H, W, dtype)
  ec.assert_candidates(got, cands, exact, dtype, 'avgpool3s2_bwd')
  ec.assert_pad_zero(got, C, 'avgpool3s2_bwd')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('hw', [(1, 1), (1, 5), (2, 2), (3, 3), (8, 12), (9, 13)])
def test_avgpool_borders(hw, dtype):
  H, W = hw
  for ints in (True, False):
    x = ec.int_nhwc((2, 39, H, W), 1, 9, 3) if ints else ec.randn_nhwc((2, 39, H, W), dtype, 6, mean=0.5)
    cands, exact = ec.emu_avgpool_fwd(x, dtype)
    got = host(ops.avgpool3s2_fwd(dev(x, 39, dtype)).t)
    ec.assert_candidates(got, cands, exact, dtype, 'avgpool3s2_fwd')
    ec.assert_pad_zero(got, 39, 'avgpool3s2_fwd')
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = ec.int_nhwc((2, 39, OH, OW), 1, 9, 4) if ints else ec.randn_nhwc((2, 39, OH, OW), dtype, 7, mean=0.5)
    cands, exact = ec.emu_avgpool_bwd(dy, H, W, dtype)
    got = host(ops.avgpool3s2_bwd(dev(dy, 39, dtype), H, W).t)
    ec.assert_candidates(got, cands, exact, dtype, 'avgpool3s2_bwd')
    ec.assert_pad_zero(got, 39, 'avgpool3s2_bwd')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', MAP_CASES)
def test_maxpool_grid_stride(case, dtype):
  """Forward: the output is enumerated; backward: the windows (even sizes) or the pixels (odd sizes) of the input."""
  shape = ec.map_shapes(dtype)[case]
  N, C, H, W = shape
  x = ec.randn_nhwc((N, C, 2 * H, 2 * W + (1 if case.startswith('ragged') else 0)), dtype, 8)
  X = dev(x, C, dtype)
  check_map(ops.maxpool2_fwd(X), ec.emu_maxpool_fwd(x), C, dtype, 'maxpool2_fwd')
  dy = ec.randn_nhwc(shape, dtype, 9)
  check_map(ops.maxpool2_bwd(X, dev(dy, C, dtype)), ec.emu_maxpool_bwd(x, dy), C, dtype, 'maxpool2_bwd')
  if case != 'cap':
    return
  # the window kernel ran past the cap above (520 x 512); the per-pixel kernel past it: odd sizes, 261 x 255 pixels = 532440 vectors
  for hw, seed in (((261, 255), 10),):
    x = ec.randn_nhwc((N, C) + hw, dtype, seed)
    dy = ec.randn_nhwc((N, C, hw[0] // 2, hw[1] // 2), dtype, seed + 1)
    check_map(ops.maxpool2_bwd(dev(x, C, dtype), dev(dy, C, dtype)), ec.emu_maxpool_bwd(x, dy), C, dtype, 'maxpool2_bwd %dx%d' % hw)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('hw', [(8, 12), (9, 13), (2, 2), (3, 2)])
def test_maxpool_ties_go_to_the_first_element(hw, dtype):
  H, W = hw
  for per_window in (True, False):
    x = plateau((2, 12, H, W), per_window)
    dy = ec.int_nhwc((2, 12, H // 2, W // 2), 1, 5, 9)
    X = dev(x, 12, dtype)
    check_map(ops.maxpool2_fwd(X), ec.emu_maxpool_fwd(x), 12, dtype, 'maxpool2_fwd plateau')
    want = ec.emu_maxpool_bwd(x, dy)
    assert torch.equal(want[:, 0:2 * (H // 2):2, 0:2 * (W // 2):2], dy)
    check_map(ops.maxpool2_bwd(X, dev(dy, 12, dtype)), want, 12, dtype, 'maxpool2_bwd plateau')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', MAP_CASES)
def test_channel_moves_and_layout(case, dtype):
  shape = ec.map_shapes(dtype)[case]
  N, C, H, W = shape
  base = ec.randn_nhwc(shape, dtype, 12)
  nch = min(3, C)
  c0 = C - nch if case != 'cap' else C - nch - 2          # cap: channels [C-5, C-2) straddle no vector edge in bf16, one in fp32
  img = ec.randn_nhwc((N, nch, H, W), dtype, 13)
  B, I = dev(base, C, dtype), dev(img, nch, dtype)
  out = Act(torch.full_like(B.t, 7.0), C)                 # every lane must be written
  ops.concat_channels(B, I, c0, out)
  want = ec.emu_concat_channels(base, img, c0, nch)
  check_map(out, want, C, dtype, 'concat_channels')
  dst = Act(B.t.clone(), C)
  ops.insert_channels(dst, I, c0)
  check_map(dst, want, C, dtype, 'insert_channels')
  dst = Act(B.t.clone(), C)
  ops.channel_copy(I, 0, dst, c0, nch)
  check_map(dst, want, C, dtype, 'channel_copy')
  if case == 'cap':
    # the two kernels above enumerate npix * nch elements and npix * (vectors touched): one sweep each with three channels.
    # Past the cap: 8 channels per pixel copied (532480 items); the whole image inserted at channel 4 of a destination that
    # is 8 channels wider (9 vectors per pixel in bf16, 8 in fp32), whose other lanes must survive the read-modify-write
    npix, nw = N * H * W, ec.WIDE_COPY_NCH
    assert ec.grid_stride_sweeps(ec.channel_copy_items(npix, nw)) == 2
    dst = Act(B.t.clone(), C)
    ops.channel_copy(B, 3, dst, C - nw - 3, nw)
    want = base.clone()
    want[..., C - nw - 3:C - 3] = base[..., 3:3 + nw]
    check_map(dst, want, C, dtype, 'channel_copy 8 channels')
    c0w = ec.WIDE_INSERT_C0
    assert ec.grid_stride_sweeps(ec.insert_channels_items(dtype, npix, c0w, C)) == 2
    wide = ec.randn_nhwc((N, C + 8, H, W), dtype, 15)
    dst = dev(wide, C + 8, dtype)
    ops.insert_channels(dst, B, c0w)
    check_map(dst, ec.emu_concat_channels(wide, base, c0w, C), C + 8, dtype, 'insert_channels whole image')
  # layout: fp32 NCHW -> NHWC storage (one RNE) and back (exact)
  src = torch.randn((N, C, H, W), generator=ec.G(14))
  a = ops.nchw_to_nhwc(src.to(DEV).contiguous(), dtype)
  check_map(a, ec.emu_nchw_to_nhwc(src, dtype), C, dtype, 'nchw_to_nhwc')
  back = host(ops.nhwc_to_nchw(B))
  ec.assert_bits_equal(back, ec.emu_nhwc_to_nchw(base, C), 'nhwc_to_nchw', F32)


def test_cast_and_copy():
  n = ec.CAST_N
  x = torch.randn(n, generator=ec.G(15)) * torch.exp(torch.randn(n, generator=ec.G(16)) * 4)
  x[:4] = torch.tensor([0.0, -0.0, SUB, 1.0 + 2.0 ** -8])           # the last one: a midpoint, rounds to even
  X = x.to(DEV)
  y = torch.full((n,), 7.0, dtype=torch.bfloat16, device=DEV)
  ops.cast_(X, y)
  ec.assert_bits_equal(host(y), x.to(torch.bfloat16), 'cast fp32 -> bf16')
  z = torch.full((n,), 7.0, dtype=torch.float32, device=DEV)
  ops.cast_(y, z)
  ec.assert_bits_equal(host(z), x.to(torch.bfloat16).float(), 'cast bf16 -> fp32')
  c = torch.full((n,), 7.0, dtype=torch.bfloat16, device=DEV)
  ops.copy_(y, c)
  ec.assert_bits_equal(host(c), host(y), 'copy (524291 vectors)')
  for m in (4, 4 * 7):                                               # one vector; seven
    s = X[:m].clone()
    d = torch.full_like(s, 7.0)
    ops.copy_(s, d)
    ec.assert_bits_equal(host(d), x[:m], 'copy (small)')


# ---- losses ---------------------------------------------------------------------------------------------------------------------
def run_twice(fn):
  a = fn()
  b = fn()
  torch.cuda.synchronize()
  return a, b


def loss_values(A, B):
  """[l1_fwd, mse_fwd, l1_fwd_bwd, l1_fwd_bwd relu_a] immediate, the same four deferred, and the two fused gradients."""
  out = torch.zeros(8, dtype=torch.float32, device=DEV)
  ops.l1_fwd(A, B, out[0:1])
  ops.mse_fwd(A, B, out[1:2])
  g0 = ops.l1_fwd_bwd(A, B, out[2:3], 2.5, relu_a=False)
  g1 = ops.l1_fwd_bwd(A, B, out[3:4], 2.5, relu_a=True)
  with ops.deferred_loss_finals():
    ops.l1_fwd(A, B, out[4:5])
    ops.mse_fwd(A, B, out[5:6])
    ops.l1_fwd_bwd(A, B, out[6:7], 2.5, relu_a=False)
    ops.l1_fwd_bwd(A, B, out[7:8], 2.5, relu_a=True)
  torch.cuda.synchronize()
  return out.cpu(), g0, g1


LOSS_NAMES = ['l1_fwd', 'mse_fwd', 'l1_fwd_bwd', 'l1_fwd_bwd relu_a']


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(ec.LOSS_SHAPES))
def test_loss_values_and_gradients(name, dtype):
  shape = ec.LOSS_SHAPES[name][dtype]
  C = shape[1]
  for ints in (True, False):
    a, b = ec.loss_int_pair(shape) if ints else ec.loss_randn_pair(shape, dtype)
    if not ints:
      a.view(-1, a.shape[-1])[0, :2] = torch.tensor([0.0, -0.0])     # the ReLU mask's edge: a == 0 is dead
    count = a[..., :C].numel()
    terms = {'l1': ec.loss_terms('l1', a, b, 0.0, dtype), 'mse': ec.loss_terms('mse', a, b, 0.0, dtype)}
    kinds = ['l1', 'mse', 'l1', 'l1']
    if ints:
      for k in terms:
        ec.assert_exact_terms(terms[k][1], k)                        # on the CPU, before any device work
    A, B = dev(a, C, dtype), dev(b, C, dtype)
    (v1, g0, g1), (v2, _, _) = run_twice(lambda: loss_values(A, B))
    assert torch.equal(v1, v2), 'a second evaluation differs'
    assert torch.equal(v1[:4], v1[4:]), 'deferred finals differ from the immediate ones'
    for i, kind in enumerate(kinds):
      t32, t64 = terms[kind]
      what = LOSS_NAMES[i] + (' int' if ints else ' randn')
      if ints:
        want = ec.loss_value_exact(int(t64.sum().item()), count)
        record(what + ' [integer-exact: |got - want|]', abs(float(v1[i]) - float(want)), 0.0)
        assert np.float32(v1[i].item()) == want, (what, float(v1[i]), float(want))
      else:
        D = ec.loss_depth(t32.shape[0], t32.shape[1])
        ec.assert_reduction(v1[i], t64.sum() / count, t64.sum() / count, D, what)
    # gradients: bit-exact, gscale = scale / float(count)
    g = ec.loss_gscale(1.0, 2.5, count)
    check_map(g0, ec.emu_l1_grad(a, b, g, dtype), C, dtype, 'l1_fwd_bwd gradient')
    check_map(g1, ec.emu_l1_grad(a, b, g, dtype, relu_a=True), C, dtype, 'l1_fwd_bwd gradient relu_a')
    if name in ('v1', 'p257', 'cap_ragged'):
      gout = torch.full((1,), 0.75, device=DEV)
      g = ec.loss_gscale(0.75, 3.0, count)
      check_map(ops.l1_bwd(A, B, gout, 3.0), ec.emu_l1_grad(a, b, g, dtype), C, dtype, 'l1_bwd')
      check_map(ops.l1_bwd(A, B, gout, 3.0, relu_a=True), ec.emu_l1_grad(a, b, g, dtype, relu_a=True), C, dtype, 'l1_bwd_relu')
      check_map(ops.mse_bwd(A, B, gout, 3.0), ec.emu_mse_grad(a, b, g, dtype), C, dtype, 'mse_bwd')


@pytest.mark.parametrize('dtype', DTYPES)
def test_loss_gradients_past_the_cap(dtype):
  """l1_bwd, l1_bwd_relu and mse_bwd are grid-stride maps over the tensor's vectors: 532480 of them, a partial second sweep."""
  shape = ec.map_shapes(dtype)['cap']
  C = shape[1]
  a, b = edge_y(shape, dtype, 21), ec.randn_nhwc(shape, dtype, 22)
  count = a[..., :C].numel()
  assert ec.grid_stride_sweeps(a.numel() // ec.VE[dtype]) == 2
  A, B = dev(a, C, dtype), dev(b, C, dtype)
  gout = torch.full((1,), 0.75, device=DEV)
  g = ec.loss_gscale(0.75, 3.0, count)
  check_map(ops.l1_bwd(A, B, gout, 3.0), ec.emu_l1_grad(a, b, g, dtype), C, dtype, 'l1_bwd')
  check_map(ops.l1_bwd(A, B, gout, 3.0, relu_a=True), ec.emu_l1_grad(a, b, g, dtype, relu_a=True), C, dtype, 'l1_bwd_relu')
  check_map(ops.mse_bwd(A, B, gout, 3.0), ec.emu_mse_grad(a, b, g, dtype), C, dtype, 'mse_bwd')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(ec.MSE_CONST_SHAPES))
def test_mse_const(name, dtype):
  shape = ec.MSE_CONST_SHAPES[name]
  for ints in (True, False):
    x = ec.int_nhwc(shape, -1, 2, 1) if ints else ec.randn_nhwc(shape, dtype, 3, mean=0.25)
    if ints:
      x.view(-1, 8)[0, 0] = x.view(-1, 8)[-1, 0] = -1.0
    t32, t64 = ec.loss_terms('mse_const', x, None, 1.0, dtype)
    count = t32.shape[0]
    if ints:
      ec.assert_exact_terms(t64, name)
    X = dev(x, 1, dtype)

    def values():
      out = torch.zeros(2, dtype=torch.float32, device=DEV)
      ops.mse_const_fwd(X, 1.0, out[0:1])
      with ops.deferred_loss_finals():
        ops.mse_const_fwd(X, 1.0, out[1:2])
      torch.cuda.synchronize()
      return out.cpu()
    v1, v2 = run_twice(values)
    assert torch.equal(v1, v2) and v1[0] == v1[1]
    what = 'mse_const_fwd' + (' int' if ints else ' randn')
    if ints:
      want = ec.loss_value_exact(int(t64.sum().item()), count)
      record(what + ' [integer-exact: |got - want|]', abs(float(v1[0]) - float(want)), 0.0)
      assert np.float32(v1[0].item()) == want, (float(v1[0]), float(want))
    else:
      ec.assert_reduction(v1[0], t64.sum() / count, t64.sum() / count, ec.loss_depth(count, 1), what)
    gout = torch.full((1,), 0.75, device=DEV)
    got = ops.mse_const_bwd(X, 1.0, gout, 2.0)
    check_map(got, ec.emu_mse_const_grad(x, 1.0, ec.loss_gscale(0.75, 2.0, count), dtype), 1, dtype, 'mse_const_bwd')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C', [1, 3])
def test_quant_loss_past_the_cap(C, dtype):
  """266240 pixels: 1024 partials and a ragged second sweep; a in either storage type, b in fp32; integer-exact in double."""
  shape = (1, C, 520, 512)
  a = ec.pad_lanes(ec.st((torch.rand((1, 520, 512, C), generator=ec.G(5)) - 0.5) * 1.3, dtype), C)
  b = ec.pad_lanes(torch.rand((1, 520, 512, C), generator=ec.G(6)) - 0.5, C)
  a.view(-1, 8)[-1, :C] = 0.5
  b.view(-1, 8)[-1, :C] = -0.5                                       # the last pixel carries the largest term
  mean, std = [0.5, 0.45, 0.55][:C], [1.0, 0.9, 1.1][:C]
  A, B = dev(a, C, dtype), dev(b, C, F32)
  for mse in (False, True):
    def value():
      slot = torch.zeros(1, dtype=torch.float32, device=DEV)
      ops.quant_loss(A, B, mean, std, mse, slot)
      return slot.cpu()
    v1, v2 = run_twice(value)
    want = ec.quant_loss_value(a, b, C, mean, std, mse)
    record('quant_loss %s [integer-exact: |got - want|]' % ('mse' if mse else 'l1'), abs(float(v1) - float(want)), 0.0)
    assert torch.equal(v1, v2) and np.float32(v1.item()) == want, (float(v1), float(want))


# ---- channel_sum ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ec.CSUM_CASES, ids=[c[0] for c in ec.CSUM_CASES])
def test_channel_sum(case):
  name, dtype, npix, C = case
  Cs = cpad(C)
  for kind in ('int', 'randn'):
    x = ec.csum_inputs(dtype, npix, C, kind)
    if kind == 'int':
      ec.assert_exact_terms(x.abs().sum(0).max(), name)
    X = dev(x.view(1, 1, npix, Cs), C, dtype)

    def value():
      out = torch.full((Cs,), 7.0, dtype=torch.float32, device=DEV)
      ops.channel_sum(X, out)
      return out.cpu()
    v1, v2 = run_twice(value)
    assert torch.equal(v1, v2), 'a second evaluation differs'
    assert (v1[C:] == 0).all(), 'sums of the padding lanes'
    if kind == 'int':
      ec.assert_bits_equal(v1, x.double().sum(0).float(), 'channel_sum int', F32)
    else:
      ec.assert_reduction(v1[:C], x.double().sum(0)[:C], x.double().abs().sum(0)[:C], ec.csum_depth(dtype, npix, Cs),
                          'channel_sum randn')


# ---- Adam -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('step', ec.ADAM_STEPS)
@pytest.mark.parametrize('n_entries', ec.ADAM_TABLES)
def test_adam(n_entries, step):
  """FusedAdam over a table of n_entries tensors of the sizes 1 .. 4099 (every third entry writes the bf16 panel copy; entry 1,
  or the only one, is a view that starts one element into its storage: the unaligned scalar path), grad_scale = 1/3, the step
  counter set to step - 1."""
  hp = ec.ADAM_HP
  cpu, params, casts = [], [], {}
  for i in range(n_entries):
    n = ec.ADAM_SIZES[(i + n_entries) % len(ec.ADAM_SIZES)]
    p, g, m, v = ec.adam_inputs(n, 100 * n_entries + i)
    cpu.append((p, g, m, v))
    unaligned = i == min(1, n_entries - 1)
    def place(t):
      if not unaligned:
        return t.to(DEV)
      buf = torch.zeros(n + 1, dtype=torch.float32, device=DEV)
      buf[1:] = t.to(DEV)
      return buf[1:]
    q = torch.nn.Parameter(place(p))
    q.grad = place(g)
    if unaligned:
      assert q.data_ptr() % 16 == 4
    if i % 3 == 0 or unaligned:
      casts[i] = torch.full((n,), 7.0, dtype=torch.bfloat16, device=DEV)
      q._jpdse_cast_out = casts[i]
    params.append(q)
  opt = FusedAdam(params, lr=hp['lr'], betas=(hp['beta1'], hp['beta2']), eps=hp['eps'], grad_scale=hp['grad_scale'])
  for q, (p, g, m, v) in zip(params, cpu):
    st = opt._ensure_state(q)
    st['step'] = torch.tensor(float(step - 1), dtype=torch.float32)
    st['exp_avg'].copy_(m.to(DEV))
    st['exp_avg_sq'].copy_(v.to(DEV))
  opt.step()
  torch.cuda.synchronize()
  sc = ec.adam_scalars(step=step, **hp)
  for i, (q, (p, g, m, v)) in enumerate(zip(params, cpu)):
    st = opt.state[q]
    assert float(st['step']) == step
    p2 = q.detach().cpu()
    ec.assert_adam(p2, st['exp_avg'].cpu(), st['exp_avg_sq'].cpu(), ec.adam64(p, g, m, v, sc), 'adam')
    ec.assert_bits_equal(host(q.grad), g, 'adam: gradient untouched', F32)
    if i in casts:
      ec.assert_bits_equal(host(casts[i]), p2.to(torch.bfloat16), 'adam: bf16 panel copy = rn_bf16(stored p)')


def test_adam_step_direct_table():
  """jpdse_adam_step on a hand-built table FusedAdam cannot express: two entries that share no allocation pattern of torch's --
  the second entry's m and v (not its p) start one element into their storage, and only the first has a panel copy."""
  from jpdse_hip import AdamEntry, lib, check
  hp = ec.ADAM_HP
  sizes, tens, entries, block0 = [1025, 4099], [], [], 0
  for i, n in enumerate(sizes):
    cpu = ec.adam_inputs(n, 300 + i)
    d = []
    for j, t in enumerate(cpu):
      buf = torch.zeros(n + 1, dtype=torch.float32, device=DEV)
      off = 1 if (i == 1 and j >= 2) else 0
      buf[off:off + n] = t.to(DEV)
      d.append(buf[off:off + n])
    cast = torch.full((n,), 7.0, dtype=torch.bfloat16, device=DEV) if i == 0 else None
    entries.append(AdamEntry(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, block0,
                             cast.data_ptr() if cast is not None else None))
    block0 += (n + 1023) // 1024
    tens.append((cpu, d, cast))
  arr = (AdamEntry * len(entries))(*entries)
  table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
  check(lib().jpdse_adam_step(ctypes.c_void_p(table.data_ptr()), len(entries), block0, hp['lr'], hp['beta1'], hp['beta2'],
                              hp['eps'], 2, hp['grad_scale'], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
        'adam_step')
  torch.cuda.synchronize()
  sc = ec.adam_scalars(step=2, **hp)
  for cpu, d, cast in tens:
    p2 = d[0].cpu()
    ec.assert_adam(p2, d[2].cpu(), d[3].cpu(), ec.adam64(*cpu, sc), 'adam (direct table)')
    if cast is not None:
      ec.assert_bits_equal(host(cast), p2.to(torch.bfloat16), 'adam (direct table): bf16 panel copy')
