"""GPU: every bf16 convolution kernel held to its rounding contract against fp64 arithmetic on its own operands
(tests/bf16_contract.py).  The fp32 suite never reaches these kernels (the dispatchers keep them for 2-byte types), and the bf16
comparisons of tests/test_hip_ops.py measure them against torch-CPU fp32 at 1e-2, several bf16 ulps.

The ops layer is driven directly so that every operand is a known bf16 value: filters are bf16 values before packing (the pack
is exact), the gradient operands are the device's own bf16 tensors (dy, or the dz that ops.act_bwd returns).  Bf16 outputs
(forward, data gradient, fused data gradient) must be a correctly rounded fp64 result of one rounding sequence the kernels
perform; fp32 outputs (weight and bias gradients) carry fp32 summation error only and are held to the fp32 bounds.  Cases and
seeds are those of tests/test_hip_ops.py."""
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import jpdse_hip
from jpdse_hip import ops, BF16, PAD_ZERO, ACT_NONE, ACT_RELU, ACT_LRELU
from jpdse_hip.layers import HipConv2d
import bf16_contract as bc
from bf16_contract import Cand
from hip_util import DEV, to_act, to_nchw
from test_hip_ops import CONV_CASES, FUSED_RELU_CASES, LRELU_CASES

POOL_SHAPES = [(2, 8, 64, 128, 128), (1, 12, 128, 64, 192), (1, 16, 64, 256, 64), (2, 6, 10, 16, 24), (1, 7, 9, 8, 8)]
CONVT_SHAPES = [(2, 128, 64, 5, 7), (1, 1024, 512, 2, 4), (1, 24, 12, 3, 5), (2, 128, 64, 12, 64), (1, 128, 64, 32, 128),
                (2, 256, 128, 8, 64), (1, 512, 256, 4, 128)]
SLICE_SHAPES = [(2, 16, 256), (1, 24, 512), (1, 10, 36)]


def G(seed):
  return torch.Generator().manual_seed(seed)


def q(t):
  return t.to(torch.bfloat16).float()


def dbl(a):
  return to_nchw(a).double()


@pytest.fixture(scope='module', autouse=True)
def _gpu():
  jpdse_hip.require_gpu(0)


def _packs(C, K, k, st, pad, mode, act, w):
  """fwd / data-gradient panels of the KCRS filter w (bf16 values), packed as HipConv2d packs them."""
  d = ops.conv_desc(BF16, 1, 64, 64, C, K, k, k, st, pad, mode, act, bc.SLOPE)
  return ops.conv_pack(d, w.permute(0, 2, 3, 1).contiguous().to(DEV), DEV)


def _wgrad(d, x, dy, K, k, C):
  dw = torch.empty((K, k, k, C), dtype=torch.float32, device=DEV)
  ops.conv_wgrad(d, x, dy, dw)
  return dw


@pytest.mark.parametrize('seed', [0, 1, 2])
@pytest.mark.parametrize('case', CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_bf16_contract(case, seed):
  """Forward (bias and activation in the epilogue), plain data gradient, weight and bias gradient of one layer."""
  name, N, H, W, C, K, k, st, pad, mode, act = case
  x, w, b, gy = bc.conv_case_inputs(case, seed)
  d = ops.conv_desc(BF16, N, H, W, C, K, k, k, st, pad, mode, act, bc.SLOPE)
  fwd_pack, dgr_pack = _packs(C, K, k, st, pad, mode, act, w)
  xa = to_act(x, BF16)
  y = ops.conv_fwd(d, xa, fwd_pack, b.to(DEV))
  dya = to_act(gy, BF16)
  dz = dya if act == ACT_NONE else ops.act_bwd(y, dya, act, bc.SLOPE)
  dx = ops.conv_dgrad(d, dz, dgr_pack)
  dw = _wgrad(d, xa, dz, K, k, C)
  db = torch.zeros(ops.cpad(K), dtype=torch.float32, device=DEV)
  ops.channel_sum(dz, db)
  torch.cuda.synchronize()

  y64, S, n = bc.fwd_reference(x, w, b, st, pad, mode, act)
  bc.assert_bf16_contract(dbl(y), [Cand(y64)], S, n, name + ' fwd')
  dz64 = dbl(dz)
  _, cands, S, n = bc.dgrad_reference(dz64, w.double(), x.shape, st, pad, mode)
  bc.assert_bf16_contract(dbl(dx), cands, S, n, name + ' dgrad')
  bc.assert_fp32_vs_fp64(dw.permute(0, 3, 1, 2).cpu(), bc.wgrad64(x.double(), dz64, w.shape, st, pad, mode), name + ' wgrad')
  bc.assert_fp32_vs_fp64(db[:K].cpu(), dz64.sum(dim=(0, 2, 3)), name + ' bias grad')


def _fused_checks(name, d, dgr_pack, gya, plain, S, n, xa, m, other):
  """Data gradient with the mask of the input's activation and / or the fan-in addend fused: (mask), (mask, addend), (addend)."""
  slope = float(m.min()) if float(m.min()) > 0 else 0.0
  oa = to_act(other, BF16)
  a64 = other.double()
  ones = torch.ones_like(m)
  runs = [('mask', dict(relu_input=xa, mask_slope=slope), torch.zeros_like(a64), m),
          ('mask + addend', dict(relu_input=xa, addend=oa, mask_slope=slope), a64, m),
          ('addend', dict(addend=oa), a64, ones)]
  for label, kw, a, mm in runs:
    got = ops.conv_dgrad(d, gya, dgr_pack, **kw)
    torch.cuda.synchronize()
    bc.assert_bf16_contract(dbl(got), bc.fused_candidates(plain, a, mm), (S + a.abs()) * mm.abs(), n,
                            name + ' dgrad, fused ' + label)


@pytest.mark.parametrize('case', FUSED_RELU_CASES, ids=[c[0] for c in FUSED_RELU_CASES])
def test_conv_dgrad_fused_relu_bf16_contract(case):
  name, N, H, W, C, K, k, st, pad, mode = case
  g = G(zlib.crc32(name.encode()) % 1000 + 7)              # draws of test_hip_ops.py::test_conv_dgrad_fused_relu
  z = q(torch.randn(N, C, H, W, generator=g))
  w = q(torch.randn(K, C, k, k, generator=g) * (1.0 / (C * k * k) ** 0.5))
  oh, ow = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
  gy = q(torch.randn(N, K, oh, ow, generator=g))
  other = q(torch.randn(z.shape, generator=g))
  x = F.relu(z)
  d = ops.conv_desc(BF16, N, H, W, C, K, k, k, st, pad, mode)
  _, dgr_pack = _packs(C, K, k, st, pad, mode, ACT_NONE, w)
  gya = to_act(gy, BF16)
  dx = ops.conv_dgrad(d, gya, dgr_pack)
  torch.cuda.synchronize()
  _, plain, S, n = bc.dgrad_reference(gy.double(), w.double(), x.shape, st, pad, mode)
  bc.assert_bf16_contract(dbl(dx), plain, S, n, name + ' dgrad')
  m = (x > 0).double()
  _fused_checks(name, d, dgr_pack, gya, plain, S, n, to_act(x, BF16), m, other)


@pytest.mark.parametrize('case', LRELU_CASES, ids=[c[0] for c in LRELU_CASES])
def test_conv_dgrad_fused_lrelu_bf16_contract(case):
  name, N, H, W, C, K, k, st, pad, mode = case
  g = G(zlib.crc32(name.encode()) % 1000 + 11)             # draws of test_hip_ops.py::test_conv_dgrad_fused_lrelu
  z = q(torch.randn(N, C, H, W, generator=g))
  w = q(torch.randn(K, C, k, k, generator=g) * (1.0 / (C * k * k) ** 0.5))
  oh, ow = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
  gy = q(torch.randn(N, K, oh, ow, generator=g))
  other = q(torch.randn(z.shape, generator=g))
  x = q(F.leaky_relu(z, bc.SLOPE))
  d = ops.conv_desc(BF16, N, H, W, C, K, k, k, st, pad, mode)
  _, dgr_pack = _packs(C, K, k, st, pad, mode, ACT_NONE, w)
  gya = to_act(gy, BF16)
  _, plain, S, n = bc.dgrad_reference(gy.double(), w.double(), x.shape, st, pad, mode)
  m = torch.where(x > 0, torch.ones_like(x), torch.full_like(x, bc.SLOPE)).double()
  _fused_checks(name, d, dgr_pack, gya, plain, S, n, to_act(x, BF16), m, other)


@pytest.mark.parametrize('shape', POOL_SHAPES, ids=['halo_128', 'halo_64in_ragged', 'halo_n64', 'generic', 'odd'])
def test_conv_fwd_pool_bf16_contract(shape):
  """conv + ReLU with the 2x2 max-pool in the epilogue: y meets the contract, the pooled tensor is the max-pool of y bit for bit."""
  N, H, W, C, K = shape
  g = G(N * 1000 + H * 10 + C)                               # draws of test_hip_ops.py::test_conv_fwd_pool
  w = q(torch.randn(K, C, 3, 3, generator=g) * (2.0 / (C * 9)) ** 0.5)
  b = torch.randn(K, generator=g) * 0.1
  x = q(torch.randn(N, C, H, W, generator=g))
  d = ops.conv_desc(BF16, N, H, W, C, K, 3, 3, 1, 1, PAD_ZERO, ACT_RELU)
  fwd_pack, _ = _packs(C, K, 3, 1, 1, PAD_ZERO, ACT_RELU, w)
  y, yp = ops.conv_fwd_pool(d, to_act(x, BF16), fwd_pack, b.to(DEV))
  torch.cuda.synchronize()
  y64, S, n = bc.fwd_reference(x, w, b, 1, 1, PAD_ZERO, ACT_RELU)
  bc.assert_bf16_contract(dbl(y), [Cand(y64)], S, n, 'conv_fwd_pool %s fwd' % (shape,))
  yn = to_nchw(y)
  assert torch.equal(to_nchw(yp), F.max_pool2d(yn, 2)), 'pooled output is not the max-pool of the stored conv output'


@pytest.mark.parametrize('shape', CONVT_SHAPES)
def test_conv_transpose_bf16_contract(shape):
  """ConvTranspose2d(3, stride 2, pad 1, output_padding 1): its forward is the data gradient of the underlying conv, its data
  gradient that conv's forward; weight gradient in fp32."""
  N, Cin, Cout, H, W = shape
  g = G(Cin + H)                                             # draws of test_hip_ops.py::test_conv_transpose
  x = q(torch.randn(N, Cin, H, W, generator=g))
  w = q(torch.randn(Cin, Cout, 3, 3, generator=g) * (1.0 / (Cin * 9) ** 0.5))     # = the underlying conv's KCRS filter
  gy = q(torch.randn(N, Cout, 2 * H, 2 * W, generator=g))
  d = ops.conv_desc(BF16, N, 2 * H, 2 * W, Cout, Cin, 3, 3, 2, 1, PAD_ZERO)
  fwd_pack, dgr_pack = _packs(Cout, Cin, 3, 2, 1, PAD_ZERO, ACT_NONE, w)
  xa, gya = to_act(x, BF16), to_act(gy, BF16)
  y = ops.conv_dgrad(d, xa, dgr_pack)
  dx = ops.conv_fwd(d, gya, fwd_pack, None)
  dw = _wgrad(d, gya, xa, Cin, 3, Cout)
  torch.cuda.synchronize()
  _, cands, S, n = bc.dgrad_reference(x.double(), w.double(), gy.shape, 2, 1, PAD_ZERO)
  bc.assert_bf16_contract(dbl(y), cands, S, n, 'convT %s fwd' % (shape,))
  dx64, S, n = bc.fwd_reference(gy, w, None, 2, 1, PAD_ZERO, ACT_NONE)
  bc.assert_bf16_contract(dbl(dx), [Cand(dx64)], S, n - 1, 'convT %s dgrad' % (shape,))
  bc.assert_fp32_vs_fp64(dw.permute(0, 3, 1, 2).cpu(), bc.wgrad64(gy.double(), x.double(), w.shape, 2, 1, PAD_ZERO),
                         'convT %s wgrad' % (shape,))


@pytest.mark.parametrize('shape', SLICE_SHAPES)
def test_conv_dgrad_input_slice_bf16_contract(shape):
  """PatchGAN layer 0 (39 -> 64, 4x4 stride 2, bias + LeakyReLU): forward, and the data gradient w.r.t. the 3 image channels
  (HipConv2d.bwd_input_slice) on the device's own dz."""
  N, H, W = shape
  g = G(N * H + W)                                           # draws of test_hip_ops.py::test_conv_dgrad_input_slice
  x = q(torch.randn(N, 39, H, W, generator=g))
  w = q(torch.randn(64, 39, 4, 4, generator=g) * (1.0 / (39 * 16) ** 0.5))
  layer = HipConv2d(39, 64, 4, 2, 2, PAD_ZERO, act=ACT_LRELU, apply_bias=True, dtype=BF16, device=DEV)
  with torch.no_grad():
    layer.weight.copy_(w)
  b = layer.bias.detach().cpu()
  y, ctx = layer.fwd(to_act(x, BF16))
  gy = q(torch.randn(to_nchw(y).shape, generator=g))
  dz = ops.act_bwd(y, to_act(gy, BF16), ACT_LRELU, bc.SLOPE)
  dx = layer.bwd_input_slice(ctx, dz, 36, 39, dy_is_dz=True)
  torch.cuda.synchronize()
  y64, S, n = bc.fwd_reference(x, w, b, 2, 2, PAD_ZERO, ACT_LRELU)
  bc.assert_bf16_contract(dbl(y), [Cand(y64)], S, n, 'layer-0 %s fwd' % (shape,))
  _, cands, S, n = bc.dgrad_reference(dbl(dz), w[:, 36:39].double(), (N, 3, H, W), 2, 2, PAD_ZERO)
  bc.assert_bf16_contract(dbl(dx), cands, S, n, 'layer-0 %s data gradient, image channels' % (shape,))
