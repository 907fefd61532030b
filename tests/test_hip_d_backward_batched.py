"""The PatchGAN's backward walked once for loss_G and loss_D: 3B gradient images
[loss_G on fake ; loss_D on fake ; loss_D on real] over the saved forward of 2B images.

Every kernel that resolves the image classes -- gradient image n >= B reads the saved operands of image n - B, only images
n < B take the feature-matching addend -- is called batched and compared, bit for bit, with the same kernel called without
aliasing: on the B and the 2B part separately where those calls take the batched call's route, otherwise on the 3B batch with
the operands written out per image (same N, hence the same route and tiles).  Then the whole discriminator: the batched
walk against the two walks."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import jpdse_hip
from jpdse_hip import ops, BF16, ACT_NONE, ACT_LRELU, PAD_ZERO
from jpdse_hip.ops import Act
from jpdse_hip.layers import HipConv2d
from ctu.models.pix2pixHD_networks import networks
from hip_util import DEV


def _rand(N, H, W, C, seed, scale=1.0):
  g = torch.Generator().manual_seed(seed)
  t = (torch.randn(N, H, W, ops.cpad(C), generator=g) * scale)
  t[..., C:] = 0
  return Act(t.to(DEV, torch.bfloat16).contiguous(), C)


def _cat(*acts):
  return Act(torch.cat([a.t for a in acts]).contiguous(), acts[0].C)


def _same(a, b, what):
  torch.cuda.synchronize()
  assert a.t.shape == b.t.shape, what
  # bit patterns, so that -0 / +0 and NaN payloads count
  bad = (a.t.view(torch.int16) != b.t.view(torch.int16))
  assert not bool(bad.any()), '%s: %d of %d elements differ' % (what, int(bad.sum()), bad.numel())


def _dgrad_route(d, flags):
  """Name of the data-gradient route of `d` under the shipped dispatch (developer build, mode 1: the same choice)."""
  with jpdse_hip.dev_mode(1) as dev:
    out = (ctypes.c_int32 * 3)()
    jpdse_hip.check(dev.jpdse_debug_conv_route(ctypes.byref(d), flags, out), 'conv_route')
    return dev.jpdse_debug_route_name(1, out[1]).decode()


# (what, C, K, k, stride, x grid, mask: False | True (LeakyReLU 0.2) | 0.0 (ReLU), route the 3B call must take)
CONV_CASES = [
    ('4x4 s2 64->128 small', 64, 128, 4, 2, (17, 33), True, 'generic'),
    ('4x4 s2 128->256 small', 128, 256, 4, 2, (17, 33), False, 'generic'),
    ('4x4 s2 64->128 fast', 64, 128, 4, 2, (65, 129), True, 'fast'),       # 2145 rows per image and phase: tiles straddle n = B, 2B
    ('4x4 s2 128->256 fast', 128, 256, 4, 2, (65, 97), False, 'fast'),     # 1617 rows per image and phase
    ('4x4 s1 128->256 taps4', 128, 256, 4, 1, (17, 33), False, 'taps4'),   # 16 x 32 core + fringe through the split-K finish
    # with a ReLU mask (slope 0): the mask alias of the tap-program kernel (core) and of the split-K finish (fringe)
    ('4x4 s1 128->256 taps4 masked', 128, 256, 4, 1, (17, 33), 0.0, 'taps4'),
    ('4x4 s1 128->1 head', 128, 1, 4, 1, (9, 17), False, 'thin1'),         # dy 10 x 18
    ('4x4 s1 256->1 head', 256, 1, 4, 1, (9, 17), False, 'thin1'),
]


@pytest.mark.parametrize('B', [1, 2])
@pytest.mark.parametrize('case', CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_dgrad_batched_equals_unbatched(case, B):
  what, C, K, k, st, (H, W), masked, want_route = case
  conv = HipConv2d(C, K, k, st, 2, PAD_ZERO, apply_bias=False, dtype=BF16, device=DEV)
  _, pack = conv.packs()
  slope, masked = (0.2, masked) if isinstance(masked, bool) else (masked, True)
  desc = lambda n: conv._desc(n, H, W)
  oh, ow = ops.conv_out_shape(desc(1))
  flags = (4 if masked else 0) | (16 if slope else 0) | 8
  route = {n: _dgrad_route(desc(n), flags if n != 2 * B else flags & ~8) for n in (B, 2 * B, 3 * B)}
  assert route[3 * B] == want_route, (what, route)
  dy = _rand(3 * B, oh, ow, K, 1)
  x = _rand(2 * B, H, W, C, 2) if masked else None      # the saved LeakyReLU output: its sign is the mask
  addend = _rand(B, H, W, C, 3)
  got = ops.conv_dgrad_batched(desc(3 * B), dy, pack, B, relu_input=x, addend=addend, mask_slope=slope)
  if route[B] == route[2 * B] == route[3 * B] and want_route != 'taps4':
    # (the fringe of the taps4 route is a split-K GEMM whose split count follows N: one N for both sides there)
    g_part = ops.conv_dgrad(desc(B), dy.batch_slice(0, B), pack, relu_input=x.batch_slice(0, B) if masked else None,
                            addend=addend, mask_slope=slope)
    d_part = ops.conv_dgrad(desc(2 * B), dy.batch_slice(B, 3 * B), pack, relu_input=x, mask_slope=slope)
  else:
    xx = _cat(x.batch_slice(0, B), x) if masked else None
    with_add = ops.conv_dgrad(desc(3 * B), dy, pack, relu_input=xx, addend=_cat(addend, addend, addend), mask_slope=slope)
    if masked:
      without = ops.conv_dgrad(desc(3 * B), dy, pack, relu_input=xx, mask_slope=slope)
    else:
      without = ops.conv_dgrad(desc(3 * B), dy, pack)
    g_part, d_part = with_add.batch_slice(0, B), without.batch_slice(B, 3 * B)
  _same(got.batch_slice(0, B), g_part, what + ': loss_G images')
  _same(got.batch_slice(B, 3 * B), d_part, what + ': loss_D images')


@pytest.mark.parametrize('B', [1, 2])
@pytest.mark.parametrize('three_kernels', [False, True], ids=['rows', 'moment-finalize-apply'])
@pytest.mark.parametrize('C', [128, 256])
def test_inorm_bwd_aliased_equals_unaliased(C, three_kernels, B):
  H, W = 9, 17
  x = _rand(2 * B, H, W, C, 4, scale=2.0)
  dy = _rand(3 * B, H, W, C, 5)

  def run():
    _, stats = ops.inorm_fwd(x, ACT_LRELU, 0.2)
    got = ops.inorm_bwd_aliased(x, stats, dy, B, ACT_LRELU, 0.2)
    g_part = ops.inorm_bwd(x.batch_slice(0, B), stats[:B], dy.batch_slice(0, B), ACT_LRELU, 0.2)
    d_part = ops.inorm_bwd(x, stats, dy.batch_slice(B, 3 * B), ACT_LRELU, 0.2)
    _same(got.batch_slice(0, B), g_part, 'inorm bwd: loss_G images')
    _same(got.batch_slice(B, 3 * B), d_part, 'inorm bwd: loss_D images')

  if three_kernels:
    with jpdse_hip.dev_mode(27):      # InstanceNorm always as moment -> finalize -> apply (the large tensors' form)
      run()
  else:
    run()


@pytest.mark.parametrize('B', [1, 2])
def test_discriminator_batched_walk_equals_two_walks(B):
  torch.manual_seed(7)
  label_nc, H, W = 36, 64, 128
  netD = networks.define_D(label_nc + 3, 16, 3, 'instance', False, 2, True, gpu_ids=[0], compute_dtype='bf16')
  for m in netD.modules():
    if hasattr(m, 'ensure_grads'):
      m.ensure_grads()
  x = _rand(2 * B, H, W, label_nc + 3, 11)
  pred, ctx = netD.fwd(x)
  one = torch.ones(1, dtype=torch.float32, device=DEV)
  dfeats = [[ops.l1_bwd(f.batch_slice(0, B), f.batch_slice(B, 2 * B), one, 5.0) for f in feats[:-1]] for feats in pred]
  heads = lambda p: (ops.mse_const_bwd(p.batch_slice(0, B), 1.0, one, 1.0), ops.mse_const_bwd(p.batch_slice(0, B), 0.0, one, 0.5),
                     ops.mse_const_bwd(p.batch_slice(B, 2 * B), 1.0, one, 0.5))
  dheads = [heads(feats[-1]) for feats in pred]
  chans = (label_nc, label_nc + 3)

  # the two walks: loss_G through the fake half (data gradients only), loss_D through the whole batch
  dx_two = netD.bwd(ctx, [dfeats[i] + [dheads[i][0]] for i in range(2)], need_dx=True, need_dw=False, batch=(0, B),
                    dx_channels=chans)
  netD.bwd(ctx, [[None] * len(dfeats[i]) + [_cat(dheads[i][1], dheads[i][2])] for i in range(2)], need_dx=False, need_dw=True)
  torch.cuda.synchronize()
  grads_two = {k: p.grad.clone() for k, p in netD.named_parameters()}
  for p in netD.parameters():
    p.grad.zero_()

  dx_one, later = netD.bwd_batched(ctx, dfeats, [_cat(*dheads[i]) for i in range(2)], B, chans)
  for call in later:
    call()
  _same(dx_one, dx_two, 'gradient to the fake image')
  for k, p in netD.named_parameters():
    assert torch.equal(p.grad.view(torch.int32), grads_two[k].view(torch.int32)), 'gradient of %s differs' % k
    assert not k.endswith('.weight') or float(grads_two[k].abs().max()) > 0.0, k
