"""GPU tests of --lambda_vq_rate on the trainer at the tiny s2hvq configuration of
tests/test_hip_vq_encoder.py: one step with the rate term (G_Rate, the code book's gradient through the grouped backward), the
flag at 0 against a trainer built without the option (bit-identical), and get_vq_rate against the entropy of get_vq_code."""
import math

import pytest
import torch

from jpdse_hip import ops, F32
from jpdse_hip.ops import Act
import hip_util as hu
from test_hip_vq_encoder import _trainer, _batch, N, H, W, C, D, L, DTYPES

pytestmark = pytest.mark.gpu
TOL = hu.RTOL[F32]
GROUPS = C // D
_stepped = {}


def _step(dtype, mode):
  """One step of a fresh trainer, once per (dtype, mode): mode 'rate' = --lambda_vq_rate 0.5, 'zero' = the flag at 0, 'plain' =
  built without the option.  Returns the losses, the code book's gradient and what the bottleneck's backward saw."""
  key = (dtype, mode)
  if key not in _stepped:
    over = {'rate': dict(lambda_vq_rate=0.5), 'zero': dict(lambda_vq_rate=0.0), 'plain': {}}[mode]
    tr = _trainer(dtype, **over)
    vq = tr.model.netE._vq
    seen = []
    inner = vq.bwd

    def spy(ctx, dy, need_dx=True, need_dw=True):
      seen.append((tuple(it.t.clone() if isinstance(it, Act) else it.clone() for it in ctx.items[1:]), dy.t.clone(),
                   vq.vq._code_book.detach().clone()))
      return inner(ctx, dy, need_dx, need_dw)

    vq.bwd = spy
    try:
      tr.step(_batch())
    finally:
      del vq.bwd
    torch.cuda.synchronize()
    assert len(seen) == 1
    _stepped[key] = (dict(tr.last_losses), vq.vq._code_book.grad.clone(), seen[0], vq.conv.weight.grad.clone())
  return _stepped[key]


@pytest.mark.parametrize('dtype', DTYPES)
def test_one_step_with_the_rate_term(dtype):
  losses, grad, (items, dy, book), _ = _step(dtype, 'rate')
  assert len(items) == 2, 'the context of a forward with a rate scale carries dhist'
  h, dhist = items
  assert tuple(dhist.shape) == (GROUPS, L) and dhist.dtype == torch.float32
  rate = losses['G_Rate']
  assert rate == rate and 0.0 < rate < float('inf')
  for k, v in losses.items():
    assert v == v and abs(v) != float('inf'), (k, v)
  # the reported value is the unscaled soft rate of the captured conv output, in bits per pixel of the batch
  want, _, want_dhist = ops.vq_rate_fwd(h.view(-1, D), book, 10.0, GROUPS, N * H * W, 0.5)
  hu.assert_close(torch.tensor([rate]), want.cpu().double(), TOL, 'G_Rate vs ops.vq_rate_fwd')
  assert torch.equal(dhist, want_dhist)
  assert rate <= math.log2(L) * GROUPS * (H >> 2) * (W >> 2) / (H * W) * (1 + 1e-5)        # at most log2 L bits per index
  # the code book's gradient is the module-level grouped backward on the captured dy and dhist
  _, dc = ops.vq_quantize_bwd(dy.view(-1, D), h.view(-1, D), book, 10.0, want_dx=False, groups=GROUPS, dhist=dhist)
  assert torch.equal(grad, dc) and float(grad.abs().max()) > 0
  # and differs from the same step without the term
  _, grad0, (items0, dy0, book0), _ = _step(dtype, 'zero')
  assert torch.equal(book0, book) and torch.equal(items0[0], h) and torch.equal(dy0, dy)
  assert not torch.equal(grad, grad0)


@pytest.mark.parametrize('dtype', DTYPES)
def test_the_flag_at_zero_is_the_step_without_the_option(dtype):
  losses0, grad0, (items0, dy0, _), wgrad0 = _step(dtype, 'zero')
  losses1, grad1, (items1, dy1, _), wgrad1 = _step(dtype, 'plain')
  assert len(items0) == 1 and len(items1) == 1, 'no dhist travels without a rate scale'
  assert 'G_Rate' not in losses0 and losses0 == losses1
  assert torch.equal(grad0, grad1) and torch.equal(wgrad0, wgrad1) and torch.equal(dy0, dy1)


@pytest.mark.parametrize('dtype', DTYPES)
def test_get_vq_rate_is_the_entropy_of_the_code(dtype):
  tr = _trainer(dtype)
  xd = _batch()
  value = tr.get_vq_rate(xd)
  code = tr.get_vq_code(xd).cpu()
  per_group = code.view(N, -1, GROUPS)
  n = N * per_group.shape[1]
  bits = 0.0
  for g in range(GROUPS):
    counts = torch.bincount(per_group[:, :, g].reshape(-1), minlength=L).double()
    keep = counts > 0
    bits -= float((counts[keep] * torch.log2(counts[keep] / n)).sum())
  want = bits / (N * H * W)
  assert isinstance(value, float) and want > 0
  assert abs(value - want) <= 1e-5 * want, (value, want)
  # an estimate, not a size: it is reported next to the coded figure without an order between them
  coded, packed = tr.get_coded_rate(xd)
  assert coded > 0 and packed > 0
