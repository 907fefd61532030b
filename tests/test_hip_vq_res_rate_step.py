"""GPU tests of opt.lambda_vq_stage_rate on the trainer at the tiny s2hvq configuration of
tests/test_hip_vq_rate_step.py with vq_stages = 3: one step with the rate term (G_Rate, the books' gradient through the grouped
backward), the field at 0 against a trainer built without it (bit-identical), and the 'uniform' schedule, under which the term
covers the drawn stage prefix only."""
import pytest
import torch

from jpdse_hip import ops, F32
from jpdse_hip.ops import Act
from oracle.ctu_cpu import model as omodel
import hip_util as hu
from test_hip_vq_encoder import _batch, N, H, W, C, D, L, DOWN, DTYPES

pytestmark = pytest.mark.gpu
TOL = hu.RTOL[F32]
GROUPS = C // D
S = 3
SIGMA = 10.0
_stepped = {}


def _trainer(dtype, seed=1234, **over):
  from ctu.trainers import get_trainer
  kw = dict(gpu_ids=[0], print_losses=False, compute_dtype=dtype, ngf=8, ndf=8, n_blocks_global=1, n_downsample_global=2,
            no_feat_encoding=False, no_encoder_binarization=False, feat_num=3, nef=8, n_downsample_E=DOWN,
            encoder_binarizer_out_channels=C, encoder_quantizer='s2hvq', vq_n_center=L, vq_center_size=D, vq_sigma=SIGMA,
            no_vgg_loss=True, no_gan_feat_loss=True, no_g_gan_loss=True, no_d_gan_loss=True, skip_unused_losses=True, vq_stages=S)
  kw.update(over)
  opt = omodel.default_opt(**kw)
  torch.manual_seed(seed)
  tr = get_trainer(opt)(opt, 'train')
  with torch.no_grad():      # books at the scale of the bottleneck's features, so that more than one centre is in use
    tr.model.netE._vq.vq._code_books.mul_(0.05)
  return tr


def _spied_step(tr, xd):
  """One step; what the bottleneck's backward saw: (the context's tensors after the conv's, dy, the books before the update)."""
  vq = tr.model.netE._vq
  seen = []
  inner = vq.bwd

  def spy(ctx, dy, need_dx=True, need_dw=True):
    seen.append((tuple(it.t.clone() if isinstance(it, Act) else it.clone() for it in ctx.items[1:]), dy.t.clone(),
                 vq.vq._code_books.detach().clone()))
    return inner(ctx, dy, need_dx, need_dw)

  vq.bwd = spy
  try:
    tr.step(xd)
  finally:
    del vq.bwd
  torch.cuda.synchronize()
  assert len(seen) == 1
  return seen[0]


def _step(dtype, mode):
  """One step of a fresh trainer, once per (dtype, mode): 'rate' = lambda_vq_stage_rate 0.5, 'zero' = the field at 0, 'plain' =
  built without the field."""
  key = (dtype, mode)
  if key not in _stepped:
    over = {'rate': dict(lambda_vq_stage_rate=0.5), 'zero': dict(lambda_vq_stage_rate=0.0), 'plain': {}}[mode]
    tr = _trainer(dtype, **over)
    vq = tr.model.netE._vq
    seen = _spied_step(tr, _batch())
    stage_values = vq.rate_stage_values.clone() if vq.rate_stage_values is not None else None
    _stepped[key] = (dict(tr.last_losses), vq.vq._code_books.grad.clone(), seen, vq.conv.weight.grad.clone(), stage_values)
  return _stepped[key]


@pytest.mark.parametrize('dtype', DTYPES)
def test_one_step_with_the_rate_term(dtype):
  losses, grad, (items, dy, books), _, stage_values = _step(dtype, 'rate')
  assert len(items) == 3, 'the context of a forward with a rate scale carries dhist'
  h, index, dhist = items
  assert tuple(dhist.shape) == (S, GROUPS, L) and dhist.dtype == torch.float32 and tuple(index.shape) == (S, h.numel() // D)
  rate = losses['G_Rate']
  assert rate == rate and 0.0 < rate < float('inf')
  for k, v in losses.items():
    assert v == v and abs(v) != float('inf'), (k, v)
  # the reported value is the unscaled total of the captured conv output, in bits per pixel of the batch; the code is the rows kernel's
  want, want_rates, _, want_dhist, _, want_index = ops.vq_res_rate_fwd(h.view(-1, D), books, SIGMA, GROUPS, N * H * W, 0.5, want_code=True)
  hu.assert_close(torch.tensor([rate]), want.cpu().double(), TOL, 'G_Rate vs ops.vq_res_rate_fwd')
  assert torch.equal(dhist, want_dhist) and torch.equal(index, want_index) and torch.equal(stage_values, want_rates)
  assert torch.equal(index, ops.vq_res_rows_fwd(h.view(-1, D), books)[1])
  # the books' gradient is the module-level grouped backward on the captured dy and dhist
  _, dc = ops.vq_res_bwd(dy.view(-1, D), h.view(-1, D), books, index, SIGMA, want_dx=False, groups=GROUPS, dhist=dhist)
  assert torch.equal(grad, dc) and float(grad.abs().max()) > 0
  # and differs from the same step without the term
  _, grad0, (items0, dy0, books0), _, _ = _step(dtype, 'zero')
  assert torch.equal(books0, books) and torch.equal(items0[0], h) and torch.equal(items0[1], index) and torch.equal(dy0, dy)
  assert not torch.equal(grad, grad0)


@pytest.mark.parametrize('dtype', DTYPES)
def test_the_field_at_zero_is_the_step_without_it(dtype):
  losses0, grad0, (items0, dy0, _), wgrad0, sv0 = _step(dtype, 'zero')
  losses1, grad1, (items1, dy1, _), wgrad1, sv1 = _step(dtype, 'plain')
  assert len(items0) == 2 and len(items1) == 2 and sv0 is None and sv1 is None, 'no dhist travels without a rate scale'
  assert 'G_Rate' not in losses0 and losses0 == losses1
  assert torch.equal(grad0, grad1) and torch.equal(wgrad0, wgrad1) and torch.equal(dy0, dy1)


@pytest.mark.parametrize('dtype', DTYPES)
def test_uniform_schedule_keeps_the_rate_term_to_the_drawn_prefix(dtype):
  tr = _trainer(dtype, vq_train_stages='uniform', lambda_vq_stage_rate=0.5)
  xd = _batch()
  vq = tr.model.netE._vq
  draw = lambda t: 1 + int(torch.randint(S, (1,), generator=torch.Generator().manual_seed(tr.model.codec_seed * 1000003 + t)))
  for n in (1, 2):
    t = next(t for t in range(100) if draw(t) == n)
    tr.model.codec_draw = t
    vq.ensure_grads()
    vq.vq._code_books.grad.fill_(7.0)                            # stale values must not survive in the unused books
    (h, index, dhist), dy, books = _spied_step(tr, xd)
    assert vq.train_stages == n and tuple(index.shape)[0] == n and tuple(dhist.shape) == (n, GROUPS, L)
    assert tuple(vq.rate_stage_values.shape) == (n,)
    grad = vq.vq._code_books.grad
    assert grad.ne(0).any(dim=2).any(dim=1).cpu().tolist() == [s < n for s in range(S)], (t, n)
    # the rate's share alone: the grouped backward with dy = 0 leaves nothing in the books beyond the draw either
    _, dc = ops.vq_res_bwd(torch.zeros_like(dy).view(-1, D), h.view(-1, D), books, index, SIGMA, want_dx=False, groups=GROUPS, dhist=dhist)
    assert bool(dc[:n].ne(0).any()) and not bool(dc[n:].any())
    want = ops.vq_res_rate_fwd(h.view(-1, D), books, SIGMA, GROUPS, N * H * W, 0.5, n_stages=n)[0]
    hu.assert_close(torch.tensor([tr.last_losses['G_Rate']]), want.cpu().double(), TOL, 'G_Rate of the drawn prefix')
