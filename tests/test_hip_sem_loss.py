"""GPU checks of the semantics-weighted distortion (jpdse_sem_weighted_loss) against the float64 yardstick
tests/sem_loss_ref.py (pinned to hand-written examples in tests/test_sem_loss_host.py): value and gradient of the kernel in
both dtypes, its edge rule at the row wrap, the batch boundary and ids beyond float32, bit-equality with the plain l1 / mse
ops under all-ones weights, run-to-run bit-equality, and the train step with the two flags.

Bounds, those of the loss tests in tests/test_hip_ops.py: the value within 1e-5 * max(1, ref) of the fp64 reference on the same
(for bf16: the bf16-rounded) values; the gradient through assert_close with RTOL[dtype]."""
import functools

import pytest
import torch

import jpdse_hip
from jpdse_hip import ops, F32, BF16
from oracle.ctu_cpu import model as omodel
from ctu.utils import synthetic

import hip_util as hu
from hip_util import DEV, RTOL, to_act, to_nchw, assert_close, quantize_like
import sem_loss_ref as ref

pytestmark = pytest.mark.gpu

N_ONEHOT = 35
SHAPES = [(1, 1, 1), (1, 1, 70), (2, 9, 7), (2, 33, 130)]     # no neighbours; one row past a wave; ragged; several blocks
KINDS = ['l1', 'mse']
SCALE = 2.5


def _table():
  t = [1.0] * N_ONEHOT
  t[0], t[N_ONEHOT - 1], t[5], t[7] = 0.0, 0.5, 4.0, 0.25     # a zero weight, weights below 1, a weight above 1
  return t


TABLE = _table()


@functools.lru_cache(maxsize=None)
def _inputs(shape):
  """(fake, real) fp32 NCHW, label float [N,H,W], inst int64 [N,H,W], on the CPU."""
  n, h, w = shape
  g = torch.Generator().manual_seed(1000 + n * 7 + h * 3 + w)
  fake = torch.randn(n, 3, h, w, generator=g)
  real = torch.randn(n, 3, h, w, generator=g)
  label = torch.randint(0, N_ONEHOT, (n, h, w), generator=g).float()
  flat = label.view(-1)
  # labels at both ends of the table, outside it on both sides, fractional ones (truncated toward zero: 5.7 -> 5, -0.5 -> 0)
  for i, v in enumerate((0.0, float(N_ONEHOT - 1), 5.7, -0.5, 5.0, 7.0, -1.0, 300.0)):
    flat[(i * 3) % flat.numel()] = v
  # instance ids in blobs a few pixels wide, so that edge and interior pixels both occur
  inst = torch.randint(0, 5, (n, (h + 3) // 4, (w + 3) // 4), generator=g)
  inst = inst.repeat_interleave(4, dim=1).repeat_interleave(4, dim=2)[:, :h, :w].contiguous().long() * 1000 + 26
  return fake, real, label, inst


def _value_ok(what, got, want):
  bound = 1e-5 * max(1.0, abs(want))
  hu.record(what, abs(got - want), bound)
  assert abs(got - want) <= bound, '%s: %.9g vs %.9g, off by %.3e > %.1e' % (what, got, want, abs(got - want), bound)


def _call(fake, real, label, inst, table, ew, kind, dtype, scale=None):
  slot = torch.zeros(1, dtype=torch.float32, device=DEV)
  g = ops.sem_weighted_loss(to_act(fake, dtype), to_act(real, dtype), label.to(DEV).contiguous(),
                            inst.to(DEV).contiguous() if inst is not None else None, table, ew, kind, slot, scale)
  return slot.item(), g


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_value_and_gradient_against_the_fp64_yardstick(shape, kind, dtype):
  fake, real, label, inst = _inputs(shape)
  fq, rq = quantize_like(fake, dtype), quantize_like(real, dtype)
  for ew in (1.0, 3.0):
    for use_inst in ((True, False) if ew == 3.0 else (True,)):
      im = inst if use_inst else None
      want = ref.loss(fq, rq, label, im, TABLE, ew, kind)
      name = '%s ew %g%s' % (kind, ew, '' if use_inst else ' no ids')
      v0, g0 = _call(fq, rq, label, im, TABLE, ew, kind, dtype)
      assert g0 is None
      _value_ok(name + ' value (value-only call)', v0, want)
      v1, g1 = _call(fq, rq, label, im, TABLE, ew, kind, dtype, SCALE)
      assert v1 == v0, 'the value must not depend on whether the gradient is asked for'
      assert g1.t.dtype == (torch.bfloat16 if dtype == BF16 else torch.float32) and g1.t.shape == to_act(fq, dtype).t.shape
      assert (g1.t[..., 3:] == 0).all(), 'padding lanes of the gradient'
      assert_close(to_nchw(g1), ref.grad(fq, rq, label, im, TABLE, ew, kind, SCALE), RTOL[dtype], name + ' gradient')
  if shape[1] * shape[2] > 1:
    assert ref.loss(fq, rq, label, inst, TABLE, 3.0, kind) != ref.loss(fq, rq, label, None, TABLE, 3.0, kind)


def _device_weight_map(label, inst, table, ew):
  """w(p) as the kernel forms it, exactly: fp32 l1 with fake - real = 1 everywhere and scale = count gives dfake = w(p)."""
  n, h, w = label.shape
  ones, zeros = torch.ones(n, 3, h, w), torch.zeros(n, 3, h, w)
  _, g = _call(ones, zeros, label, inst, table, ew, 'l1', F32, scale=float(n * h * w * 3))
  m = to_nchw(g)
  assert torch.equal(m[:, 0], m[:, 1]) and torch.equal(m[:, 0], m[:, 2])
  return m[:, 0].double()


def test_ids_beyond_float32_are_told_apart():
  a, b = 2 ** 30 + 1, 2 ** 30 + 2
  assert torch.tensor(a).float() == torch.tensor(b).float()       # a float32 compare would see no edge
  inst = torch.tensor([[[a, a, a, b, b, b, b]]], dtype=torch.int64)
  label = torch.full((1, 1, 7), 3.0)
  w = _device_weight_map(label, inst, TABLE, 3.0)
  assert torch.equal(w, torch.tensor([[[1, 1, 3, 3, 1, 1, 1]]], dtype=torch.float64))
  assert torch.equal(w, ref.weight_map(label, inst, TABLE, 3.0))
  top = torch.tensor([[[2 ** 31 - 1, 2 ** 31 - 2], [2 ** 31 - 1, 2 ** 31 - 2]]], dtype=torch.int64)
  assert torch.equal(_device_weight_map(torch.full((1, 2, 2), 3.0), top, TABLE, 3.0), torch.full((1, 2, 2), 3.0, dtype=torch.float64))


def test_no_edge_across_the_row_wrap_or_the_batch_boundary():
  # every row of image 0 is 7 7 9 9, of image 1 is 11 11 13 13: a row's end and the next row's start differ (9 | 7), and so do
  # the last row of image 0 and the first of image 1, but only columns 1 and 2 hold a pixel whose neighbour differs
  rows = torch.tensor([[7, 7, 9, 9], [11, 11, 13, 13]], dtype=torch.int64)
  inst = rows[:, None, :].expand(2, 5, 4).contiguous()
  label = torch.full((2, 5, 4), 3.0)
  want = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=torch.float64).expand(2, 5, 4)
  w = _device_weight_map(label, inst, TABLE, 3.0)
  assert torch.equal(w, want) and torch.equal(ref.weight_map(label, inst, TABLE, 3.0), want)
  # images that are constant, each with its own id: no edge at all, also where image 0 ends and image 1 begins
  const = torch.stack([torch.full((5, 4), 1), torch.full((5, 4), 2)]).long()
  assert torch.equal(_device_weight_map(label, const, TABLE, 3.0), torch.ones(2, 5, 4, dtype=torch.float64))
  # labels outside the table and fractional ones, as the kernel reads them
  lab = torch.tensor([[[0.0, 34.0, -1.0, 300.0, 5.7, -0.5, 35.0, 256.0, 7.0, 1e10, -1e10, float('nan')]]])
  want = torch.tensor([[[0.0, 0.5, 1.0, 1.0, 4.0, 0.0, 1.0, 1.0, 0.25, 1.0, 1.0, 1.0]]], dtype=torch.float64)
  assert torch.equal(_device_weight_map(lab, None, TABLE, 1.0), want) and torch.equal(ref.weight_map(lab, None, TABLE, 1.0), want)


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
def test_all_ones_weights_are_the_plain_ops_bit_for_bit(dtype):
  fake, real, label, inst = _inputs((2, 33, 130))
  fq, rq = quantize_like(fake, dtype), quantize_like(real, dtype)
  A, B = to_act(fq, dtype), to_act(rq, dtype)
  ones = [1.0] * N_ONEHOT
  slot = torch.zeros(1, dtype=torch.float32, device=DEV)
  v, g = _call(fq, rq, label, inst, ones, 1.0, 'l1', dtype, SCALE)
  assert torch.equal(g.t, ops.l1_fwd_bwd(A, B, slot, SCALE).t)
  _value_ok('all-ones l1 value', v, (fq.double() - rq.double()).abs().mean().item())
  v, g = _call(fq, rq, label, inst, ones, 1.0, 'mse', dtype, SCALE)
  assert torch.equal(g.t, ops.mse_bwd(A, B, torch.ones(1, dtype=torch.float32, device=DEV), SCALE).t)
  _value_ok('all-ones mse value', v, ((fq.double() - rq.double()) ** 2).mean().item())


@pytest.mark.parametrize('kind', KINDS)
def test_two_calls_are_bit_identical(kind):
  fake, real, label, inst = _inputs((2, 33, 130))
  runs = [_call(fake, real, label, inst, TABLE, 3.0, kind, BF16, SCALE) for _ in range(2)]
  assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1].t, runs[1][1].t)


# ---- the train step -----------------------------------------------------------------------------------------------------------
FLAGS = dict(class_distortion_weights='24:4,26:2', edge_distortion_weight=3.0)
DT = {F32: 'fp32', BF16: 'bf16'}


def _batch():
  xd = synthetic.synthetic_batch(2, 64, 128, seed=9)
  xd['label'][:, :, :32, :40] = 24.0                # both weighted classes occur
  xd['label'][:, :, 40:, 90:] = 26.0
  return xd


def _trainer(dtype, **kw):
  from ctu.trainers import get_trainer
  opt = omodel.default_opt(gpu_ids=[0], print_losses=False, ngf=8, ndf=8, n_blocks_global=1, compute_dtype=DT[dtype], **kw)
  torch.manual_seed(4321)
  return get_trainer(opt)(opt, 'train'), opt


def _weights(tr):
  return {k: v.clone() for k, v in tr.model.netG.state_dict().items()}


@functools.lru_cache(maxsize=None)
def _default_step(dtype):
  """(losses, generator weights) after one default-flag step from the seeded initial state."""
  tr, _ = _trainer(dtype)
  assert tr.model.sem_weights is None
  tr.step(_batch())
  torch.cuda.synchronize()
  return dict(tr.last_losses), _weights(tr)


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
def test_step_reports_the_weighted_distortion_and_moves_the_generator_elsewhere(dtype):
  tr, opt = _trainer(dtype, **FLAGS)
  table, ew = tr.model.sem_weights
  assert len(table) == N_ONEHOT and table[24] == 4.0 and table[26] == 2.0 and ew == 3.0
  xd = _batch()
  start = _weights(tr)
  fake = tr.get_img(xd).cpu()                        # G is deterministic: the train-mode forward produces the same image
  real = quantize_like(xd['image'], dtype)
  label, inst = xd['label'][:, 0], xd['instance'][:, 0]
  want = ref.loss(fake, real, label, inst, table, ew, 'l1')
  assert want > 1.2 * ref.loss(fake, real, label, None, [1.0], 1.0, 'l1')       # the weights matter on this batch
  tr.train()
  losses = dict(zip(('G_GAN', 'G_GAN_Feat', 'G_VGG', 'G_Distortion', 'D_real', 'D_fake'), tr.model.get_train_loss(xd)))
  _value_ok('G_Distortion of get_train_loss', losses['G_Distortion'].item(), want)
  wd = tr.get_weighted_distortion(xd)
  assert isinstance(wd, float)
  _value_ok('get_weighted_distortion', wd, want)
  tr.step(xd)
  torch.cuda.synchronize()
  _value_ok('G_Distortion of the step', tr.last_losses['G_Distortion'], want)
  after = _weights(tr)
  _, plain_after = _default_step(dtype)
  assert any(not torch.equal(after[k], start[k]) for k in after if k.endswith('.weight')), 'the step must move the generator'
  assert any(not torch.equal(after[k], plain_after[k]) for k in after if k.endswith('.weight')), \
      'the weighted step must not end where the default-flag step ends'


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
def test_all_ones_flag_is_the_default_step_bit_for_bit(dtype):
  tr, _ = _trainer(dtype, class_distortion_weights='0:1', edge_distortion_weight=1.0)
  assert tr.model.sem_weights is None
  xd = _batch()
  tr.step(xd)
  torch.cuda.synchronize()
  losses, weights = _default_step(dtype)
  assert tr.last_losses == losses
  for k, v in tr.model.netG.state_dict().items():
    assert torch.equal(v, weights[k]), k
  # with trivial weights get_weighted_distortion is the plain mean
  fake = tr.get_img(xd).cpu()
  _value_ok('get_weighted_distortion, trivial weights', tr.get_weighted_distortion(xd),
            (fake.double() - quantize_like(xd['image'], dtype).double()).abs().mean().item())


def test_zero_ins_blanks_the_edge_lane_not_the_loss_weights():
  tr, _ = _trainer(BF16, zero_ins=True, **FLAGS)
  table, ew = tr.model.sem_weights
  xd = _batch()
  tr.train()
  state, slots, layout = tr.model._forward_losses(xd)
  raw = xd['instance'].to(DEV)[:, 0].contiguous()
  assert torch.equal(state['inst_raw'].view(raw.shape), raw)
  assert not tr.model.preprocess(xd, build_base=False)['inst'].any()       # the networks see a blank instance map
  got = slots[layout['dist']].item()
  fake, real, label = state['fake'], state['real'], state['label']         # the frozen fake of the --zero_ins forward
  slot = torch.zeros(2, dtype=torch.float32, device=DEV)
  ops.sem_weighted_loss(fake, real, label, raw, table, ew, 'l1', slot[0:1])
  ops.sem_weighted_loss(fake, real, label, torch.zeros_like(raw), table, ew, 'l1', slot[1:2])
  with_raw, with_zeroed = slot.tolist()
  assert got == with_raw, 'the model must weight with the dataset\'s own instance map under --zero_ins'
  assert with_zeroed < with_raw
  want = ref.loss(to_nchw(fake), to_nchw(real), xd['label'][:, 0], xd['instance'][:, 0], table, ew, 'l1')
  _value_ok('G_Distortion under --zero_ins', got, want)
