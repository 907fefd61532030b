"""GPU tests of the vector-quantizer bottleneck inside the learned codec (layers.HipVQBottleneck, Encoder(quantizer='s2hvq'),
--encoder_quantizer s2hvq on the model and the trainer).  One small configuration: nef 8, two down-samplings,
64 x 32 images, a bottleneck of 16 channels in vectors of 4, 8 centres, batch 2, fp32 and bf16."""
import pytest
import torch

from jpdse_hip import ops, F32, BF16
from jpdse_hip.ops import Act
from jpdse_hip.layers import run_chain_fwd
from oracle.ctu_cpu import model as omodel
import hip_util as hu

pytestmark = pytest.mark.gpu
DEV = hu.DEV
N, H, W, C, D, L, DOWN = 2, 64, 32, 16, 4, 8, 2
CODE_LEN = (H >> DOWN) * (W >> DOWN) * (C // D)
DTYPES = ['fp32', 'bf16']


def _trainer(dtype, seed=1234, **over):
  from ctu.trainers import get_trainer
  kw = dict(gpu_ids=[0], print_losses=False, compute_dtype=dtype, ngf=8, ndf=8, n_blocks_global=1, n_downsample_global=2,
            no_feat_encoding=False, no_encoder_binarization=False, feat_num=3, nef=8, n_downsample_E=DOWN,
            encoder_binarizer_out_channels=C, encoder_quantizer='s2hvq', vq_n_center=L, vq_center_size=D, vq_sigma=10.0,
            no_vgg_loss=True, no_gan_feat_loss=True, no_g_gan_loss=True, no_d_gan_loss=True, skip_unused_losses=True)
  kw.update(over)
  opt = omodel.default_opt(**kw)
  torch.manual_seed(seed)
  tr = get_trainer(opt)(opt, 'train')
  # a code book at the scale of the bottleneck's features, so that more than one centre is in use
  with torch.no_grad():
    tr.model.netE._vq.vq._code_book.mul_(0.05)
  return tr


def _batch(seed=3):
  return omodel.synthetic_batch(N, H, W, seed=seed)


_shared = {}


def _pair(dtype):
  """(trainer, batch, get_img of the batch), built once per dtype; tests that train build their own."""
  if dtype not in _shared:
    tr = _trainer(dtype)
    xd = _batch()
    _shared[dtype] = (tr, xd, tr.get_img(xd).clone())
  return _shared[dtype]


@pytest.mark.parametrize('dtype', DTYPES)
def test_encoder_forward_is_the_hand_composed_chain(dtype):
  tr, xd, _ = _pair(dtype)
  enc = tr.model.netE
  x = ops.nchw_to_nhwc(xd['image'].to(DEV).float().contiguous(), tr.model.cdtype)
  for training, hard in ((False, True), (True, True), (True, False)):
    enc.train(training)
    enc._vq.hard_forward = hard
    try:
      y, _ = enc.fwd(x)
      h, _ = run_chain_fwd(enc._pre, x)
      hc, _ = enc._vq.conv.fwd(h)
      with torch.no_grad():
        yq, code, _ = enc._vq.vq.quantize(hc.t.view(N, -1), CODE_LEN, hard_forward=hard)
      want, _ = run_chain_fwd(enc._post, Act(yq.view(hc.t.shape), C))
      assert torch.equal(y.t, want.t), (training, hard)
      assert code.shape == (N, CODE_LEN)
      if hard:
        assert torch.equal(enc.vq_code(x).long(), code)
    finally:
      enc._vq.hard_forward = True
      enc.train(False)
  assert len(torch.unique(code)) > 1, 'the fixture uses a single centre'


@pytest.mark.parametrize('dtype', DTYPES)
def test_state_dict_round_trips(dtype):
  tr, xd, img = _pair(dtype)
  sd = {k: v.detach().clone() for k, v in tr.model.netE.state_dict().items()}
  assert 'model.10.conv.weight' in sd and 'model.10.vq._code_book' in sd
  assert tuple(sd['model.10.conv.weight'].shape) == (C, 8 * 2 ** DOWN, 1, 1) and tuple(sd['model.10.vq._code_book'].shape) == (L, D)
  other = _trainer(dtype, seed=99)
  other.model.netG.load_state_dict(tr.model.netG.state_dict())
  assert not torch.equal(other.get_img(xd), img)
  other.model.netE.load_state_dict(sd)
  got = other.model.netE.state_dict()
  assert list(got.keys()) == list(sd.keys()) and all(torch.equal(got[k], sd[k]) for k in sd)
  assert torch.equal(other.get_img(xd), img)


@pytest.mark.parametrize('dtype', DTYPES)
def test_one_trainer_step_trains_the_code_book(dtype):
  tr = _trainer(dtype)
  xd = _batch()
  vq = tr.model.netE._vq
  book0 = vq.vq._code_book.detach().clone()
  w0 = vq.conv.weight.detach().clone()
  seen = []
  inner = vq.bwd

  def spy(ctx, dy, need_dx=True, need_dw=True):
    seen.append((ctx.items[1].t.clone(), dy.t.clone(), vq.vq._code_book.detach().clone()))
    return inner(ctx, dy, need_dx, need_dw)

  vq.bwd = spy
  try:
    tr.step(xd)
  finally:
    del vq.bwd
  torch.cuda.synchronize()
  for k, v in tr.last_losses.items():
    assert v == v and abs(v) != float('inf'), (k, v)
  assert len(seen) == 1
  h, dy, book = seen[0]
  assert torch.equal(book, book0)
  _, dc = ops.vq_quantize_bwd(dy.view(-1, D), h.view(-1, D), book, 10.0, want_dx=False)
  grad = vq.vq._code_book.grad
  assert grad is not None and torch.equal(grad, dc) and float(grad.abs().max()) > 0
  assert not torch.equal(vq.vq._code_book.detach(), book0), 'the code book did not move'
  assert not torch.equal(vq.conv.weight.detach(), w0), 'the 1x1 conv did not move'
  assert bool(torch.isfinite(vq.vq._code_book.detach()).all()) and bool(torch.isfinite(vq.conv.weight.detach()).all())


@pytest.mark.parametrize('dtype', DTYPES)
def test_code_files_and_decoders_reproduce_get_img(dtype):
  from ctu.utils import vqstream
  tr, xd, img = _pair(dtype)
  code = tr.get_vq_code(xd)
  assert code.dtype == torch.int64 and code.is_cuda and tuple(code.shape) == (N, CODE_LEN)
  assert int(code.min()) >= 0 and int(code.max()) < L
  receiver = {'label': xd['label'], 'instance': xd['instance']}
  assert torch.equal(tr.decode(code, receiver), img)
  assert torch.equal(tr.decode(code.cpu(), receiver), img)
  blobs = tr.get_coded(xd)
  assert isinstance(blobs, list) and len(blobs) == N and all(isinstance(b, bytes) for b in blobs)
  assert torch.equal(tr.decode_coded(blobs, receiver), img)
  pixels = H * W
  coded, packed = tr.get_coded_rate(xd)
  assert coded == sum(8.0 * len(b) / pixels for b in blobs) / N
  assert packed == 8.0 * (vqstream.HEADER_BYTES + vqstream.packed_bytes(CODE_LEN, L)) / pixels
  for i, b in enumerate(blobs):
    n, code_len, Lb, S, mode, _ = vqstream.parse_blob(b)
    assert (n, code_len, Lb) == (1, CODE_LEN, L) and (mode == vqstream.MODE_PACKED or S == (C // D) * 8)
    assert len(b) <= vqstream.HEADER_BYTES + vqstream.packed_bytes(CODE_LEN, L)
    assert torch.equal(vqstream.read_indices(b, DEV), code[i:i + 1])
  # files alone, and the total rate, pick the blob kind from the encoder
  sem = tr.get_coded_semantics(xd)
  assert torch.equal(tr.decode_from_files(blobs, sem), img)
  code_bpp, sem_bpp, total = tr.get_total_rate(xd)
  assert code_bpp == coded and total == code_bpp + sem_bpp
  # a code that does not fit is refused
  with pytest.raises(ValueError, match='shape'):
    tr.decode(code[:, :-1], receiver)
  bad = code.clone()
  bad[0, 0] = L
  with pytest.raises(ValueError, match='outside'):
    tr.decode(bad, receiver)
  with pytest.raises(ValueError, match='int64'):
    tr.decode(code.float(), receiver)
  for call in (tr.get_code, tr.get_eval_rate, tr.get_context_rate, tr.get_rate_map, tr.get_class_rates):
    with pytest.raises(ValueError, match='encoder_quantizer'):
      call(xd)
  # the eval loss runs with the VQ encoder
  assert float(tr.get_eval_loss(xd)) >= 0


@pytest.mark.parametrize('dtype', DTYPES)
def test_soft_forward_changes_the_training_features_only(dtype):
  tr, xd, img = _pair(dtype)
  soft = _trainer(dtype, vq_soft_forward=True)
  soft.model.netG.load_state_dict(tr.model.netG.state_dict())
  soft.model.netE.load_state_dict(tr.model.netE.state_dict())
  assert soft.model.netE._vq.hard_forward is False and tr.model.netE._vq.hard_forward is True
  assert torch.equal(soft.get_img(xd), img)
  assert torch.equal(soft.get_vq_code(xd), tr.get_vq_code(xd))
  x = ops.nchw_to_nhwc(xd['image'].to(DEV).float().contiguous(), tr.model.cdtype)
  feats = []
  for t in (tr, soft):
    t.model.netE.train(True)
    try:
      feats.append(t.model.netE.fwd(x)[0].t.clone())
    finally:
      t.model.netE.train(False)
  assert not torch.equal(feats[0], feats[1])
  tr.model.netE.train(False)
  assert torch.equal(tr.model.netE.fwd(x)[0].t, soft.model.netE.fwd(x)[0].t)
