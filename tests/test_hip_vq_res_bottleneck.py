"""GPU tests of the residual quantizer as the encoder's bottleneck (layers.HipResidualVQBottleneck, Encoder(vq_stages > 1),
codec.VQStagesCodec, opt.vq_stages / opt.vq_train_stages on the model and the trainer).  One small configuration:
ngf 8, nef 8, two down-samplings, 64 x 128 images, batch 2, a bottleneck of 16 channels in vectors of 8, 16 centres, 3 stages,
fp32 and bf16."""
import pytest
import torch

from jpdse_hip import ops, F32, BF16
from jpdse_hip.ops import Act
from jpdse_hip.layers import HipResidualVQBottleneck, HipVQBottleneck, run_chain_fwd
from ctu.utils import vqstages
from oracle.ctu_cpu import model as omodel
import hip_util as hu
import vq_residual_ref as ref

pytestmark = pytest.mark.gpu
DEV = hu.DEV
N, H, W, C, D, L, S, DOWN = 2, 64, 128, 16, 8, 16, 3, 2
CODE_LEN = (H >> DOWN) * (W >> DOWN) * (C // D)
DTYPES = ['fp32', 'bf16']
CODE = {'fp32': F32, 'bf16': BF16}
BOOKS_KEY = 'model.%d.vq._code_books' % (4 + 3 * DOWN)


def _trainer(dtype, seed=1234, scale_books=True, **over):
  from ctu.trainers import get_trainer
  kw = dict(gpu_ids=[0], print_losses=False, compute_dtype=dtype, ngf=8, ndf=8, n_blocks_global=1, n_downsample_global=2,
            no_feat_encoding=False, no_encoder_binarization=False, feat_num=3, nef=8, n_downsample_E=DOWN,
            encoder_binarizer_out_channels=C, encoder_quantizer='s2hvq', vq_n_center=L, vq_center_size=D, vq_sigma=10.0,
            no_vgg_loss=True, no_gan_feat_loss=True, no_g_gan_loss=True, no_d_gan_loss=True, skip_unused_losses=True, vq_stages=S)
  kw.update(over)
  kw = {k: v for k, v in kw.items() if v is not _ABSENT}
  opt = omodel.default_opt(**kw)
  torch.manual_seed(seed)
  tr = get_trainer(opt)(opt, 'train')
  if scale_books:      # books at the scale of the bottleneck's features, so that more than one centre is in use
    with torch.no_grad():
      for p in tr.model.netE._vq.vq.parameters():
        p.mul_(0.05)
  return tr


_ABSENT = object()


def _batch(seed=3):
  return omodel.synthetic_batch(N, H, W, seed=seed)


_shared = {}


def _pair(dtype):
  """(trainer, batch, get_img of the batch), built once per dtype; tests that train or fit build their own."""
  if dtype not in _shared:
    tr = _trainer(dtype)
    xd = _batch()
    _shared[dtype] = (tr, xd, tr.get_img(xd).clone())
  return _shared[dtype]


# ---- the layer ------------------------------------------------------------------------------------------------------------------
def _layer(dtype, seed=5):
  torch.manual_seed(seed)
  layer = HipResidualVQBottleneck(32, C, L, D, S, sigma=1.0 / D, dtype=CODE[dtype], device=DEV)
  g = torch.Generator().manual_seed(seed)
  x = ops.nchw_to_nhwc((4.0 * torch.randn(N, 32, 16, 32, generator=g)).to(DEV), CODE[dtype])
  dy = ops.nchw_to_nhwc(torch.randn(N, C, 16, 32, generator=g).to(DEV), CODE[dtype])
  layer.train()
  layer.ensure_grads()
  return layer, x, dy


@pytest.mark.parametrize('dtype', DTYPES)
def test_layer_books_are_the_stated_draws(dtype):
  layer, _, _ = _layer(dtype)
  want = torch.stack([(2 * torch.rand(L, D, generator=torch.Generator().manual_seed(0 + s)) - 1) * 0.5 ** s for s in range(S)])
  assert torch.equal(layer.vq._code_books.detach().cpu(), want)
  assert [n for n, _ in layer.named_parameters()] == ['conv.weight', 'vq._code_books']
  assert (layer.groups, layer.cout, layer.center_size, layer.n_center, layer.n_stages) == (C // D, C, D, L, S)


@pytest.mark.parametrize('dtype', DTYPES)
def test_layer_forward_is_the_hand_composed_chain(dtype):
  layer, x, _ = _layer(dtype)
  books = layer.vq._code_books.detach()
  h, _ = layer.conv.fwd(x)
  for training in (True, False):
    layer.train(training)
    for stages in (None, 1, 2, 3):
      n = S if stages is None else stages
      y, ctx = layer.fwd(x, stages)
      want_y, want_index, _, _ = ops.vq_res_fwd(h.t.view(-1, D), books, n_stages=n)
      assert torch.equal(y.t, want_y.view(h.t.shape)) and y.C == C, (training, stages)
      assert torch.equal(ctx.items[2], want_index) and torch.equal(ctx.items[1].t, h.t)
      code = layer.code(x, stages)
      assert code.dtype == torch.int32 and tuple(code.shape) == (N, n, want_index.shape[1] // N)
      assert torch.equal(code, want_index.view(n, N, -1).transpose(0, 1))
      back, status = layer.decode(code, N, h.H, h.W, CODE[dtype])
      assert torch.equal(back.t, y.t) and int(status.item()) == 0
  assert len(torch.unique(want_index)) > 1, 'the fixture uses a single centre'
  layer.train()
  layer.train_stages = 2                                         # the owner's count holds in training, never in eval
  assert layer.fwd(x)[1].items[2].shape[0] == 2
  layer.eval()
  assert layer.fwd(x)[1].items[2].shape[0] == S
  for bad in (0, S + 1, True, 1.0):
    with pytest.raises(ValueError, match='stages must be an int in 1 .. 3'):
      layer.fwd(x, bad)


@pytest.mark.parametrize('stages', [None, 2])
@pytest.mark.parametrize('dtype', DTYPES)
def test_layer_backward_is_the_composed_chain_and_matches_fp64(dtype, stages):
  layer, x, dy = _layer(dtype)
  n = S if stages is None else stages
  sigma = layer.vq.sigma
  books = layer.vq._code_books.detach().clone()
  fired = []
  layer.grad_ready_hook = lambda mod: fired.append(mod.vq._code_books.grad.clone())
  layer.vq._code_books.grad.fill_(7.0)                           # stale values beyond `stages` must be overwritten with zeros
  y, ctx = layer.fwd(x, stages)
  dx = layer.bwd(ctx, dy)
  got = dict(dx=dx.t.clone(), dw=layer.conv.weight.grad.clone(), dc=layer.vq._code_books.grad.clone())
  assert len(fired) == 1 and torch.equal(fired[0], got['dc'])
  # the composed chain, call for call
  h, c_conv = layer.conv.fwd(x)
  index = ctx.items[2]
  dh, dc = ops.vq_res_bwd(dy.t.view(-1, D), h.t.view(-1, D), books, index, sigma)
  want_dx = layer.conv.bwd(c_conv, Act(dh.view(h.t.shape), h.C), True, True)
  assert torch.equal(got['dx'], want_dx.t) and torch.equal(got['dw'], layer.conv.weight.grad) and torch.equal(got['dc'], dc)
  assert tuple(dc.shape) == (S, L, D) and not bool(dc[n:].any()) and bool(dc[:n].any(dim=2).any(dim=1).all())
  # the quantizer's gradients against the fp64 autograd oracle, on the rows fp64 decides as the device did
  h64 = h.t.view(-1, D).double().cpu()
  _, index64, _, _, decided = ref.forward(h64, books.double().cpu(), n)
  keep = decided & (index64 == index.cpu().long()).all(dim=0)
  assert int((~keep).sum()) <= 0.01 * h64.shape[0]
  dyk = dy.t.view(-1, D) * keep.to(DEV).unsqueeze(1).to(dy.t.dtype)
  dhk, dck = ops.vq_res_bwd(dyk.contiguous(), h.t.view(-1, D), books, index, sigma)
  dx64, dc64 = ref.grads(dyk.double().cpu()[keep], h64[keep], books.double().cpu(), sigma, n)
  hu.assert_close(dhk[keep.to(DEV)].double().cpu(), dx64, hu.RTOL[CODE[dtype]], 'HipResidualVQBottleneck dh')
  hu.assert_close(dck.double().cpu(), dc64, hu.RTOL[F32], 'HipResidualVQBottleneck dbooks')


# ---- model and trainer ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_one_stage_is_todays_bottleneck(dtype):
  xd = _batch()
  plain = _trainer(dtype, vq_stages=_ABSENT)
  want = plain.get_img(xd)
  for over in (dict(vq_stages=1), dict(vq_stages=1, vq_train_stages='all')):
    tr = _trainer(dtype, **over)
    assert type(tr.model.netE._vq) is HipVQBottleneck and type(tr.model.codec).__name__ == 'VQIndexCodec'
    assert list(tr.model.netE.state_dict().keys()) == list(plain.model.netE.state_dict().keys())
    assert all(torch.equal(a, b) for a, b in zip(tr.model.netE.state_dict().values(), plain.model.netE.state_dict().values()))
    assert torch.equal(tr.get_img(xd), want)
    assert tuple(tr.get_vq_code(xd, stages=1).shape) == (N, CODE_LEN)
    with pytest.raises(ValueError, match='vq_stages = 1'):
      tr.get_vq_code(xd, stages=2)


@pytest.mark.parametrize('dtype', DTYPES)
def test_a_trainer_step_trains_every_book_and_repeats(dtype):
  xd = _batch()
  runs = []
  for _ in range(2):
    tr = _trainer(dtype)
    vq = tr.model.netE._vq
    assert type(vq) is HipResidualVQBottleneck and type(tr.model.codec).__name__ == 'VQStagesCodec'
    books0, w0 = vq.vq._code_books.detach().clone(), vq.conv.weight.detach().clone()
    tr.step(xd)
    torch.cuda.synchronize()
    for k, v in tr.last_losses.items():
      assert v == v and abs(v) != float('inf'), (k, v)
    assert 'G_Rate' not in tr.last_losses
    moved = (vq.vq._code_books.detach() != books0).any(dim=2).any(dim=1)
    assert moved.cpu().tolist() == [True] * S, 'a code book did not move'
    assert not torch.equal(vq.conv.weight.detach(), w0), 'the 1x1 conv did not move'
    tr.step(_batch(seed=4))
    torch.cuda.synchronize()
    runs.append({k: v.detach().clone() for net in (tr.model.netE, tr.model.netG) for k, v in net.state_dict().items()})
    assert all(bool(torch.isfinite(v).all()) for v in runs[-1].values())
  assert runs[0].keys() == runs[1].keys() and all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])


@pytest.mark.parametrize('dtype', DTYPES)
def test_uniform_schedule_zeroes_the_books_beyond_the_draw(dtype):
  tr = _trainer(dtype, vq_train_stages='uniform')
  xd = _batch()
  vq = tr.model.netE._vq
  draw = lambda t: 1 + int(torch.randint(S, (1,), generator=torch.Generator().manual_seed(tr.model.codec_seed * 1000003 + t)))
  steps = [next(t for t in range(100) if draw(t) == n) for n in (1, 2)]
  for t, n in zip(steps, (1, 2)):
    tr.model.codec_draw = t
    vq.ensure_grads()
    vq.vq._code_books.grad.fill_(7.0)                            # stale values must not survive in the unused books
    tr.step(xd)
    torch.cuda.synchronize()
    assert tr.model.codec_draw == t + 1 and vq.train_stages == n == tr.model.train_stage_count(t)
    grad = vq.vq._code_books.grad
    used = grad.ne(0).any(dim=2).any(dim=1).cpu().tolist()
    assert used == [s < n for s in range(S)], (t, n, used)
  tr.eval()
  assert tuple(tr.get_vq_code(xd).shape) == (N, S, CODE_LEN)     # eval mode takes all stages


@pytest.mark.parametrize('dtype', DTYPES)
def test_state_dict_round_trips(dtype):
  tr, xd, img = _pair(dtype)
  sd = {k: v.detach().clone() for k, v in tr.model.netE.state_dict().items()}
  assert BOOKS_KEY in sd and tuple(sd[BOOKS_KEY].shape) == (S, L, D) and BOOKS_KEY.replace('vq._code_books', 'conv.weight') in sd
  other = _trainer(dtype, seed=99)
  other.model.netG.load_state_dict(tr.model.netG.state_dict())
  assert not torch.equal(other.get_img(xd), img)
  other.model.netE.load_state_dict(sd)
  got = other.model.netE.state_dict()
  assert list(got.keys()) == list(sd.keys()) and all(torch.equal(got[k], sd[k]) for k in sd)
  assert torch.equal(other.get_img(xd), img)
  one = _trainer(dtype, vq_stages=1)
  with pytest.raises(RuntimeError):                              # a one-stage checkpoint into three stages, and back
    other.model.netE.load_state_dict(one.model.netE.state_dict())
  with pytest.raises(RuntimeError):
    one.model.netE.load_state_dict(sd)


@pytest.mark.parametrize('dtype', DTYPES)
def test_code_files_and_every_prefix_decode(dtype):
  tr, xd, img = _pair(dtype)
  code = tr.get_vq_code(xd)
  assert code.dtype == torch.int64 and code.is_cuda and tuple(code.shape) == (N, S, CODE_LEN)
  assert int(code.min()) >= 0 and int(code.max()) < L and len(torch.unique(code[:, 0])) > 1
  receiver = {'label': xd['label'], 'instance': xd['instance']}
  assert torch.equal(tr.decode(code, receiver), img)
  assert torch.equal(tr.decode(code.cpu(), receiver), img)
  blobs = tr.get_coded(xd)
  assert isinstance(blobs, list) and len(blobs) == N and all(isinstance(b, bytes) and b[:4] == vqstages.MAGIC for b in blobs)
  assert all(vqstages.parse_stages(b)[:4] == (S, 1, CODE_LEN, L) for b in blobs)
  assert torch.equal(tr.decode_coded(blobs, receiver), img)
  coded, packed = tr.get_coded_rate(xd)
  assert coded == sum(8.0 * len(b) / (H * W) for b in blobs) / N and packed > 0
  for n in (1, 2):
    assert torch.equal(tr.get_vq_code(xd, stages=n), code[:, :n])
    cut = [vqstages.truncate_stages(b, n) for b in blobs]
    assert tr.get_coded_stages(xd, stages=n) == cut
    a = tr.decode(code[:, :n], receiver)
    assert torch.equal(tr.decode_coded(cut, receiver), a)
    assert torch.equal(tr.decode_coded(tr.get_coded_stages(xd, stages=n), receiver), a)
    assert not torch.equal(a, img)
  assert tr.get_coded_stages(xd) == blobs == tr.get_coded_stages(xd, stages=S)
  with pytest.raises(ValueError, match='same stage count'):
    tr.decode_coded([blobs[0], vqstages.truncate_stages(blobs[1], 1)], receiver)
  bad = code.clone()
  bad[0, 1, 0] = L
  with pytest.raises(ValueError, match='an index outside'):
    tr.decode(bad, receiver)


@pytest.mark.parametrize('dtype', DTYPES)
def test_stage_curve(dtype):
  """On 192 x 256 images: MS-SSIM's five scales need a shorter side of 176, which the 64 x 128 batch of the other tests lacks."""
  tr, _, _ = _pair(dtype)
  H, W = 192, 256
  xd = omodel.synthetic_batch(N, H, W, seed=5)
  rows = tr.get_stage_curve(xd)
  blobs = tr.get_coded(xd)
  assert [r['stages'] for r in rows] == [1, 2, 3] and all(sorted(r) == ['bpp', 'l1', 'ms_ssim', 'mse', 'psnr', 'stages'] for r in rows)
  assert rows[0]['bpp'] < rows[1]['bpp'] < rows[2]['bpp']
  for r in rows:
    assert r['bpp'] == sum(8.0 * len(vqstages.truncate_stages(b, r['stages'])) / (H * W) for b in blobs) / N
  full = tr.get_eval_metrics(xd)
  assert all(rows[2][k] == full[k] for k in ('l1', 'mse', 'psnr', 'ms_ssim'))
  assert any(rows[0][k] != full[k] for k in ('l1', 'mse'))


@pytest.mark.parametrize('dtype', DTYPES)
def test_code_book_fit_reports_every_stage(dtype):
  tr = _trainer(dtype)
  xd = _batch()
  books = tr.model.netE._vq.vq._code_books
  ptr, before = books.data_ptr(), books.detach().clone()
  reports = tr.fit_vq_code_book([xd], n_iter=2)
  assert isinstance(reports, list) and len(reports) == S and books.data_ptr() == ptr and not torch.equal(books.detach(), before)
  finals = [r['final'] for r in reports]
  assert all(f == f and f >= 0 for f in finals) and finals[1] <= finals[0] and finals[2] <= finals[1], finals
  assert all(len(r['distortion']) == 3 for r in reports)
  assert torch.equal(tr.decode(tr.get_vq_code(xd), xd), tr.get_img(xd))
