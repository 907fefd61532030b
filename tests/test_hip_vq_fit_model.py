"""GPU tests of the code-book fit on the model and the trainer (fit_vq_code_book, get_vq_usage), in the tiny
configuration of tests/test_hip_vq_encoder.py (nef 8, two down-samplings, 64 x 32 images, 16 bottleneck channels in vectors of 4,
8 centres, batch 2) with two synthetic batches, fp32 and bf16."""
import pytest
import torch

from jpdse_hip import ops, F32
import hip_util as hu
from test_hip_vq_encoder import _trainer, _batch, N, H, W, C, D, L, DOWN, CODE_LEN, DTYPES

pytestmark = pytest.mark.gpu
DEV = hu.DEV
TOL = hu.RTOL[F32]
GROUPS = C // D
PER_GROUP = N * (H >> DOWN) * (W >> DOWN)          # indices per channel group of a batch


@pytest.mark.parametrize('dtype', DTYPES)
def test_fit_on_the_encoder_features(dtype):
  tr = _trainer(dtype)
  batches = [_batch(3), _batch(4)]
  xd = batches[0]
  vq = tr.model.netE._vq
  book = vq.vq._code_book
  ptr = book.data_ptr()
  usage0 = tr.get_vq_usage(xd)
  assert usage0.dtype == torch.int64 and tuple(usage0.shape) == (GROUPS, L)
  assert torch.equal(usage0.sum(dim=1).cpu(), torch.full((GROUPS,), PER_GROUP))
  out = tr.fit_vq_code_book(batches, n_iter=4, init='current')
  assert book.data_ptr() == ptr and book.requires_grad
  assert len(out['distortion']) == 5 and len(out['dead']) == 4 and len(out['reseeded']) == 4
  assert out['distortion'][-1] <= out['distortion'][0]
  # the last entry, recomputed from the features, the hard assignment and torch
  enc = tr.model.netE
  with torch.no_grad():
    feats = []
    for b in batches:
      x = ops.nchw_to_nhwc(b['image'].to(DEV).float().contiguous(), tr.model.cdtype)
      enc.train(False)
      feats.append(enc.vq_features(x))
    assert all(f.shape == (N * CODE_LEN, D) for f in feats)
    assert feats[0].dtype == (torch.float32 if dtype == 'fp32' else torch.bfloat16)
    total, count = 0.0, 0
    for f in feats:
      index, _ = ops.vq_hard_fwd(f.contiguous(), book.detach())
      diff = f.double() - book.detach().double()[index.long()]
      total += float((diff * diff).sum())
      count += f.shape[0]
  want = total / count
  assert abs(out['distortion'][-1] - want) <= TOL * want, (out['distortion'][-1], want)
  assert int(out['counts'].sum()) == count
  # the code paths still agree with get_img, bit for bit, under the fitted book
  img = tr.get_img(xd)
  code = tr.get_vq_code(xd)
  assert torch.equal(tr.decode(code, xd), img)
  assert torch.equal(tr.decode_coded(tr.get_coded(xd), xd), img)
  # the usage is the histogram of the code per channel group
  usage = tr.get_vq_usage(xd)
  assert torch.equal(usage.sum(dim=1).cpu(), torch.full((GROUPS,), PER_GROUP))
  per_group = code.view(N, -1, GROUPS)
  for g in range(GROUPS):
    assert torch.equal(usage[g].cpu(), torch.bincount(per_group[:, :, g].reshape(-1).cpu(), minlength=L))
  # training goes on from the fitted book, on the same tensor
  fitted = book.detach().clone()
  tr.step(xd)
  assert book.data_ptr() == ptr and not torch.equal(book.detach(), fitted)


def test_fit_with_sampled_start_is_deterministic():
  books = []
  for _ in range(2):
    tr = _trainer('fp32')
    out = tr.fit_vq_code_book([_batch(3), _batch(4)], n_iter=2, init='sample', seed=11)
    books.append((tr.model.netE._vq.vq._code_book.detach().clone(), out['distortion']))
  assert torch.equal(books[0][0], books[1][0]) and books[0][1] == books[1][1]
  assert books[0][1][-1] <= books[0][1][0]


def test_binarizer_model_refuses_both_calls():
  from ctu.trainers import get_trainer
  from oracle.ctu_cpu import model as omodel
  opt = omodel.default_opt(gpu_ids=[0], print_losses=False, compute_dtype='fp32', ngf=8, ndf=8, n_blocks_global=1,
                           n_downsample_global=2, no_feat_encoding=False, no_encoder_binarization=False, feat_num=3, nef=8,
                           n_downsample_E=DOWN, encoder_binarizer_out_channels=C, no_vgg_loss=True, no_gan_feat_loss=True,
                           no_g_gan_loss=True, no_d_gan_loss=True, skip_unused_losses=True)
  tr = get_trainer(opt)(opt, 'train')
  with pytest.raises(ValueError, match='--encoder_quantizer s2hvq'):
    tr.fit_vq_code_book([_batch()])
  with pytest.raises(ValueError, match='--encoder_quantizer s2hvq'):
    tr.get_vq_usage(_batch())
