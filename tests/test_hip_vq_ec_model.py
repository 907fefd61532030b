"""GPU tests of the entropy-constrained code on the model and the trainer (VQIndexCodec.code, get_vq_code / get_coded_ec /
get_coded_rate_ec / get_vq_ec_report).  One small configuration, as tests/test_hip_vq_encoder.py builds it:
ngf 8, nef 8, 32 x 64 images, a bottleneck of 16 channels in vectors of 4, batch 2 -- with 64 centres, not 8: at 3 bits an
index the 512 indices of an image pack into 192 bytes, which no coded file of 32 streams undercuts, so every code, constant or
not, would be stored as the same packed file of 220 bytes and a rate could not show in a file size."""
import pytest
import torch

from oracle.ctu_cpu import model as omodel
import hip_util as hu

pytestmark = pytest.mark.gpu
N, H, W, C, D, L, DOWN = 2, 32, 64, 16, 4, 64, 2
CODE_LEN = (H >> DOWN) * (W >> DOWN) * (C // D)
_shared = {}


def _trainer(key, **over):
  if key not in _shared:
    from ctu.trainers import get_trainer
    kw = dict(gpu_ids=[0], print_losses=False, compute_dtype='bf16', ngf=8, ndf=8, n_blocks_global=1, n_downsample_global=2,
              no_feat_encoding=False, no_encoder_binarization=False, feat_num=3, nef=8, n_downsample_E=DOWN,
              encoder_binarizer_out_channels=C, no_vgg_loss=True, no_gan_feat_loss=True, no_g_gan_loss=True, no_d_gan_loss=True,
              skip_unused_losses=True)
    kw.update(over)
    opt = omodel.default_opt(**kw)
    torch.manual_seed(1234)
    tr = get_trainer(opt)(opt, 'train')
    xd = omodel.synthetic_batch(N, H, W, seed=3)
    if 'encoder_quantizer' in over:      # a code book fitted to the bottleneck's features: every centre in use, a varied code
      tr.fit_vq_code_book([xd], n_iter=2)
    _shared[key] = (tr, xd)
  return _shared[key]


def _vq_trainer(context=False):
  over = dict(encoder_quantizer='s2hvq', vq_n_center=L, vq_center_size=D, vq_sigma=10.0)
  if context:
    over['vq_context_coder'] = True
  return _trainer('ctx' if context else 'vq', **over)


def test_the_defaults_give_the_plain_code():
  tr, xd = _vq_trainer()
  plain = tr.get_vq_code(xd)
  assert torch.equal(tr.get_vq_code(xd, rate_lambda=0), plain) and torch.equal(tr.get_vq_code(xd, rate_lambda=0.0, n_iter=5), plain)
  assert tr.get_coded_ec(xd) == tr.get_coded(xd) and tr.get_coded_ec(xd, rate_lambda=0) == tr.get_coded(xd)
  assert tr.get_coded_rate_ec(xd, rate_lambda=0) == tr.get_coded_rate(xd)


@pytest.mark.parametrize('context', [False, True])
def test_the_receiver_takes_the_constrained_code_unchanged(context):
  tr, xd = _vq_trainer(context)
  code = tr.get_vq_code(xd, rate_lambda=1.0)
  assert code.dtype == torch.int64 and tuple(code.shape) == (N, CODE_LEN)
  assert int(code.min()) >= 0 and int(code.max()) < L
  blobs = tr.get_coded_ec(xd, rate_lambda=1.0)
  assert len(blobs) == N and all(isinstance(b, bytes) for b in blobs)
  assert torch.equal(tr.decode_coded(blobs, xd), tr.decode(code, xd))
  reports = tr.get_vq_ec_report(xd, 1.0)
  assert len(reports) == N and all(len(r['cost']) == 3 for r in reports)
  assert all(r['bits'][-1] <= r['bits'][0] for r in reports)


def test_a_huge_multiplier_shrinks_the_files():
  """With the context coder on: a .jpdv file of 32 streams pays 12 bytes a stream, 384 in all, as much as the packed indices of
  a 32 x 64 image take (measured: 412 bytes for the plain and for the constant code alike), so at this size only the .jpdw file
  of a constant plane can undercut the packed one."""
  tr, xd = _vq_trainer(True)
  plain, small = tr.get_coded(xd), tr.get_coded_ec(xd, rate_lambda=1e6)
  assert all(len(s) < len(p) for s, p in zip(small, plain)), ([len(b) for b in small], [len(b) for b in plain])
  assert tr.get_coded_rate_ec(xd, rate_lambda=1e6)[0] < tr.get_coded_rate(xd)[0]
  code = tr.get_vq_code(xd, rate_lambda=1e6).view(N, -1, C // D)
  assert bool((code == code[:, :1, :]).all())      # a constant plane per image and group


def test_the_binarizer_refuses():
  tr, xd = _trainer('bin')
  for call in (tr.get_coded_ec, tr.get_coded_rate_ec):
    with pytest.raises(ValueError, match='--encoder_quantizer s2hvq'):
      call(xd, rate_lambda=1.0)
  with pytest.raises(ValueError, match='--encoder_quantizer s2hvq'):
    tr.get_vq_code(xd, rate_lambda=1.0)
  assert tr.get_coded_ec(xd) == tr.get_coded(xd)
