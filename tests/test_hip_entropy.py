"""GPU: the entropy-coded bitstream of the learned codec (entropy.hip: ops.code_entropy_encode / code_entropy_decode,
trainer.get_coded / decode_coded / get_coded_rate) against the pure-Python coder tests/entropy_ref.py, which was written
from the format text of DESIGN.md 4.8.  The coder is lossless and deterministic: every comparison is exact.

Sizes measured with the reference at the largest shape (3 x 64 x 16 x 33, 12672 raw bytes): see DESIGN.md 4.8."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'jpd-se_amd'), os.path.dirname(os.path.abspath(__file__))):
  if _p not in sys.path:
    sys.path.insert(0, _p)

import code_import_ref as cref  # noqa: E402
import entropy_cases as cases  # noqa: E402
import entropy_ref as eref  # noqa: E402
from jpdse_hip import F32, BF16, ops  # noqa: E402

_shape = dict(argnames='shape', argvalues=cases.SHAPES, ids=cases.shape_id)
DEV = torch.device('cuda', 0)


def _act(b, dtype):
  return ops.nchw_to_nhwc(torch.from_numpy(np.array(b)).to(DEV), dtype)


def _imported(b, dtype):
  """code_import(code_export(b)) on the device: the stored tensor a receiver of the raw code gets, padding lanes included."""
  N, C, H, W = b.shape
  return ops.code_import(ops.code_export(_act(b, dtype), packed=True), N, H, W, C, dtype).t


def test_the_inputs_exercise_carry_propagation():
  """Asserted on the reference's counters (CPU work, but it guards what the device tests below can show): among the inputs
  there is a carry that ran through two or more pending 0xFF bytes, and plain carries are plentiful."""
  total = eref.Counters()
  for shape in cases.SHAPES:
    total.add(cases.reference(shape, 'half')[2])
  print('carries %d, longest pending run %d, carries into a run >= 2: %d' % (total.carries, total.longest_run,
                                                                         total.carries_into_run2))
  assert total.carries_into_run2 >= 1 and total.longest_run >= 2 and total.carries >= 100


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize(**_shape)
def test_device_coder_against_the_reference(shape, kind, dtype):
  N, C, H, W = shape
  b, want, _ = cases.reference(shape, kind)
  # 1. the device encoder's payloads are the reference's, byte for byte (a set status word raises inside the call)
  got = ops.code_entropy_encode(_act(b, dtype))
  assert isinstance(got, list) and len(got) == N and all(isinstance(p, bytes) for p in got)
  for n in range(N):
    assert len(got[n]) == len(want[n]), (n, len(got[n]), len(want[n]))
    assert got[n] == want[n], 'image %d: first difference at byte %d' % (
        n, next(i for i in range(len(want[n])) if got[n][i] != want[n][i]))
  # 2. the device decoder on the REFERENCE's payloads: code_import(code_export(b)), every lane of the stored tensor
  stored = _imported(b, dtype)
  dec = ops.code_entropy_decode(list(want), N, H, W, C, dtype)
  assert dec.dtype == dtype and dec.C == C and tuple(dec.t.shape) == (N, H, W, cref.cpad(C))
  assert torch.equal(dec.t, stored)
  if cref.cpad(C) > C:
    assert bool((dec.t[..., C:] == 0).all())
  assert torch.equal(ops.nhwc_to_nchw(dec).float().cpu(), torch.from_numpy(np.where(b > 0, np.float32(1), np.float32(-1))))
  # 3. and on the device encoder's own
  assert torch.equal(ops.code_entropy_decode(got, N, H, W, C, dtype).t, stored)


def test_encode_is_deterministic_and_ignores_padding_lanes():
  shape = (2, 3, 1, 9)
  b, want, _ = cases.reference(shape, 'half')
  act = _act(b, F32)
  act.t[..., 3:] = 5.0                       # the padding lanes of the input are never coded
  assert ops.code_entropy_encode(act) == list(want) == ops.code_entropy_encode(act)


# ---- end to end -----------------------------------------------------------------------------------------------------------
def _trainer(dtype='fp32'):
  from ctu.trainers import get_trainer
  from ctu.utils.synthetic import default_opt
  opt = default_opt(gpu_ids=[0], print_losses=False, ngf=8, ndf=8, n_blocks_global=1, no_feat_encoding=False,
                    no_encoder_binarization=False, feat_num=3, nef=8, n_downsample_E=4, encoder_binarizer_out_channels=32,
                    compute_dtype=dtype)
  torch.manual_seed(4321)
  return get_trainer(opt)(opt, 'train')


@pytest.fixture(scope='module')
def trainer():
  return _trainer()


def _blob_batch(tr, N, H, W):
  """A batch of piecewise-constant images.  Image 0: a flat background with one 16 x 16 pixel square in a corner -- its code
  is flat with one blob (one code element and the encoder's halo around it).  The others: flat 64 x 64 pixel blocks
  (4 x 4 code elements each).  Spatially correlated codes, in rising order of detail."""
  from ctu.utils.synthetic import synthetic_batch
  xd = synthetic_batch(N, H, W, seed=5)
  g = torch.Generator().manual_seed(9)
  coarse = torch.rand((N, 3, H // 64, W // 64), generator=g) - 0.5
  image = torch.nn.functional.interpolate(coarse, size=(H, W), mode='nearest').contiguous()
  image[0] = torch.tensor([-0.2, 0.1, 0.3]).view(3, 1, 1)
  image[0, :, :16, :16] = torch.tensor([0.4, -0.3, 0.0]).view(3, 1, 1)
  xd['image'] = image
  xd['compressed_img'] = image.clone()
  return xd


@pytest.mark.parametrize('size', [(64, 128), (128, 256)], ids=['64x128', '128x256'])
def test_trainer_round_trip_and_rate(trainer, size, tmp_path):
  from ctu.utils import bitstream, entropy
  H, W = size
  N = 2
  xd = _blob_batch(trainer, N, H, W)
  rx = dict(label=xd['label'].clone(), instance=xd['instance'].clone())
  shape = trainer.model.netE.code_shape(H, W)
  assert shape == (32, H // 16, W // 16)
  packed = trainer.get_code(xd, packed=True)
  payloads = trainer.get_coded(xd)
  assert isinstance(payloads, list) and len(payloads) == N and all(isinstance(p, bytes) for p in payloads)
  # the payloads are the reference coder's for the stored code
  code = cref.import_packed(packed.cpu().numpy(), N, *shape)
  assert payloads == eref.encode(code)
  want = trainer.decode(packed, rx)
  got = trainer.decode_coded(payloads, rx)
  assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)
  # the rate is the size of the files
  sizes, modes = [], []
  for j in range(N):
    path = str(tmp_path / ('i%d%s' % (j, entropy.SUFFIX)))
    n = entropy.write_coded(path, payloads[j], packed[j].cpu(), shape)
    assert n == os.path.getsize(path)
    back, mode, got_shape = entropy.read_coded(path)
    assert got_shape == shape
    if mode == entropy.MODE_CODED:
      assert back == payloads[j]
    else:
      assert torch.equal(back, packed[j].cpu())
    sizes.append(n)
    modes.append(mode)
  coded_bpp, raw_bpp = trainer.get_coded_rate(xd)
  assert isinstance(coded_bpp, float) and isinstance(raw_bpp, float)
  assert coded_bpp == sum(8.0 * n / (H * W) for n in sizes) / N
  assert raw_bpp == 8.0 * (bitstream.HEADER_BYTES + bitstream.payload_bytes(shape)) / (H * W)
  print('%dx%d: raw %d bytes per image, coded payloads %s, files %s, modes %s' % (W, H, bitstream.payload_bytes(shape),
                                                                                [len(p) for p in payloads], sizes, modes))
  if size == (128, 256):
    # 32 streams of 128 symbols: table entry and flush are 8 of a stream's 16 raw bytes, so only the flat-with-a-blob code pays
    assert entropy.MODE_CODED in modes, 'no image of the blob-like batch took mode 1'
    assert coded_bpp < raw_bpp


def test_decode_coded_refusals_leave_the_library_untouched(trainer, monkeypatch):
  import jpdse_hip
  H, W, N = 64, 128, 2
  xd = _blob_batch(trainer, N, H, W)
  rx = dict(label=xd['label'].clone(), instance=xd['instance'].clone())
  good = trainer.get_coded(xd)
  want = trainer.decode_coded(good, rx)
  broken = bytearray(good[1])
  broken[0] ^= 1                               # the first stream length off by one: the table no longer adds up
  touched = lambda: (_ for _ in ()).throw(AssertionError('library touched'))
  with monkeypatch.context() as m:
    m.setattr(jpdse_hip, 'lib', touched)
    m.setattr(ops, 'lib', touched)
    for bad in (good[:1], good + good[:1], [good[0], np.frombuffer(good[1], dtype=np.uint8)], [good[0], None],
                good[0], [good[0], bytes(broken)], [good[0], good[1][:-1]], [good[0], good[1] + b'\0'], [good[0], b'']):
      with pytest.raises(ValueError, match='decode_coded'):
        trainer.decode_coded(bad, rx)
    with pytest.raises(ValueError, match='decode_coded'):
      trainer.decode_coded(good, dict(label=xd['label'][..., :120], instance=xd['instance'][..., :120]))
    for bad in (good[:1], [good[0], None], [good[0], bytes(broken)]):
      with pytest.raises(ValueError, match='code_entropy_decode'):
        ops.code_entropy_decode(bad, N, 4, 8, 32, F32)
  assert torch.equal(trainer.decode_coded(good, rx), want)    # and the trainer is still usable
