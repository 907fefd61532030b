"""GPU: the context-coded index planes of the vector quantizer (vq_plane.hip: ops.vq_plane_encode / vq_plane_decode,
ctu.utils.vqplane, --vq_context_coder) against the pure-Python coder tests/vq_plane_ref.py, which was written from the format
text of DESIGN.md 4.19.  The coder is lossless and deterministic: every comparison is exact.  Sizes: tests/test_vq_plane_host.py
(the device payloads are the reference's, byte for byte, so the size conditions are evaluated there once)."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'jpd-se_amd'), os.path.dirname(os.path.abspath(__file__))):
  if _p not in sys.path:
    sys.path.insert(0, _p)

import vq_plane_cases as cases  # noqa: E402
import vq_plane_ref as pref  # noqa: E402
import jpdse_hip  # noqa: E402
from jpdse_hip import ops, VqPlaneDecodeArgs  # noqa: E402

_shape = dict(argnames='shape', argvalues=cases.SHAPES, ids=cases.shape_id)
DEV = torch.device('cuda', 0)


def _dev(v):
  return torch.from_numpy(np.array(v, dtype=np.int32)).to(DEV)


def test_the_inputs_exercise_carry_propagation():
  """Asserted on the reference's counters (CPU work, but it guards what the device tests below can show): among the uniform and
  correlated inputs there is a carry that ran through two pending 0xFF bytes, and plain carries are plentiful."""
  total = cases.carry_counters()
  print('carries %d, longest pending run %d, carries into a run >= 2: %d' % (total.carries, total.longest_run,
                                                                         total.carries_into_run2))
  assert total.carries_into_run2 >= 1 and total.longest_run >= 2 and total.carries >= 100


@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize(**_shape)
def test_device_coder_against_the_reference(shape, kind):
  h, w, G, L, strip_rows = shape
  v, want, _ = cases.reference(shape, kind)
  index = _dev(v)
  # 1. the device payload is the reference's, byte for byte (a set status bit raises inside the call)
  got = ops.vq_plane_encode(index, *shape)
  assert isinstance(got, bytes)
  print('%s %s: %d bytes (capacity %d)' % (cases.shape_id(shape), kind, len(got), pref.capacity(*shape)))
  assert len(got) == len(want), (len(got), len(want))
  assert got == want, 'first difference at byte %d' % next(i for i in range(len(want)) if got[i] != want[i])
  # 2. the device decoder on the REFERENCE's payload
  dec = ops.vq_plane_decode(want, h, w, G, L, strip_rows, DEV)
  assert dec.dtype == torch.int32 and tuple(dec.shape) == (h * w * G,) and dec.device == index.device
  assert torch.equal(dec, index)
  # 3. and on the device encoder's own
  assert torch.equal(ops.vq_plane_decode(got, h, w, G, L, strip_rows, DEV), index)
  # 4. a second encode gives identical bytes
  assert ops.vq_plane_encode(index, *shape) == got


# ---- hostile and wrong input: the clipped paths of the format -------------------------------------------------------------------
HOSTILE = (16, 8, 5, 100, 3)                  # 30 streams; the last strip has one row


def _raw_decode(arena, at, nbytes, shape, guard=64):
  """jpdse_vq_plane_decode on the nbytes at arena[at:], straight through the C ABI (ops refuses a table that does not add
  up): (the indices, the status word, the guard words behind the output)."""
  h, w, G, L, strip_rows = shape
  M = h * w * G
  out = torch.full((M + guard,), -7, dtype=torch.int32, device=DEV)
  status = torch.zeros(1, dtype=torch.int32, device=DEV)
  args = VqPlaneDecodeArgs(h, w, G, L, strip_rows, arena.data_ptr() + at, nbytes, out.data_ptr(), status.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
  jpdse_hip.check(jpdse_hip.lib().jpdse_vq_plane_decode(ctypes.byref(args)), 'vq_plane_decode')
  torch.cuda.synchronize()
  return out[:M].cpu().tolist(), int(status.item()), out[M:].cpu().tolist()


def _clipped_streams(payload, S):
  """The streams a decoder reads from an UNTRUSTED payload (stream_span): a table entry that does not lie
  inside the bytes present reads as 0, every stream is clipped to them."""
  have = len(payload)
  lens = [struct.unpack_from('<I', payload, 4 * j)[0] if 4 * j + 4 <= have else 0 for j in range(S)]
  out, at = [], 4 * S
  for n in lens:
    start = min(at, have)
    out.append(payload[start:min(start + n, have)])
    at += n
  return out


def test_all_ones_bytes_decode_inside_the_alphabet():
  h, w, G, L, strip_rows = HOSTILE
  S, body = 30, 60
  payload = b''.join(struct.pack('<I', body) for _ in range(S)) + b'\xff' * (S * body)
  want, clipped = pref.decode_streams(pref.split_payload(payload, S), *HOSTILE)
  assert clipped and max(want) == L - 1
  arena = torch.frombuffer(bytearray(payload), dtype=torch.uint8).to(DEV)
  got, status, guard = _raw_decode(arena, 0, len(payload), HOSTILE)
  assert min(got) >= 0 and max(got) < L and got == want
  assert status == 2 and guard == [-7] * len(guard)
  with pytest.raises(ValueError, match='outside'):
    ops.vq_plane_decode(payload, h, w, G, L, strip_rows, DEV)


@pytest.mark.parametrize('shape', [HOSTILE, (12, 4, 16, 257, 2)], ids=cases.shape_id)
def test_a_lying_length_table_is_clipped_to_the_payload(shape):
  """The payload sits at the very end of its allocation; the table claims more than is there (one entry of 2^32 - 1, the
  others doubled), and in further runs the buffer ends inside a stream and at the end of the table.  The decoder reads what
  stream_span gives it and zeros beyond: the output equals the reference decoder's on the clipped streams, and the words behind
  it are untouched."""
  h, w, G, L, strip_rows = shape
  S = pref.strips(h, strip_rows) * G
  good = cases.reference(shape, 'correlated')[1]
  lens = list(struct.unpack_from('<%dI' % S, good))
  lens = [2 * n for n in lens]
  lens[S // 2] = 0xFFFFFFFF
  lying = struct.pack('<%dI' % S, *lens) + good[4 * S:]
  for payload in (lying, lying[:4 * S + 100], good[:4 * S]):
    arena = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    at = arena.numel() - len(payload)
    arena[at:] = torch.frombuffer(bytearray(payload), dtype=torch.uint8).to(DEV)
    want, _ = pref.decode_streams(_clipped_streams(payload, S), *shape)
    got, status, guard = _raw_decode(arena, at, len(payload), shape)
    assert min(got) >= 0 and max(got) < L
    assert got == want
    assert status in (0, 2) and guard == [-7] * len(guard)
  with pytest.raises(ValueError, match='length table sums to'):
    ops.vq_plane_decode(lying, h, w, G, L, strip_rows, DEV)


@pytest.mark.parametrize('bad', [-1, 'L', 1 << 30, -(1 << 31)])
def test_encode_refuses_an_index_outside_the_alphabet(bad):
  h, w, G, L, strip_rows = HOSTILE
  v = cases.reference(HOSTILE, 'correlated')[0].copy()
  v[317] = L if bad == 'L' else bad
  with pytest.raises(ValueError, match='outside'):
    ops.vq_plane_encode(_dev(v), *HOSTILE)
  v[317] = L - 1
  assert pref.decode(ops.vq_plane_encode(_dev(v), *HOSTILE), *HOSTILE) == v.tolist()      # and the call is still usable


# ---- end to end: the tiny s2hvq trainer of tests/test_hip_vq_encoder.py -------------------------------------------------------
N, H, W, C, D, L_VQ, DOWN = 2, 64, 32, 16, 4, 8, 2
PLANES = (H >> DOWN, W >> DOWN, C // D)
CODE_LEN = PLANES[0] * PLANES[1] * PLANES[2]
_shared = {}


def _trainer(**over):
  from ctu.trainers import get_trainer
  from oracle.ctu_cpu import model as omodel
  kw = dict(gpu_ids=[0], print_losses=False, compute_dtype='fp32', ngf=8, ndf=8, n_blocks_global=1, n_downsample_global=2,
            no_feat_encoding=False, no_encoder_binarization=False, feat_num=3, nef=8, n_downsample_E=DOWN,
            encoder_binarizer_out_channels=C, encoder_quantizer='s2hvq', vq_n_center=L_VQ, vq_center_size=D, vq_sigma=10.0,
            no_vgg_loss=True, no_gan_feat_loss=True, no_g_gan_loss=True, no_d_gan_loss=True, skip_unused_losses=True)
  kw.update(over)
  opt = omodel.default_opt(**kw)
  torch.manual_seed(1234)
  tr = get_trainer(opt)(opt, 'train')
  with torch.no_grad():                          # a code book at the scale of the features: more than one centre in use
    tr.model.netE._vq.vq._code_book.mul_(0.05)
  return tr


def _setup():
  """(flag-on trainer, flag-off trainer with the same weights, batch, get_img of the batch), built once."""
  if not _shared:
    from oracle.ctu_cpu import model as omodel
    on, off = _trainer(vq_context_coder=True), _trainer()
    xd = omodel.synthetic_batch(N, H, W, seed=3)
    img = on.get_img(xd).clone()
    assert torch.equal(off.get_img(xd), img)    # same seed, same weights
    _shared['v'] = (on, off, xd, img)
  return _shared['v']


def test_flag_on_files_decode_to_get_img_and_are_never_larger():
  from ctu.utils import vqplane
  on, off, xd, img = _setup()
  assert on.model.codec.context_coder is True and off.model.codec.context_coder is False
  receiver = {'label': xd['label'], 'instance': xd['instance']}
  blobs, plain = on.get_coded(xd), off.get_coded(xd)
  assert len(blobs) == len(plain) == N and all(isinstance(b, bytes) for b in blobs)
  assert torch.equal(on.decode_coded(blobs, receiver), img)
  for b, p in zip(blobs, plain):
    print('flag on: %s of %d bytes, flag off: .jpdv of %d bytes' % (b[:4].decode(), len(b), len(p)))
    assert p[:4] == b'JPDV' and b[:4] in (b'JPDV', b'JPDW') and len(b) <= len(p)
    assert b == p if b[:4] == b'JPDV' else len(b) < len(p)
  coded, _ = on.get_coded_rate(xd)
  assert coded == sum(8.0 * len(b) / (H * W) for b in blobs) / N
  # a receiver needs no flag
  assert torch.equal(off.decode_coded(blobs, receiver), img)
  # a header that does not fit the label map or the code book is refused on the host
  code = on.get_vq_code(xd)
  with pytest.raises(ValueError, match='holds planes of'):
    off.decode_coded([vqplane.write_planes(None, code[0], (PLANES[1], PLANES[0], PLANES[2]), L_VQ)] * N, receiver)
  with pytest.raises(ValueError, match='n_center 16'):
    off.decode_coded([vqplane.write_planes(None, code[0], PLANES, 16)] * N, receiver)


@pytest.mark.parametrize('strip_rows', [8, 3, 64])
def test_forced_jpdw_blobs_round_trip(strip_rows, tmp_path):
  """.jpdw blobs straight from vqplane.write_planes, whichever container get_coded would have chosen: through the file, the
  reader, the reference coder and the flag-off receiver."""
  from ctu.utils import vqplane
  on, off, xd, img = _setup()
  code = on.get_vq_code(xd)
  assert code.dtype == torch.int64 and tuple(code.shape) == (N, CODE_LEN)
  blobs = []
  for i in range(N):
    path = str(tmp_path / ('c%d%s' % (i, vqplane.SUFFIX)))
    blob = vqplane.write_planes(path, code[i], PLANES, L_VQ, strip_rows)
    assert open(path, 'rb').read() == blob and vqplane.coded_bits(blob) == 8 * os.path.getsize(path)
    assert struct.unpack_from('<4sIIIIIII', blob) == (b'JPDW', 1) + PLANES + (L_VQ, strip_rows, 1)
    assert blob[32:] == pref.encode(code[i].cpu().tolist(), *PLANES, L_VQ, strip_rows)
    for src in (blob, path):
      back, planes, n_center = vqplane.read_planes(src, DEV)
      assert back.dtype == torch.int64 and planes == PLANES and n_center == L_VQ and torch.equal(back, code[i])
    blobs.append(blob)
  receiver = {'label': xd['label'], 'instance': xd['instance']}
  assert torch.equal(off.decode_coded(blobs, receiver), img)
  assert torch.equal(on.decode_coded([blobs[0], off.get_coded(xd)[1]], receiver), img)      # one of each in a batch
