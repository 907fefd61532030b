"""GPU: the coded index stream of the vector quantizer (vq_coder.hip: ops.vq_index_encode / vq_index_decode,
ctu.utils.vqstream) against the pure-Python coder tests/vq_coder_ref.py, which was written from the format text of DESIGN.md
4.14.  The coder is lossless and deterministic: every comparison is exact.  Sizes: tests/test_vq_coder_host.py (the device
payloads are the reference's, byte for byte, so the size claims are made there once)."""
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

import vq_coder_cases as cases  # noqa: E402
import vq_coder_ref as vref  # noqa: E402
import jpdse_hip  # noqa: E402
from jpdse_hip import ops, VqIndexDecodeArgs  # noqa: E402

_shape = dict(argnames='shape', argvalues=cases.SHAPES, ids=cases.shape_id)
DEV = torch.device('cuda', 0)


def _dev(v):
  return torch.from_numpy(np.array(v, dtype=np.int32)).to(DEV)


def test_the_inputs_exercise_carry_propagation():
  """Asserted on the reference's counters (CPU work, but it guards what the device tests below can show): among the uniform
  inputs there is a carry that ran through two pending 0xFF bytes, and plain carries are plentiful."""
  total = vref.Counters()
  for shape in cases.SHAPES:
    total.add(cases.reference(shape, 'uniform')[2])
  print('carries %d, longest pending run %d, carries into a run >= 2: %d' % (total.carries, total.longest_run,
                                                                         total.carries_into_run2))
  assert total.carries_into_run2 >= 1 and total.longest_run >= 2 and total.carries >= 100


@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize(**_shape)
def test_device_coder_against_the_reference(shape, kind):
  M, L, S = shape
  v, want, _ = cases.reference(shape, kind)
  index = _dev(v)
  # 1. the device payload is the reference's, byte for byte (a set status bit raises inside the call)
  got = ops.vq_index_encode(index, L, S)
  assert isinstance(got, bytes)
  print('%s %s: %d bytes (capacity %d)' % (cases.shape_id(shape), kind, len(got), vref.capacity(M, L, S)))
  assert len(got) == len(want), (len(got), len(want))
  assert got == want, 'first difference at byte %d' % next(i for i in range(len(want)) if got[i] != want[i])
  # 2. the device decoder on the REFERENCE's payload
  dec = ops.vq_index_decode(want, M, L, S, DEV)
  assert dec.dtype == torch.int32 and tuple(dec.shape) == (M,) and dec.device == index.device
  assert torch.equal(dec, index)
  # 3. and on the device encoder's own
  assert torch.equal(ops.vq_index_decode(got, M, L, S, DEV), index)
  # 4. a second encode gives identical bytes
  assert ops.vq_index_encode(index, L, S) == got


# ---- hostile and wrong input: the clipped paths of the format -------------------------------------------------------------------
def _raw_decode(arena, at, nbytes, M, L, S, guard=64):
  """jpdse_vq_index_decode on the nbytes at arena[at:], straight through the C ABI (ops refuses a table that does not add
  up): (the M indices, the status word, the guard words behind the output)."""
  out = torch.full((M + guard,), -7, dtype=torch.int32, device=DEV)
  status = torch.zeros(1, dtype=torch.int32, device=DEV)
  args = VqIndexDecodeArgs(M, L, S, arena.data_ptr() + at, nbytes, out.data_ptr(), status.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
  jpdse_hip.check(jpdse_hip.lib().jpdse_vq_index_decode(ctypes.byref(args)), 'vq_index_decode')
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
  M, L, S = 3000, 100, 7
  body = 400
  payload = b''.join(struct.pack('<I', body) for _ in range(S)) + b'\xff' * (S * body)
  want, clipped = vref.decode_streams(vref.split_payload(payload, S), M, L, S)
  assert clipped and max(want) == L - 1
  arena = torch.frombuffer(bytearray(payload), dtype=torch.uint8).to(DEV)
  got, status, guard = _raw_decode(arena, 0, len(payload), M, L, S)
  assert min(got) >= 0 and max(got) < L and got == want
  assert status == 2 and guard == [-7] * len(guard)
  with pytest.raises(ValueError, match='outside'):
    ops.vq_index_decode(payload, M, L, S, DEV)


@pytest.mark.parametrize('shape', [(3000, 100, 7), (4096, 257, 130)], ids=cases.shape_id)
def test_a_lying_length_table_is_clipped_to_the_payload(shape):
  """The payload sits at the very end of its allocation; the table claims more than is there (one entry of 2^32 - 1, the
  others doubled), and in a second run the buffer ends inside the table.  The decoder reads what stream_span gives it and
  zeros beyond: the output equals the reference decoder's on the clipped streams, and the words behind it are untouched."""
  M, L, S = shape
  good = cases.reference(shape, 'geometric')[1]
  lens = list(struct.unpack_from('<%dI' % S, good))
  lens = [2 * n for n in lens]
  lens[S // 2] = 0xFFFFFFFF
  lying = struct.pack('<%dI' % S, *lens) + good[4 * S:]
  for payload in (lying, lying[:4 * S + 100], good[:4 * S]):
    arena = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    at = arena.numel() - len(payload)
    arena[at:] = torch.frombuffer(bytearray(payload), dtype=torch.uint8).to(DEV)
    want, _ = vref.decode_streams(_clipped_streams(payload, S), M, L, S)
    got, status, guard = _raw_decode(arena, at, len(payload), M, L, S)
    assert min(got) >= 0 and max(got) < L
    assert got == want
    assert status in (0, 2) and guard == [-7] * len(guard)
  with pytest.raises(ValueError, match='length table sums to'):
    ops.vq_index_decode(lying, M, L, S, DEV)


@pytest.mark.parametrize('bad', [-1, 'L', 1 << 30, -(1 << 31)])
def test_encode_refuses_an_index_outside_the_alphabet(bad):
  M, L, S = 3000, 100, 7
  v = cases.reference((M, L, S), 'geometric')[0].copy()
  v[1500] = L if bad == 'L' else bad
  with pytest.raises(ValueError, match='outside'):
    ops.vq_index_encode(_dev(v), L, S)
  v[1500] = L - 1
  assert vref.decode(ops.vq_index_encode(_dev(v), L, S), M, L, S) == v.tolist()      # and the call is still usable


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def _golden(golden_dir):
  z = np.load(os.path.join(golden_dir, 's2hvq.npz'))
  n = len({k.split('_')[0] for k in z.files})
  return [{k[len('c%d_' % i):]: torch.from_numpy(z[k]) for k in z.files if k.startswith('c%d_' % i)} for i in range(n)]


def test_module_code_through_the_file_and_back(golden_dir, tmp_path):
  from ctu.quantizers import S2HVQ
  from ctu.utils import vqstream
  modes = set()
  for i, gold in enumerate(_golden(golden_dir)):
    n, d, code_len, L = (int(v) for v in gold['cfg'][:4])
    vq = S2HVQ(gold['code_book'].clone(), sigma=float(gold['cfg'][4])).to(DEV).eval()
    x = gold['x'].to(DEV)
    with torch.no_grad():
      code = vq.encode(x, code_len, train=False, raw=False)
      want = vq.decode(vq.encode(x, code_len, train=False))
    assert code.dtype == torch.int64 and tuple(code.shape) == (n, code_len)
    path = str(tmp_path / ('c%d%s' % (i, vqstream.SUFFIX)))
    blob = vqstream.write_indices(path, code, L)
    assert isinstance(blob, bytes) and open(path, 'rb').read() == blob
    header = struct.unpack_from('<4sIIIIII', blob)
    M = n * code_len
    assert header[:5] == (b'JPDV', 1, n, code_len, L) and header[5] == (min(64, M) if header[6] == 1 else 0)
    modes.add(header[6])
    # the payload inside is the reference coder's, and the mode is the smaller form
    flat = code.view(-1).cpu().numpy()
    ref = vref.encode(flat.tolist(), L, min(64, M))
    assert blob == vqstream.build_blob((n, code_len), L, min(64, M), ref, flat)
    for src in (blob, path):
      back = vqstream.read_indices(src, DEV)
      assert back.dtype == torch.int64 and back.device == code.device and torch.equal(back, code)
    got = vqstream.reconstruct(vq, path)
    assert got.dtype == want.dtype and got.shape == want.shape == (n, d) and torch.equal(got, want)
    assert vqstream.coded_bits(blob) == 8 * os.path.getsize(path)
    print('golden %d: %d x %d indices of L = %d: file %d bytes, mode %d' % (i, n, code_len, L, len(blob), header[6]))
    # with one stream per index the table alone outweighs the packed form: mode 0, S stored as 0
    many = vqstream.write_indices(None, code, L, n_streams=1 << 20)
    assert struct.unpack_from('<II', many, 20) == (0, 0) and torch.equal(vqstream.read_indices(many, DEV), code)
  # a skewed code of the bench's alphabet takes mode 1 through the same calls
  v = cases.reference((4096, 64, 64), 'geometric')[0]
  code = torch.from_numpy(v.astype(np.int64)).view(64, 64).to(DEV)
  blob = vqstream.write_indices(None, code, 64)
  assert struct.unpack_from('<II', blob, 20) == (64, 1) and blob[28:] == cases.reference((4096, 64, 64), 'geometric')[1]
  assert torch.equal(vqstream.read_indices(blob, DEV), code)
  for bad in (64, -1, 1 << 32):                     # the last would be 0 after a cast to the coder's int32
    code[17, 5] = bad
    with pytest.raises(ValueError, match='outside'):
      vqstream.write_indices(None, code, 64)
