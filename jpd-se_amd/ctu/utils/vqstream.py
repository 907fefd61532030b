"""The coded file of a vector-quantised code: the indices of `ctu.quantizers.S2HVQ` as bytes (extension; the reference never
writes its code; the format of the coded payload: DESIGN.md 4.14).  ONE code tensor per file, suffix .jpdv.

  offset  bytes  field (all little-endian)
       0      4  magic b'JPDV'
       4      4  format version, uint32 (1)
       8      4  n          rows of the code
      12      4  code_len   indices per row; M = n * code_len
      16      4  L          n_center, 2 .. 512; an index takes nb = max(1, bit_length(L - 1)) bits
      20      4  S          streams of the coded payload, 1 .. min(M, 65535); 0 in mode 0
      24      4  mode, uint32: 1 = coded payload, 0 = packed indices
      28         mode 1: S uint32 stream lengths, then the S range-coded streams (what ops.vq_index_encode returns)
                 mode 0: the M indices in row-major order, nb bits each, packed LSB-first into ceil(M * nb / 8) bytes (bit j
                 of the packed string is bit j % 8 of byte j // 8; an index's least significant bit comes first; the unused
                 high bits of the last byte are 0)

write_indices stores the packed form whenever the coded payload is not smaller.  The file size is the rate of the code:
coded_bits = 8 * file bytes, header included.  The header, the refusals and the packing run on the host (numpy); the coder
itself is the device library's (there is no CPU coder here).
"""
import struct

import numpy as np
import torch

from jpdse_hip import ops, streams
from . import container

MAGIC = b'JPDV'
VERSION = 1
SUFFIX = '.jpdv'
MODE_PACKED, MODE_CODED = 0, 1
_HEADER = struct.Struct('<4sIIIIII')
HEADER_BYTES = _HEADER.size
MAX_N_CENTER = ops.VQ_MAX_L
MAX_STREAMS = streams.VQ_INDEX_MAX_S

index_bits = streams.vq_index_bits


def packed_bytes(M, n_center):
  """Size of the mode-0 body of M indices of an alphabet of n_center."""
  return (int(M) * index_bits(n_center) + 7) // 8


def pack_indices(values, nb):
  """The 1-D integer array `values`, each in [0, 2^nb), as nb bits each, LSB-first -> bytes of ceil(len * nb / 8)."""
  v = np.asarray(values, dtype=np.int64).reshape(-1)
  if v.size and (v.min() < 0 or v.max() >= 1 << nb):
    raise ValueError('pack_indices: a value outside [0, %d)' % (1 << nb))
  bits = ((v[:, None] >> np.arange(nb, dtype=np.int64)[None, :]) & 1).astype(np.uint8).reshape(-1)
  return np.packbits(bits, bitorder='little').tobytes()


def unpack_indices(data, M, nb):
  """The inverse: int64 numpy array [M].  ValueError unless `data` is exactly ceil(M * nb / 8) bytes with zero padding bits."""
  M, nb = int(M), int(nb)
  want = (M * nb + 7) // 8
  if len(data) != want:
    raise ValueError('unpack_indices: %d bytes, %d indices of %d bits take %d' % (len(data), M, nb, want))
  bits = np.unpackbits(np.frombuffer(bytes(data), dtype=np.uint8), bitorder='little')
  if bits[M * nb:].any():
    raise ValueError('unpack_indices: non-zero padding bits after the last index')
  weights = (1 << np.arange(nb, dtype=np.int64))
  return (bits[:M * nb].reshape(M, nb).astype(np.int64) * weights[None, :]).sum(axis=1)


def _limits(n, code_len, L, who):
  if min(n, code_len) < 1:
    raise ValueError('%s: empty code shape (%d, %d)' % (who, n, code_len))
  if not 2 <= L <= MAX_N_CENTER:
    raise ValueError('%s: n_center L = %d, outside 2 .. %d' % (who, L, MAX_N_CENTER))
  if n * code_len * index_bits(L) >= 1 << 31:
    raise ValueError('%s: a code of %d x %d indices of %d bits is beyond the coder\'s limits' % (who, n, code_len, index_bits(L)))


def build_blob(shape, n_center, n_streams, payload, indices):
  """The file's bytes for a code of `shape` = (n, code_len): `payload` (bytes: ops.vq_index_encode of the flat indices in
  n_streams streams) in mode 1 or, when that is not smaller than the packed form, `indices` (flat integer array, row-major)
  packed in mode 0.  Host only."""
  n, code_len = (int(v) for v in shape)
  L, S = int(n_center), int(n_streams)
  _limits(n, code_len, L, 'build_blob')
  M = n * code_len
  if not 1 <= S <= min(M, MAX_STREAMS):
    raise ValueError('build_blob: S = %d streams, outside 1 .. min(M = %d, %d)' % (S, M, MAX_STREAMS))
  streams.check_payload(payload, S, 'build_blob', 'build_blob: a coded payload is bytes, got %s')
  flat = np.asarray(indices).reshape(-1)
  if flat.size != M:
    raise ValueError('build_blob: %d indices for a code of %d x %d' % (flat.size, n, code_len))
  if flat.min() < 0 or flat.max() >= L:
    raise ValueError('build_blob: an index outside [0, %d)' % L)
  if len(payload) < packed_bytes(M, L):
    return _HEADER.pack(MAGIC, VERSION, n, code_len, L, S, MODE_CODED) + bytes(payload)
  return _HEADER.pack(MAGIC, VERSION, n, code_len, L, 0, MODE_PACKED) + pack_indices(flat, index_bits(L))


def parse_blob(blob, who='blob'):
  """(n, code_len, L, S, mode, body) of a file's bytes; body: the coded payload (mode 1) or the int64 numpy array [M] of the
  unpacked indices (mode 0).  ValueError on a wrong magic, an unknown version or mode, L or S out of range, an empty shape,
  truncated data, trailing bytes, a mode-1 length table that does not add up and a mode-0 value >= L.  Host only."""
  if not isinstance(blob, (bytes, bytearray)):
    raise ValueError('%s: a .jpdv blob is bytes, got %s' % (who, type(blob).__name__))
  n, code_len, L, S, mode = container.header(blob, _HEADER, MAGIC, VERSION, 'coded index', who,
                                             short='%s: truncated, %d bytes are shorter than the %d-byte header')
  if mode not in (MODE_PACKED, MODE_CODED):
    raise ValueError('%s: unknown mode %d (0 = packed, 1 = coded)' % (who, mode))
  _limits(n, code_len, L, who)
  M = n * code_len
  body = bytes(blob[HEADER_BYTES:])
  if mode == MODE_PACKED:
    if S != 0:
      raise ValueError('%s: S = %d streams in mode 0, which stores 0' % (who, S))
    container.check_raw_body(len(body), packed_bytes(M, L), who, 'body', 'that %d indices of %d bits take' % (M, index_bits(L)))
    values = unpack_indices(body, M, index_bits(L))
    if values.size and values.max() >= L:
      raise ValueError('%s: a packed value %d outside [0, %d)' % (who, int(values.max()), L))
    return n, code_len, L, S, mode, values
  if not 1 <= S <= min(M, MAX_STREAMS):
    raise ValueError('%s: S = %d streams, outside 1 .. min(M = %d, %d)' % (who, S, M, MAX_STREAMS))
  streams.check_length_table(body, S, who)     # mode 1 has no size of its own: truncation and trailing bytes show here
  return n, code_len, L, S, mode, body


def clamp_streams(n_streams, M):
  """The stream count write_indices codes M indices in when asked for n_streams: at least 1, at most M and the coder's limit."""
  return max(1, min(int(n_streams), int(M), MAX_STREAMS))


def write_indices(path, code, n_center, n_streams=64):
  """code: the int64 (n, code_len) device tensor of S2HVQ.encode(..., train=False, raw=False) -> the file's bytes, also
  written to `path` unless that is None.  n_streams is clamped to the number of indices.  ValueError for an index outside
  [0, n_center)."""
  if not torch.is_tensor(code) or code.dim() != 2 or code.dtype != torch.int64:
    raise ValueError('write_indices: the code is an int64 (n, code_len) tensor')
  n, code_len, L = int(code.shape[0]), int(code.shape[1]), int(n_center)
  _limits(n, code_len, L, 'write_indices')
  M = n * code_len
  S = clamp_streams(n_streams, M)
  flat = code.contiguous().view(-1)
  if bool(((flat < 0) | (flat >= L)).any()):      # before the cast to the coder's int32 could fold a far value into range
    raise ValueError('write_indices: an index outside [0, %d)' % L)
  payload = ops.vq_index_encode(flat.to(torch.int32), L, S)
  blob = build_blob((n, code_len), L, S, payload, flat.cpu().numpy())
  if path is not None:
    with open(path, 'wb') as fh:
      fh.write(blob)
  return blob


def _read(blob_or_path, device):
  """(code, L) of a blob or file."""
  blob, who = container.load(blob_or_path)
  n, code_len, L, S, mode, body = parse_blob(blob, who)
  dev = torch.device(streams.default_device(device))
  if mode == MODE_PACKED:
    return torch.from_numpy(body.astype(np.int64)).view(n, code_len).to(dev), L
  return ops.vq_index_decode(body, n * code_len, L, S, dev).to(torch.int64).view(n, code_len), L


def read_indices(blob_or_path, device=None):
  """The int64 (n, code_len) code of a blob or file write_indices wrote, on `device` (default: the current GPU).  Every refusal
  of parse_blob is raised on the host before any device call; a packed file (mode 0) needs no device call at all."""
  return _read(blob_or_path, device)[0]


def coded_bits(blob):
  """The rate of a written code: 8 * file bytes, header included."""
  return 8 * len(blob)


def reconstruct(s2h, blob_or_path):
  """(n, d) float32: the indices of the file through the module's code book (ops.vq_decode) -- bit for bit
  s2h.decode(s2h.encode(x, code_len, train=False)) of the x the file was written from."""
  book = s2h.code_book.detach().contiguous()
  code, L = _read(blob_or_path, book.device)
  if L != book.shape[0]:
    raise ValueError('reconstruct: the file was coded for n_center %d, the module has %d' % (L, book.shape[0]))
  y, status = ops.vq_decode(code.view(-1).to(torch.int32), book)
  if int(status.item()) != 0:
    raise ValueError('reconstruct: an index outside [0, %d)' % book.shape[0])
  return y.view(code.shape[0], code.shape[1] * book.shape[1])
