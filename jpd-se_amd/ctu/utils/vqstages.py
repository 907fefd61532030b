"""The coded file of a residual vector-quantised code: the stage codes of `ctu.quantizers.ResidualS2HVQ`, one .jpdv blob
(vqstream.py) per stage, in a container that can be CUT after any stage.  Suffix .jpdr.

  offset  bytes  field (all little-endian)
       0      4  magic b'JPDR'
       4      4  format version, uint32 (1)
       8      4  S          stages, 1 .. 8
      12      4  n          rows of every stage's code
      16      4  code_len   indices per row
      20      4  L          n_center of every stage, 2 .. 512
      24    4 S  the S uint32 byte lengths of the stage blobs
 24 + 4 S        the S blobs in stage order, each exactly what vqstream.write_indices writes for that stage's (n, code_len) code

A receiver that has the first n stages reproduces y^(n): truncate_stages rewrites the header and the length table and copies the
first blobs byte for byte -- no device, no re-coding.  coded_bits = 8 * file bytes, headers included.  Header, length table and
every inner blob's own header are checked on the host before any device call; each failure is a ValueError naming the field.
"""
import struct

import torch

from jpdse_hip import ops, streams
from . import container, vqstream

MAGIC = b'JPDR'
VERSION = 1
SUFFIX = '.jpdr'
_HEADER = struct.Struct('<4sIIIII')
HEADER_BYTES = _HEADER.size
MAX_STAGES = ops.VQ_RES_MAX_STAGES


def build_stages(blobs, n, code_len, n_center):
  """The file's bytes from the S stage blobs (bytes each, in stage order).  Host only; the blobs are not inspected here."""
  blobs = [bytes(b) for b in blobs]
  if not 1 <= len(blobs) <= MAX_STAGES:
    raise ValueError('build_stages: S = %d stages, outside 1 .. %d' % (len(blobs), MAX_STAGES))
  table = struct.pack('<%dI' % len(blobs), *[len(b) for b in blobs])
  return _HEADER.pack(MAGIC, VERSION, len(blobs), int(n), int(code_len), int(n_center)) + table + b''.join(blobs)


def parse_stages(blob, who='blob', stages=None):
  """(S, n, code_len, L, blobs) of a file's bytes, blobs the first `stages` (default: all S) stage blobs.  ValueError on a wrong
  magic, an unknown version, S outside 1 .. 8, an empty shape or L out of range, a length table that is truncated or does not add
  up to the file size, `stages` outside 1 .. S, and an inner blob whose own header disagrees with the outer n, code_len or L (or
  fails vqstream.parse_blob).  Only the first `stages` blobs are looked at.  Host only."""
  if not isinstance(blob, (bytes, bytearray)):
    raise ValueError('%s: a .jpdr blob is bytes, got %s' % (who, type(blob).__name__))
  S, n, code_len, L = container.header(blob, _HEADER, MAGIC, VERSION, 'coded stage', who)
  if not 1 <= S <= MAX_STAGES:
    raise ValueError('%s: S = %d stages, outside 1 .. %d' % (who, S, MAX_STAGES))
  vqstream._limits(n, code_len, L, who)
  start = HEADER_BYTES + 4 * S
  if len(blob) < start:
    raise ValueError('%s: truncated, %d bytes are shorter than the header and its length table of %d stages (%d bytes)'
                     % (who, len(blob), S, start))
  lengths = struct.unpack_from('<%dI' % S, blob, HEADER_BYTES)
  for s, v in enumerate(lengths):
    if v < vqstream.HEADER_BYTES:
      raise ValueError('%s: length table: stage %d takes %d bytes, less than a %d-byte .jpdv header' % (who, s, v, vqstream.HEADER_BYTES))
  container.check_raw_body(len(blob) - start, sum(lengths), who, 'stage', 'that the length table of %d stages adds up to' % S)
  take = S if stages is None else int(stages)
  if not 1 <= take <= S:
    raise ValueError('%s: stages = %r, the file holds 1 .. %d' % (who, stages, S))
  out, at = [], start
  for s in range(take):
    inner = bytes(blob[at:at + lengths[s]])
    at += lengths[s]
    inner_who = '%s: stage %d' % (who, s)
    ni, ci, Li = vqstream.parse_blob(inner, inner_who)[:3]
    for name, got, want in (('n', ni, n), ('code_len', ci, code_len), ('n_center', Li, L)):
      if got != want:
        raise ValueError('%s: its %s = %d, the container says %d' % (inner_who, name, got, want))
    out.append(inner)
  return S, n, code_len, L, out


def write_stages(path, code, n_center, n_streams=64):
  """code: the int64 (S, n, code_len) device tensor of ResidualS2HVQ.encode -> the file's bytes, also written to `path` unless that
  is None.  Every stage is coded on its own by vqstream.write_indices (n_streams streams, clamped).  ValueError for an index
  outside [0, n_center)."""
  if not torch.is_tensor(code) or code.dim() != 3 or code.dtype != torch.int64:
    raise ValueError('write_stages: the code is an int64 (S, n, code_len) tensor')
  if not 1 <= code.shape[0] <= MAX_STAGES:
    raise ValueError('write_stages: S = %d stages, outside 1 .. %d' % (code.shape[0], MAX_STAGES))
  blob = build_stages([vqstream.write_indices(None, code[s], n_center, n_streams) for s in range(code.shape[0])],
                      code.shape[1], code.shape[2], n_center)
  if path is not None:
    with open(path, 'wb') as fh:
      fh.write(blob)
  return blob


def _read(blob_or_path, device, stages):
  blob, who = container.load(blob_or_path)
  S, n, code_len, L, blobs = parse_stages(blob, who, stages)      # every refusal before the first device call
  dev = torch.device(streams.default_device(device))
  return torch.stack([vqstream.read_indices(b, dev) for b in blobs]), L


def read_stages(blob_or_path, device=None, stages=None):
  """The int64 (S', n, code_len) code of the first `stages` (default: all) stages of a blob or file write_stages wrote, on `device`
  (default: the current GPU).  Only those blobs are touched."""
  return _read(blob_or_path, device, stages)[0]


def truncate_stages(blob_or_path, stages):
  """The bytes of a valid .jpdr file that holds the first `stages` stages: a new header and length table, the stage blobs copied
  byte for byte.  Host only."""
  blob, who = container.load(blob_or_path)
  S, n, code_len, L, blobs = parse_stages(blob, who, stages)
  return build_stages(blobs, n, code_len, L)


def coded_bits(blob_or_path, stages=None):
  """The rate of a written code: 8 * file bytes, headers included; with `stages`, of the file cut after that many stages."""
  blob, _ = container.load(blob_or_path)
  return 8 * len(blob if stages is None else truncate_stages(blob, stages))


def reconstruct_stages(rvq, blob_or_path, stages=None):
  """(n, d) float32: the first `stages` stages of the file through the module's code books (ops.vq_res_decode) -- bit for bit
  rvq.decode(rvq.encode(x, code_len), stages) of the x the file was written from."""
  books = rvq.code_books.detach().contiguous()
  code, L = _read(blob_or_path, books.device, stages)
  if L != books.shape[1]:
    raise ValueError('reconstruct_stages: the file was coded for n_center %d, the module has %d' % (L, books.shape[1]))
  return rvq.decode(code)
