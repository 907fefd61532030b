"""The entropy-coded file of the learned codec's bitstream (extension; the reference never writes a coded stream; the format of
the coded payload: DESIGN.md 4.8): ONE image per file, suffix .jpda.

  offset  bytes  field (all little-endian)
       0      4  magic b'JPDA'
       4      4  format version, uint32 (1)
       8      4  C   code channels
      12      4  H   code height
      16      4  W   code width
      20      4  mode, uint32: 1 = coded payload, 0 = raw packed payload
      24         mode 1: C uint32 stream lengths, then the C range-coded streams in channel order (what
                 trainer.get_coded returns for the image); mode 0: the ceil(C*H*W / 8) bytes of a .jpdc file's payload
                 (ctu.utils.bitstream: a row of trainer.get_code(x_dict, packed=True))

write_coded stores the raw form whenever the coded payload is not smaller, so a .jpda file is never more than 4 bytes (the
mode word) larger than the .jpdc file of the same code.  The file size is the rate of the coded bitstream:
8 * file_bytes(...) bits.  Everything here runs on the host; nothing touches the device library.
"""
import struct

import torch

from jpdse_hip import streams
from . import bitstream, container

MAGIC = b'JPDA'
VERSION = 1
SUFFIX = '.jpda'
MODE_RAW, MODE_CODED = 0, 1
_HEADER = struct.Struct('<4sIIIII')
HEADER_BYTES = _HEADER.size


def _shape(code_shape, who):
  C, H, W = (int(v) for v in code_shape)
  if min(C, H, W) < 1 or max(C, H, W) >= 1 << 32:
    raise ValueError('%s: bad code shape %r' % (who, tuple(code_shape)))
  return C, H, W


def check_payload(payload, C, who='payload'):
  """ValueError unless `payload` is bytes holding a table of C uint32 lengths that add up to the bytes after it."""
  streams.check_payload(payload, C, who, who + ': a coded payload is bytes, got %s')


def mode_of(payload_len, code_shape):
  """The mode write_coded picks for a coded payload of that many bytes: raw unless coding made it smaller."""
  return MODE_CODED if payload_len < bitstream.payload_bytes(code_shape) else MODE_RAW


def file_bytes(payload_len, code_shape):
  """Size of the file write_coded writes for a coded payload of that many bytes."""
  return HEADER_BYTES + min(int(payload_len), bitstream.payload_bytes(code_shape))


def write_coded(path, payload, packed_row, code_shape):
  """Write one image: `payload` (bytes: the image's entry of trainer.get_coded) or, when that is not smaller, `packed_row`
  (uint8 [ceil(C*H*W / 8)]: the image's row of get_code(packed=True)).  Returns the number of bytes written."""
  C, H, W = _shape(code_shape, 'write_coded')
  check_payload(payload, C, 'write_coded')
  row = container.packed_row(packed_row, bitstream.payload_bytes((C, H, W)), (C, H, W), 'write_coded')
  mode = mode_of(len(payload), (C, H, W))
  body = bytes(payload) if mode == MODE_CODED else row.cpu().contiguous().numpy().tobytes()
  data = _HEADER.pack(MAGIC, VERSION, C, H, W, mode) + body
  with open(path, 'wb') as fh:
    fh.write(data)
  return len(data)


def read_coded(path):
  """(payload, mode, (C, H, W)) of a file write_coded wrote.  mode 1: payload = the coded bytes; mode 0: payload = the packed
  row, a uint8 CPU tensor [ceil(C*H*W / 8)] as bitstream.read_code returns it.  ValueError on a wrong magic, an unknown
  version or mode, an empty shape, truncated data, trailing bytes, and a mode-1 length table that does not add up."""
  data = container.read_file(path)
  C, H, W, mode = container.header(data, _HEADER, MAGIC, VERSION, 'coded code', path)
  if mode not in (MODE_RAW, MODE_CODED):
    raise ValueError('%s: unknown mode %d (0 = raw, 1 = coded)' % (path, mode))
  if min(C, H, W) < 1:
    raise ValueError('%s: empty code shape (%d, %d, %d)' % (path, C, H, W))
  body = data[HEADER_BYTES:]
  if mode == MODE_RAW:
    container.check_raw_body(len(body), bitstream.payload_bytes((C, H, W)), path, 'payload', 'a %d x %d x %d code needs' % (C, H, W))
    return torch.frombuffer(bytearray(body), dtype=torch.uint8), mode, (C, H, W)
  check_payload(bytes(body), C, path)      # mode 1 has no size of its own: truncation and trailing bytes show here
  return bytes(body), mode, (C, H, W)
