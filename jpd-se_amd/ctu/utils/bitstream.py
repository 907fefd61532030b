"""The stored form of the learned codec's bitstream (extension; the reference never writes its code to a file): ONE image
per file.

  offset  bytes  field (all little-endian)
       0      4  magic b'JPDC'
       4      4  format version, uint32 (1)
       8      4  C   code channels (the binarizer's output channels)
      12      4  H   code height (image height >> n_downsample_E)
      16      4  W   code width
      20   ceil(C*H*W / 8)  the code: element e = (c*H + y)*W + x in bit 7 - (e & 7) of byte e >> 3 -- a row of
                 trainer.get_code(x_dict, packed=True) as it is; the unused low bits of the last byte are written as 0

Nothing else: no entropy coding, no image size (the receiver takes it from the label map it decodes with).  The file size
is therefore the honest rate of the uncoded bitstream: 8 * (20 + ceil(bits / 8)) bits.
"""
import struct

import torch

from . import container

MAGIC = b'JPDC'
VERSION = 1
_HEADER = struct.Struct('<4sIIII')
HEADER_BYTES = _HEADER.size


def payload_bytes(code_shape):
  C, H, W = (int(v) for v in code_shape)
  return (C * H * W + 7) // 8


def write_code(path, packed_row, code_shape):
  """Write one image's packed code (uint8 [ceil(C*H*W / 8)], any device: a row of get_code(packed=True)) with its
  code_shape = (C, H, W) (Encoder.code_shape).  Returns the number of bytes written."""
  C, H, W = (int(v) for v in code_shape)
  if min(C, H, W) < 1 or max(C, H, W) >= 1 << 32:
    raise ValueError('write_code: bad code shape %r' % (tuple(code_shape),))
  row = container.packed_row(packed_row, payload_bytes((C, H, W)), (C, H, W), 'write_code')
  data = _HEADER.pack(MAGIC, VERSION, C, H, W) + row.cpu().contiguous().numpy().tobytes()
  with open(path, 'wb') as fh:
    fh.write(data)
  return len(data)


def read_code(path):
  """(packed_row, (C, H, W)) of a file write_code wrote: a uint8 CPU tensor [ceil(C*H*W / 8)] and the code shape.
  ValueError on a wrong magic, an unknown version, a truncated or an over-long payload."""
  data = container.read_file(path)
  C, H, W = container.header(data, _HEADER, MAGIC, VERSION, 'code', path)
  if min(C, H, W) < 1:
    raise ValueError('%s: empty code shape (%d, %d, %d)' % (path, C, H, W))
  container.check_raw_body(len(data) - HEADER_BYTES, payload_bytes((C, H, W)), path, 'payload', 'a %d x %d x %d code needs' % (C, H, W),
                           trailing='bytes')
  row = torch.frombuffer(bytearray(data[HEADER_BYTES:]), dtype=torch.uint8)
  return row, (C, H, W)
