"""What the stored forms share (bitstream .jpdc, entropy .jpda, semantics .jpds, vqstream .jpdv: DESIGN.md 4.18; vqplane .jpdw: 4.19; vqstages .jpdr, magic b'JPDR': 4.23): loading a
file or a blob, the start of every header (size, magic, format version), the size check of a raw body and the one-row check of a
packed code.  Each format keeps its own fields, modes and shape checks, and every message is the one its module raised before.
Everything here runs on the host.
"""
import torch

SHORT_HEADER = '%s: %d bytes, shorter than the %d-byte header'


def read_file(path):
  with open(path, 'rb') as fh:
    return fh.read()


def load(blob_or_path):
  """(bytes, who) of a blob (who = 'blob') or of the file at a path (who = the path)."""
  if isinstance(blob_or_path, (bytes, bytearray)):
    return bytes(blob_or_path), 'blob'
  return read_file(blob_or_path), str(blob_or_path)


def header(data, layout, magic, version, noun, who, short=SHORT_HEADER):
  """The fields of `data`'s header (a struct.Struct that starts with the magic and the uint32 format version) after those two.
  ValueError, under the name `who`, for data shorter than the header (`short`: the wording, which differs for .jpdv), a wrong
  magic ('not a <noun> file') and an unknown version."""
  if len(data) < layout.size:
    raise ValueError(short % (who, len(data), layout.size))
  fields = layout.unpack_from(data)
  if fields[0] != magic:
    raise ValueError('%s: not a %s file (magic %r, expected %r)' % (who, noun, fields[0], magic))
  if fields[1] != version:
    raise ValueError('%s: format version %d, this reader knows %d' % (who, fields[1], version))
  return fields[2:]


def check_raw_body(got, want, who, unit, needs, trailing='trailing bytes'):
  """ValueError unless a raw body of `got` bytes has the `want` bytes that `needs` (the end of the sentence) names."""
  if got < want:
    raise ValueError('%s: truncated, %d %s bytes of the %d %s' % (who, got, unit, want, needs))
  if got > want:
    raise ValueError('%s: %d %s beyond the %d %s' % (who, got - want, trailing, want, needs))


def packed_row(row, nbytes, code_shape, who):
  """`row` as a tensor; ValueError unless it is the one uint8 row of `nbytes` values that holds a packed C x H x W code."""
  row = torch.as_tensor(row)
  if row.dtype != torch.uint8 or row.dim() != 1 or row.numel() != nbytes:
    raise ValueError('%s: a %d x %d x %d code is %d uint8 values in one row, got %s %s'
                     % ((who,) + tuple(code_shape) + (nbytes, row.dtype, tuple(row.shape))))
  return row
