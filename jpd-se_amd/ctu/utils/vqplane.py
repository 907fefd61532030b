"""The context-coded file of ONE image's vector-quantised code: the index planes of the S2HVQ bottleneck as bytes (extension;
the format of the coded payload: DESIGN.md 4.19).  Suffix .jpdw.

  offset  bytes  field (all little-endian)
       0      4  magic b'JPDW'
       4      4  format version, uint32 (1)
       8      4  h           rows of the feature map
      12      4  w           columns; the code holds M = h * w * G indices, pixel by pixel, groups ascending inside a pixel
      16      4  G           channel groups per pixel
      20      4  L           n_center, 2 .. 512
      24      4  strip_rows  rows per strip, at least 1; S = ceil(h / strip_rows) * G streams, at most 65535
      28      4  mode, uint32: 1 = coded payload
      32         S uint32 stream lengths, then the S range-coded streams (what ops.vq_plane_encode returns)

There is no packed mode: a writer that does not gain by this coder stores the .jpdv file of ctu.utils.vqstream instead (the
model's codec does).  The file size is the rate of the code: coded_bits = 8 * file bytes, header included.  The
header and the refusals run on the host; the coder itself is the device library's.
"""
import struct

import torch

from jpdse_hip import ops, streams
from . import container

MAGIC = b'JPDW'
VERSION = 1
SUFFIX = '.jpdw'
MODE_CODED = 1
DEFAULT_STRIP_ROWS = 8
_HEADER = struct.Struct('<4sIIIIIII')
HEADER_BYTES = _HEADER.size


def build_blob(shape, n_center, strip_rows, payload):
  """The file's bytes for a code of `shape` = (h, w, G): `payload` is ops.vq_plane_encode of its flat indices in strips of
  strip_rows rows.  Host only."""
  h, w, G = (int(v) for v in shape)
  h, w, G, L, strip_rows, S = streams.vq_plane_shape('build_blob', h, w, G, n_center, strip_rows)
  streams.check_payload(payload, S, 'build_blob', 'build_blob: a coded payload is bytes, got %s')
  return _HEADER.pack(MAGIC, VERSION, h, w, G, L, strip_rows, MODE_CODED) + bytes(payload)


def parse_blob(blob, who='blob'):
  """(h, w, G, L, strip_rows, payload) of a file's bytes.  ValueError on a wrong magic, an unknown version or mode, a field out
  of range, an empty shape, truncated data, trailing bytes and a length table that does not add up.  Host only."""
  if not isinstance(blob, (bytes, bytearray)):
    raise ValueError('%s: a .jpdw blob is bytes, got %s' % (who, type(blob).__name__))
  h, w, G, L, strip_rows, mode = container.header(blob, _HEADER, MAGIC, VERSION, 'coded index plane', who,
                                                  short='%s: truncated, %d bytes are shorter than the %d-byte header')
  if mode != MODE_CODED:
    raise ValueError('%s: unknown mode %d (1 = coded)' % (who, mode))
  h, w, G, L, strip_rows, S = streams.vq_plane_shape(who, h, w, G, L, strip_rows)
  body = bytes(blob[HEADER_BYTES:])
  streams.check_length_table(body, S, who)       # the file has no size of its own: truncation and trailing bytes show here
  return h, w, G, L, strip_rows, body


def write_planes(path, code, shape, n_center, strip_rows=DEFAULT_STRIP_ROWS):
  """code: the int64 device tensor of ONE image's h * w * G indices (any shape; the order of Encoder.vq_code), `shape` =
  (h, w, G) -> the file's bytes, also written to `path` unless that is None.  ValueError for an index outside [0, n_center)."""
  if not torch.is_tensor(code) or code.dtype != torch.int64:
    raise ValueError('write_planes: the code is an int64 tensor of h * w * G indices')
  h, w, G = (int(v) for v in shape)
  h, w, G, L, strip_rows, _ = streams.vq_plane_shape('write_planes', h, w, G, n_center, strip_rows)
  flat = code.contiguous().view(-1)
  if flat.numel() != h * w * G:
    raise ValueError('write_planes: %d indices for planes of %d x %d x %d' % (flat.numel(), h, w, G))
  if bool(((flat < 0) | (flat >= L)).any()):      # before the cast to the coder's int32 could fold a far value into range
    raise ValueError('write_planes: an index outside [0, %d)' % L)
  blob = build_blob((h, w, G), L, strip_rows, ops.vq_plane_encode(flat.to(torch.int32), h, w, G, L, strip_rows))
  if path is not None:
    with open(path, 'wb') as fh:
      fh.write(blob)
  return blob


def read_planes(blob_or_path, device=None):
  """(code, (h, w, G), L): the int64 [h * w * G] code of a blob or file write_planes wrote, on `device` (default: the current
  GPU).  Every refusal of parse_blob is raised on the host before any device call."""
  blob, who = container.load(blob_or_path)
  h, w, G, L, strip_rows, body = parse_blob(blob, who)
  dev = torch.device(streams.default_device(device))
  return ops.vq_plane_decode(body, h, w, G, L, strip_rows, dev).to(torch.int64), (h, w, G), L


def coded_bits(blob):
  """The rate of a written code: 8 * file bytes, header included."""
  return 8 * len(blob)
