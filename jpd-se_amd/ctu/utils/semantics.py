"""The coded file of one image's label and instance maps (extension; the reference hands its receiver the semantics for
free; the format of a coded plane: DESIGN.md 4.9): ONE image per file, suffix .jpds.

  offset  bytes  field (all little-endian)
       0      4  magic b'JPDS'
       4      4  format version, uint32 (1)
       8      4  H   map height
      12      4  W   map width
      16      4  strip_rows, uint32 >= 1: a plane is coded in S = ceil(H / strip_rows) independent strips
      20      4  plane mask, uint32: bit 0 the label plane, bit 1 the instance plane (1 or 3; --no_instance runs write 1)
      24      4  mode of the label plane, uint32: 1 = coded, 0 = raw
      28      4  mode of the instance plane (0 when the plane is absent)
      32         the planes the mask names, label first.  mode 1: S uint32 stream lengths, then the S range-coded streams in
                 strip order (its size is 4 S + the sum of the table); mode 0: H*W uint8 (label) or H*W int32 (instance)

A plane is stored raw whenever a stream of it was cut or coding did not make it smaller (jpdse_hip.ops.semantics_encode
decides; `pack` refuses a coded plane that is not smaller than the raw one), so a .jpds file is never larger than the file
that stores the same planes raw.  The file size is the rate of the semantics: 8 * len(blob) bits.  Everything here runs on
the host; nothing touches the device library.  The rules of a plane entry (modes, raw sizes, strip count, the length table)
are those of jpdse_hip.streams, which produces and consumes the entries: semantics_check_entry is the one check of both.
"""
import struct

from jpdse_hip.streams import (SEM_RAW as MODE_RAW, SEM_CODED as MODE_CODED, SEM_RAW_BYTES as RAW_BYTES, semantics_strips as strips,
                               semantics_check_entry, length_table_size)
from . import container

MAGIC = b'JPDS'
VERSION = 1
SUFFIX = '.jpds'
PLANES = ('label', 'instance')
_HEADER = struct.Struct('<4sIIIIIII')
HEADER_BYTES = _HEADER.size


def raw_plane_bytes(plane, H, W):
  return H * W * RAW_BYTES[plane]


def raw_file_bytes(H, W, mask):
  """Size of the file that stores the planes of `mask` raw."""
  return HEADER_BYTES + sum(raw_plane_bytes(p, H, W) for p in range(2) if mask >> p & 1)


def _geometry(H, W, strip_rows, who):
  H, W, strip_rows = int(H), int(W), int(strip_rows)
  if min(H, W) < 1 or max(H, W, strip_rows) >= 1 << 32:
    raise ValueError('%s: empty or oversized map shape (%d, %d)' % (who, H, W))
  if strip_rows < 1:
    raise ValueError('%s: strip_rows %d is below 1' % (who, strip_rows))
  return H, W, strip_rows


def pack(H, W, strip_rows, planes):
  """The body of a .jpds file.  planes: [label entry, instance entry or None], an entry being (mode, bytes) as
  ops.semantics_encode returns it."""
  H, W, strip_rows = _geometry(H, W, strip_rows, 'pack')
  if not isinstance(planes, (list, tuple)) or len(planes) != 2 or planes[0] is None:
    raise ValueError('pack: planes is [label entry, instance entry or None]')
  mask, modes, body = 0, [0, 0], []
  for p, entry in enumerate(planes):
    if entry is None:
      continue
    who = 'pack: %s plane' % PLANES[p]
    semantics_check_entry(entry, p, H, W, strip_rows, who)
    mode, payload = entry
    raw = raw_plane_bytes(p, H, W)
    if mode == MODE_CODED and len(payload) >= raw:
      raise ValueError('%s: a coded payload of %d bytes is not smaller than the raw plane (%d): store it raw'
                       % (who, len(payload), raw))
    mask |= 1 << p
    modes[p] = mode
    body.append(bytes(payload))
  return _HEADER.pack(MAGIC, VERSION, H, W, strip_rows, mask, modes[0], modes[1]) + b''.join(body)


def unpack(blob, who='semantics blob'):
  """(H, W, strip_rows, mask, [label entry, instance entry or None]) of what `pack` made.  ValueError on a wrong magic, an
  unknown version, mode or mask, an empty shape, truncated data, trailing bytes and a length table that does not add up."""
  if not isinstance(blob, (bytes, bytearray)):
    raise ValueError('%s: the body of a %s file is bytes, got %s' % (who, SUFFIX, type(blob).__name__))
  H, W, strip_rows, mask, mode0, mode1 = container.header(blob, _HEADER, MAGIC, VERSION, 'coded semantics', who)
  if mask not in (1, 3):
    raise ValueError('%s: unknown plane mask %d (1 = label, 3 = label and instance)' % (who, mask))
  modes = (mode0, mode1)
  if mode0 not in (MODE_RAW, MODE_CODED) or mode1 not in (MODE_RAW, MODE_CODED) or (mask == 1 and mode1 != MODE_RAW):
    raise ValueError('%s: unknown mode %d / %d (0 = raw, 1 = coded; 0 for an absent plane)' % (who, mode0, mode1))
  if min(H, W) < 1:
    raise ValueError('%s: empty map shape (%d, %d)' % (who, H, W))
  if strip_rows < 1:
    raise ValueError('%s: strip_rows %d is below 1' % (who, strip_rows))
  S = strips(H, strip_rows)
  at, planes = HEADER_BYTES, [None, None]
  for p in range(2):
    if not mask >> p & 1:
      continue
    name = '%s: %s plane' % (who, PLANES[p])
    # a coded plane is self-delimiting; whether the blob holds all of it shows below, as for a raw one
    size = raw_plane_bytes(p, H, W) if modes[p] == MODE_RAW else length_table_size(blob, S, name, at)
    if len(blob) - at < size:
      raise ValueError('%s: truncated, %d bytes of the %d the plane needs (%s)'
                       % (name, len(blob) - at, size, 'raw' if modes[p] == MODE_RAW else 'its length table sums to %d' % (size - 4 * S)))
    planes[p] = (modes[p], bytes(blob[at:at + size]))
    at += size
  if at != len(blob):
    raise ValueError('%s: %d trailing bytes' % (who, len(blob) - at))
  return H, W, strip_rows, mask, planes


def write(path, blob):
  """Store what trainer.get_coded_semantics returned for one image (checked with `unpack` first).  Returns the bytes written."""
  unpack(blob, 'write')
  with open(path, 'wb') as fh:
    fh.write(blob)
  return len(blob)


def read(path):
  """The blob of a file `write` wrote, checked: ValueError as `unpack` raises it, on the host, before any device call."""
  blob = container.read_file(path)
  unpack(blob, path)
  return blob
