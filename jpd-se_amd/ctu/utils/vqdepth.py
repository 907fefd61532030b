"""The coded file of a residual vector-quantised code whose stage depth differs from cell to cell: stage s holds
the indices of the cells with depth > s only, one .jpdv blob (vqstream.py) per stage, in a container that can be CUT
after any stage as .jpdr can (vqstages.py).  Suffix .jpdm.  The depth map itself is NOT in the file: sender and
receiver derive it from the label map they both hold, and the per-stage cell counts let the reader refuse a map that is not the
sender's before anything is decoded.

  offset  bytes  field (all little-endian)
       0      4  magic b'JPDM'
       4      4  format version, uint32 (1)
       8      4  S          stages, 1 .. 8
      12      4  n          rows of the dense code
      16      4  code_len   indices per row
      20      4  L          n_center of every stage, 2 .. 512
      24    4 S  the S uint32 byte lengths of the stage blobs (0: a stage without a cell, which has no blob)
 24 + 4 S   4 S  the S uint32 counts of cells coded per stage
 24 + 8 S        the blobs in stage order

The dense code is int64 (S, n, code_len) with -1 past a cell's depth; its n * code_len indices per stage are `cells` cells of G =
n * code_len / cells consecutive indices each (one pixel of the feature map holds its G channel groups), cells = the size of the
depth map.  Stage s's blob is what vqstream.write_indices writes for the (count_s, G) code of the cells with min(depth, S) > s in
raster order, in a stream count that is a multiple of G, so a stream still holds one channel group.  truncate_depth_stages rewrites
the header and the two tables and copies the first blobs byte for byte -- no device, no depth map.  coded_bits = 8 * file bytes,
headers included.  Header, tables and every inner blob's own header are checked on the host before any device call; each failure
is a ValueError naming the field.
"""
import struct

import numpy as np
import torch

from jpdse_hip import ops, streams
from . import container, vqstream

MAGIC = b'JPDM'
VERSION = 1
SUFFIX = '.jpdm'
_HEADER = struct.Struct('<4sIIIII')
HEADER_BYTES = _HEADER.size
MAX_STAGES = ops.VQ_RES_MAX_STAGES


def host_depth(depth, who='depth'):
  """The depth map as a flat int64 numpy array (a device tensor is read back once).  ValueError unless it is an integer tensor or
  array with at least one cell."""
  if torch.is_tensor(depth):
    if depth.dtype not in (torch.int32, torch.int64):
      raise ValueError('%s: the depth map is an int32 or int64 tensor, got %s' % (who, depth.dtype))
    depth = depth.detach().cpu().numpy()
  d = np.asarray(depth)
  if d.dtype.kind not in 'iu' or d.size < 1:
    raise ValueError('%s: the depth map is a non-empty integer array, got %s of %d values' % (who, d.dtype, d.size))
  return d.reshape(-1).astype(np.int64)


def depth_map_host(label, table, default, step):
  """int64 numpy [N, H / step, W / step]: ops.vq_depth_map's rule on the host -- the maximum over a cell's step x step pixels of
  table[class], the class of a pixel its label when that is an integer in [0, len(table)), any other pixel taking `default`.
  label: a [N, 1, H, W] tensor or array (a device tensor is read back)."""
  lab = label.detach().cpu().numpy() if torch.is_tensor(label) else np.asarray(label)
  lab = lab.astype(np.float32)
  N, _, H, W = lab.shape
  table = np.asarray(table, dtype=np.int64)
  with np.errstate(invalid='ignore'):
    inside = (lab >= 0) & (lab < np.float32(len(table))) & (lab == np.floor(lab))
  k = np.where(inside, lab, 0).astype(np.int64)
  per_pixel = np.where(inside, table[k] if len(table) else 0, int(default))[:, 0]
  return per_pixel.reshape(N, H // step, step, W // step, step).max(axis=(2, 4)).astype(np.int64)


def stage_counts(depth, stages):
  """[count_0 .. count_{stages - 1}]: the cells with min(depth, stages) > s, depth clamped to 1 .. as the kernels clamp it."""
  d = np.clip(host_depth(depth), 1, int(stages))
  return [int((d > s).sum()) for s in range(int(stages))]


def build_depth_stages(blobs, counts, n, code_len, n_center):
  """The file's bytes from the S stage blobs (bytes each, in stage order; b'' for a stage without a cell) and the S cell counts.
  Host only; the blobs are not inspected here."""
  blobs = [bytes(b) for b in blobs]
  counts = [int(c) for c in counts]
  if not 1 <= len(blobs) <= MAX_STAGES:
    raise ValueError('build_depth_stages: S = %d stages, outside 1 .. %d' % (len(blobs), MAX_STAGES))
  if len(counts) != len(blobs):
    raise ValueError('build_depth_stages: %d counts for %d stages' % (len(counts), len(blobs)))
  for s, (b, c) in enumerate(zip(blobs, counts)):
    if (c == 0) != (len(b) == 0) or c < 0:
      raise ValueError('build_depth_stages: stage %d: count = %d cells with a blob of %d bytes' % (s, c, len(b)))
  S = len(blobs)
  return (_HEADER.pack(MAGIC, VERSION, S, int(n), int(code_len), int(n_center)) + struct.pack('<%dI' % S, *[len(b) for b in blobs]) +
          struct.pack('<%dI' % S, *counts) + b''.join(blobs))


def parse_depth_stages(blob, who='blob', stages=None, depth=None):
  """(S, n, code_len, L, counts, blobs) of a file's bytes; counts and blobs of the first `stages` (default: all S) stages.
  ValueError on a wrong magic, an unknown version, S outside 1 .. 8, an empty shape or L out of range, tables that are truncated,
  a length table that does not add up to the file size, a stage whose count and length disagree about its being empty, counts
  that rise from one stage to the next or exceed n * code_len, `stages` outside 1 .. S; with `depth` (the receiver's map): a map
  whose size does not divide n * code_len, and per-stage counts that are not the counts the map implies; and an inner blob whose
  own header disagrees with (count, G, L) (or fails vqstream.parse_blob; G is known with `depth` only).  Host only."""
  if not isinstance(blob, (bytes, bytearray)):
    raise ValueError('%s: a .jpdm blob is bytes, got %s' % (who, type(blob).__name__))
  S, n, code_len, L = container.header(blob, _HEADER, MAGIC, VERSION, 'coded depth-stage', who)
  if not 1 <= S <= MAX_STAGES:
    raise ValueError('%s: S = %d stages, outside 1 .. %d' % (who, S, MAX_STAGES))
  vqstream._limits(n, code_len, L, who)
  M = n * code_len
  start = HEADER_BYTES + 8 * S
  if len(blob) < start:
    raise ValueError('%s: truncated, %d bytes are shorter than the header and its two tables of %d stages (%d bytes)'
                     % (who, len(blob), S, start))
  lengths = struct.unpack_from('<%dI' % S, blob, HEADER_BYTES)
  counts = struct.unpack_from('<%dI' % S, blob, HEADER_BYTES + 4 * S)
  for s in range(S):
    if (counts[s] == 0) != (lengths[s] == 0):
      raise ValueError('%s: stage %d: count table says %d cells, length table says %d bytes' % (who, s, counts[s], lengths[s]))
    if 0 < lengths[s] < vqstream.HEADER_BYTES:
      raise ValueError('%s: length table: stage %d takes %d bytes, less than a %d-byte .jpdv header' % (who, s, lengths[s], vqstream.HEADER_BYTES))
    if counts[s] > M or (s > 0 and counts[s] > counts[s - 1]):
      raise ValueError('%s: count table: stage %d codes %d cells, more than %s' % (
          who, s, counts[s], 'the %d indices of a stage' % M if counts[s] > M else 'the %d of the stage before' % counts[s - 1]))
  if counts[0] == 0:
    raise ValueError('%s: count table: stage 0 codes no cell (every cell has a depth of at least 1)' % who)
  container.check_raw_body(len(blob) - start, sum(lengths), who, 'stage', 'that the length table of %d stages adds up to' % S)
  take = S if stages is None else int(stages)
  if not 1 <= take <= S:
    raise ValueError('%s: stages = %r, the file holds 1 .. %d' % (who, stages, S))
  G = None
  if depth is not None:
    d = host_depth(depth, who)
    if M % d.size != 0:
      raise ValueError('%s: the depth map has %d cells, which do not divide the %d indices of a stage' % (who, d.size, M))
    G = M // d.size
    want = stage_counts(d, S)
    for s in range(take):
      if counts[s] != want[s]:
        raise ValueError('%s: count table: stage %d codes %d cells, the depth map implies %d (another label map?)'
                         % (who, s, counts[s], want[s]))
  out, at = [], start
  for s in range(take):
    inner = bytes(blob[at:at + lengths[s]])
    at += lengths[s]
    if counts[s] > 0:
      inner_who = '%s: stage %d' % (who, s)
      ni, ci, Li = vqstream.parse_blob(inner, inner_who)[:3]
      checks = [('n', ni, counts[s]), ('n_center', Li, L)] + ([('code_len', ci, G)] if G is not None else [])
      for name, got, need in checks:
        if got != need:
          raise ValueError('%s: its %s = %d, the container says %d' % (inner_who, name, got, need))
    out.append(inner)
  return S, n, code_len, L, list(counts[:take]), out


def _cell_depth(depth, M, S, who):
  """(d int64 numpy [cells] clamped to 1 .. S, G)"""
  d = host_depth(depth, who)
  if M % d.size != 0:
    raise ValueError('%s: the depth map has %d cells, which do not divide the %d indices of a stage' % (who, d.size, M))
  return np.clip(d, 1, S), M // d.size


def write_depth_stages(path, code, depth, n_center, groups=None, n_streams=64):
  """code: the dense int64 (S, n, code_len) device tensor of ResidualS2HVQ.encode(..., depth=, groups=); depth: the integer map of
  n * code_len / groups cells -> the file's bytes, also written to `path` unless that is None.  groups (None: derived from the
  map's size) is checked against it.  Stage s codes the cells with min(depth, S) > s by vqstream.write_indices in the largest
  multiple of `groups` streams within n_streams (at least `groups`).  What the code holds past a cell's depth is not looked at;
  ValueError for an index outside [0, n_center) inside it."""
  if not torch.is_tensor(code) or code.dim() != 3 or code.dtype != torch.int64:
    raise ValueError('write_depth_stages: the code is an int64 (S, n, code_len) tensor')
  S, n, code_len = (int(v) for v in code.shape)
  if not 1 <= S <= MAX_STAGES:
    raise ValueError('write_depth_stages: S = %d stages, outside 1 .. %d' % (S, MAX_STAGES))
  d, G = _cell_depth(depth, n * code_len, S, 'write_depth_stages')
  if groups is not None and int(groups) != G:
    raise ValueError('write_depth_stages: groups = %r, the depth map of %d cells over %d indices gives %d' % (groups, d.size, n * code_len, G))
  cells = code.reshape(S, d.size, G)
  dd = torch.from_numpy(d).to(code.device)
  blobs, counts = [], []
  for s in range(S):
    picked = cells[s][dd > s]                    # (count_s, G), raster order
    counts.append(int(picked.shape[0]))
    if counts[-1] == 0:
      blobs.append(b'')
      continue
    ns = max(G, min(int(n_streams), counts[-1] * G, vqstream.MAX_STREAMS) // G * G)
    blobs.append(vqstream.write_indices(None, picked.contiguous(), n_center, ns))
  blob = build_depth_stages(blobs, counts, n, code_len, n_center)
  if path is not None:
    with open(path, 'wb') as fh:
      fh.write(blob)
  return blob


def read_depth_stages(blob_or_path, depth, device=None, stages=None):
  """The dense int64 (S', n, code_len) code of the first `stages` (default: all) stages of a blob or file write_depth_stages wrote,
  on `device` (default: the current GPU), -1 past a cell's depth.  depth: the receiver's map; every check of parse_depth_stages
  against it is made on the host before the first device call."""
  blob, who = container.load(blob_or_path)
  S, n, code_len, L, counts, blobs = parse_depth_stages(blob, who, stages, depth)
  d, G = _cell_depth(depth, n * code_len, S, who)
  dev = torch.device(streams.default_device(device))
  dd = torch.from_numpy(d).to(dev)
  out = torch.full((len(blobs), d.size, G), -1, dtype=torch.int64, device=dev)
  for s, inner in enumerate(blobs):
    if counts[s] > 0:
      out[s][dd > s] = vqstream.read_indices(inner, dev)
  return out.view(len(blobs), n, code_len)


def truncate_depth_stages(blob_or_path, stages):
  """The bytes of a valid .jpdm file that holds the first `stages` stages: a new header and tables, the stage blobs copied byte
  for byte.  Host only; needs no depth map.  The cut file decodes with min(depth, stages)."""
  blob, who = container.load(blob_or_path)
  S, n, code_len, L, counts, blobs = parse_depth_stages(blob, who, stages)
  return build_depth_stages(blobs, counts, n, code_len, L)


def coded_bits(blob_or_path, stages=None):
  """The rate of a written code: 8 * file bytes, headers included; with `stages`, of the file cut after that many stages."""
  blob, _ = container.load(blob_or_path)
  return 8 * len(blob if stages is None else truncate_depth_stages(blob, stages))


def reconstruct_depth_stages(rvq, blob_or_path, depth, stages=None):
  """(n, d) float32: the first `stages` stages of the file through the module's code books (ops.vq_res_decode with the depth map)
  -- bit for bit rvq.quantize(x, code_len, depth=, groups=)'s y of the x the file was written from."""
  books = rvq.code_books.detach().contiguous()
  code = read_depth_stages(blob_or_path, depth, books.device, stages)
  M = code.shape[1] * code.shape[2]
  d, G = _cell_depth(depth, M, rvq.n_stages, 'reconstruct_depth_stages')
  return rvq.decode(code, depth=torch.from_numpy(d).to(books.device), groups=G)
