"""The host half of the device coders (entropy.hip, semantics.hip, vq_coder.hip: DESIGN.md 4.18; vq_plane.hip: 4.19; the cost walks
of the two index coders, vq_cost.hip: 4.20): the layout of their
buffers, the payload rules (length tables, plane entries, index limits), the staging of payload rows for one upload, what is
refused before the library is touched, and the reading of status words.  `jpdse_hip.ops` re-exports every public name.

The payload rules (check_length_table, length_table_size, check_payload, the SEM_* constants, semantics_check_entry,
vq_index_bits and its limits) run on the host alone: the container modules of ctu.utils take them from here.
"""
import ctypes
import struct

import torch

from . import (lib, check, JpdseError, VqIndexEncodeArgs, VqIndexDecodeArgs, VqPlaneEncodeArgs, VqPlaneDecodeArgs, VqIndexCostArgs,
               VqPlaneCostArgs)


# ---- shared by the three coders ----------------------------------------------------------------------------------------------
def default_device(device=None):
  """`device`, or the current GPU when it is None."""
  return device if device is not None else torch.device('cuda', torch.cuda.current_device())


def _head(words):
  """Bytes of `words` int32 meta words (sizes, status), rounded up so that the rows behind them start 16-byte aligned."""
  return (4 * words + 15) // 16 * 16


def _coder_buffer(words, rows, cap, dev):
  """Encode side: one uint8 device buffer [meta words rounded to 16 | `rows` payload rows of `cap` bytes] -> (the buffer,
  the int32 view of its meta words, the byte offset of the first row)."""
  head = _head(words)
  buf = torch.empty(head + rows * cap, dtype=torch.uint8, device=dev)
  return buf, buf[:4 * words].view(torch.int32), head


def _stage_rows(rows, min_widths, refusal, head=0):
  """Decode side: the payloads of N rows in one uint8 host tensor [head | N rows of `stride` bytes], zero where no payload
  lies, ready for one upload.  rows[n][p]: the bytes of plane p of row n, or None for nothing; plane p sits at offsets[p] of
  its row and is as wide as its longest payload (at least min_widths[p]).  ValueError(refusal % stride) for a stride of 2^31
  or more.  Returns (host, sizes, offsets, stride); sizes[n][p] = the bytes staged (0 for None)."""
  widths = [max([len(row[p]) for row in rows if row[p] is not None] + [w]) for p, w in enumerate(min_widths)]
  offsets = [sum(widths[:p]) for p in range(len(widths))]
  stride = sum(widths)
  if stride >= 1 << 31:
    raise ValueError(refusal % stride)
  raw = bytearray(head + len(rows) * stride)      # zeroed; each payload is copied into it once, the tensor is a view of it
  view = memoryview(raw)                          # (a bytearray's own slice assignment copies the bytes twice)
  for n, row in enumerate(rows):
    for p, payload in enumerate(row):
      if payload is not None:
        at = head + n * stride + offsets[p]
        view[at:at + len(payload)] = payload
  return torch.frombuffer(raw, dtype=torch.uint8), [[len(p) if p is not None else 0 for p in row] for row in rows], offsets, stride


def length_table_size(buf, count, who, at=0):
  """The payload layout of DESIGN.md 4.8 on the host: buf[at:] starts with a table of `count` little-endian uint32 stream
  lengths, then the streams.  Returns the size the table gives the payload, 4 * count + its sum; ValueError when buf ends
  inside the table.  Nothing is copied."""
  if len(buf) - at < 4 * count:
    raise ValueError('%s: truncated, %d bytes are shorter than the table of %d stream lengths' % (who, len(buf) - at, count))
  return 4 * count + sum(struct.unpack_from('<%dI' % count, buf, at))


def check_length_table(payload, count, who):
  """ValueError unless the table of `count` lengths at the start of `payload` adds up to exactly the bytes that follow it."""
  size = length_table_size(payload, count, who)
  if size != len(payload):
    raise ValueError('%s: the length table sums to %d, but %d bytes follow it' % (who, size - 4 * count, len(payload) - 4 * count))


def check_payload(payload, count, who, not_bytes):
  """The one check of a coded payload: it is bytes -- ValueError(not_bytes % the type's name) otherwise -- and its table of
  `count` lengths adds up (check_length_table under the name `who`)."""
  if not isinstance(payload, (bytes, bytearray)):
    raise ValueError(not_bytes % type(payload).__name__)
  check_length_table(payload, count, who)


# ---- learned codec: entropy-coded bitstream (entropy.hip; format: DESIGN.md 4.8) -------------------------------------------
def code_entropy_encode(b):
  """The entropy-coded payload of every image of the code `b` (jpdse_code_entropy_encode): a list of N `bytes`, each the
  image's C little-endian uint32 stream lengths followed by its C streams.  One device buffer -- the N sizes, the N status
  words, then the payload rows -- is copied to the host once.  JpdseError if a stream outgrew its derived capacity."""
  L = lib()
  N, dev = b.N, b.t.device
  cap = L.jpdse_code_entropy_capacity(b.H, b.W, b.C)
  n_ws = L.jpdse_code_entropy_workspace_size(N, b.H, b.W, b.C)
  if cap == 0 or n_ws == 0:
    raise ValueError('code_entropy_encode: a %d x %d x %d x %d code is beyond the coder\'s limits' % (N, b.C, b.H, b.W))
  buf, meta, head = _coder_buffer(2 * N, N, cap, dev)
  ws = workspace(n_ws, dev)
  check(L.jpdse_code_entropy_encode(b.dtype, N, b.H, b.W, b.C, _p(b.t), _p(buf[head:]), cap, _p(meta[:N]), _p(meta[N:]),
                                    _p(ws), ws.numel(), _stream()), 'code_entropy_encode')
  host = buf.cpu().numpy()
  sizes, status = host[:4 * N].view('<i4'), host[4 * N:8 * N].view('<i4')
  if status.any():
    raise JpdseError('code_entropy_encode: a stream outgrew its H*W + 8 bytes (status %s)' % (status.tolist(),))
  return [host[head + n * cap:head + n * cap + int(sizes[n])].tobytes() for n in range(N)]


def code_entropy_decode(payloads, N, H, W, C, dtype_code, device=None):
  """The inverse (jpdse_code_entropy_decode): N payloads as code_entropy_encode returns them -> the NHWC Act [N, H, W, C] of
  +1 / -1 that code_import gives for the raw code.  ValueError before any library call for a wrong payload count, an item
  that is not `bytes`, or a payload whose length table does not add up to the bytes that follow it.  device: where the Act
  is made (default: the current device)."""
  if not isinstance(payloads, (list, tuple)) or len(payloads) != N:
    raise ValueError('code_entropy_decode: expected a list of %d payloads, got %s'
                     % (N, 'a list of %d' % len(payloads) if isinstance(payloads, (list, tuple)) else type(payloads).__name__))
  for n, p in enumerate(payloads):
    check_payload(p, C, 'code_entropy_decode: payload %d' % n, 'code_entropy_decode: payload %d is %%s, not bytes' % n)
  rows, sizes, _, stride = _stage_rows([[p] for p in payloads], [0], 'code_entropy_decode: a payload of %d bytes')
  sizes = (ctypes.c_int32 * N)(*[s[0] for s in sizes])
  dev = default_device(device)
  rows = rows.to(dev)
  b = Act.empty(N, H, W, C, dtype_code, dev)
  check(lib().jpdse_code_entropy_decode(dtype_code, N, H, W, C, _p(rows), stride, sizes, _p(b.t), _stream()),
        'code_entropy_decode')
  return b


# ---- learned codec: coded label and instance maps (semantics.hip; format: DESIGN.md 4.9) -----------------------------------
SEM_RAW, SEM_CODED = 0, 1
SEM_RAW_BYTES = (1, 4)                      # label plane: uint8, instance plane: little-endian int32
_SEM_RAW_DTYPE = (torch.uint8, torch.int32)
_SEM_NAMES = ('label', 'instance')


def semantics_strips(H, strip_rows):
  return (H + strip_rows - 1) // strip_rows


def _sem_maps(label, inst, who):
  if not torch.is_tensor(label) or label.dtype != torch.float32 or label.dim() != 4 or label.shape[1] != 1:
    raise ValueError('%s: the label map is a float32 [N, 1, H, W] tensor' % who)
  if inst is not None and (not torch.is_tensor(inst) or inst.dtype != torch.int64 or tuple(inst.shape) != tuple(label.shape)):
    raise ValueError('%s: the instance map is an int64 tensor of the label map\'s shape %s' % (who, tuple(label.shape)))
  if not label.is_contiguous() or (inst is not None and not inst.is_contiguous()):
    raise ValueError('%s: the maps must be contiguous' % who)
  return int(label.shape[0]), int(label.shape[2]), int(label.shape[3])


def semantics_encode(label, inst, strip_rows=8):
  """The coded planes of every image (jpdse_semantics_encode).  label: device float32 [N, 1, H, W] with integer values in
  [0, 255]; inst: device int64 [N, 1, H, W] with values in [0, 2^31), or None for no instance plane -- the tensors the input
  builder reads.  Returns a list of N items [label entry, instance entry]; an entry is (mode, payload) and None for the
  absent instance plane.  mode 1: payload = the plane's S uint32 stream lengths and its S streams; mode 0: the raw plane
  (uint8, or little-endian int32), taken where a stream outgrew its slot (status bit 0) or coding did not make the plane
  smaller.  ValueError, naming the image, for a value out of range (status bit 1).  The sizes and status words are copied
  to the host first, then each payload by itself: the rows of the device buffer are capacity-sized, the payloads are not."""
  N, H, W = _sem_maps(label, inst, 'semantics_encode')
  strip_rows = int(strip_rows)
  if strip_rows < 1:
    raise ValueError('semantics_encode: strip_rows %d is below 1' % strip_rows)
  L = lib()
  mask = 1 | (2 if inst is not None else 0)
  cap = L.jpdse_semantics_capacity(H, W, strip_rows, mask)
  n_ws = L.jpdse_semantics_workspace_size(N, H, W, strip_rows, mask)
  if cap == 0 or n_ws == 0:
    raise ValueError('semantics_encode: %d maps of %d x %d in strips of %d rows are beyond the coder\'s limits' % (N, H, W, strip_rows))
  dev = label.device
  offs = (0, L.jpdse_semantics_capacity(H, W, strip_rows, 1))
  buf, meta, head = _coder_buffer(4 * N, N, cap, dev)
  meta.zero_()
  ws = workspace(n_ws, dev)
  check(L.jpdse_semantics_encode(N, H, W, strip_rows, mask, _p(label), _p(inst), _p(buf[head:]), cap, _p(meta[:2 * N]),
                                 _p(meta[2 * N:]), _p(ws), ws.numel(), _stream()), 'semantics_encode')
  # the rows are capacity-sized (raw + 12 S bytes per plane): the sizes and status words go to the host first, then only
  # the payloads themselves
  host = meta.cpu().numpy()
  sizes, status = host[:2 * N].reshape(N, 2), host[2 * N:].reshape(N, 2)
  planes = [(0, label)] + ([(1, inst)] if inst is not None else [])
  for n in range(N):
    for p, _ in planes:
      if status[n, p] & 2:
        raise ValueError('semantics_encode: the %s map of image %d holds a value outside the plane\'s range (%s)'
                         % (_SEM_NAMES[p], n, 'integers in [0, 255]' if p == 0 else '[0, 2^31)'))
  out = []
  for n in range(N):
    item = [None, None]
    for p, t in planes:
      raw = H * W * SEM_RAW_BYTES[p]
      size = int(sizes[n, p])
      if (status[n, p] & 1) or size >= raw:
        item[p] = (SEM_RAW, t[n, 0].to(_SEM_RAW_DTYPE[p]).cpu().numpy().astype('u1' if p == 0 else '<i4').tobytes())
      else:
        at = head + n * cap + offs[p]
        item[p] = (SEM_CODED, buf[at:at + size].cpu().numpy().tobytes())
    out.append(item)
  return out


def semantics_check_entry(entry, plane, H, W, strip_rows, who):
  """ValueError unless `entry` is (mode, bytes) holding a raw plane of the right size or a coded payload whose table of
  S = ceil(H / strip_rows) lengths adds up to the bytes after it.  Host only."""
  if not isinstance(entry, (tuple, list)) or len(entry) != 2 or not isinstance(entry[1], (bytes, bytearray)):
    raise ValueError('%s: an entry is (mode, bytes)' % who)
  mode, payload = entry
  if mode not in (SEM_RAW, SEM_CODED):
    raise ValueError('%s: unknown mode %r (0 = raw, 1 = coded)' % (who, mode))
  if mode == SEM_CODED:
    check_length_table(payload, semantics_strips(H, strip_rows), who)
  elif len(payload) != H * W * SEM_RAW_BYTES[plane]:
    raise ValueError('%s: a raw plane (%s) of %d x %d is %d bytes, got %d'
                     % (who, _SEM_NAMES[plane], H, W, H * W * SEM_RAW_BYTES[plane], len(payload)))


def semantics_decode(items, H, W, strip_rows, num_labels, device=None):
  """The inverse (jpdse_semantics_decode): N items as semantics_encode returns them -> (label float32 [N, 1, H, W],
  instance int64 [N, 1, H, W]) on the device, the form the input builder reads; without an instance plane the instance map
  is zeros.  ValueError before any library call for anything that is not such a list (all items with the same planes), a raw
  plane of the wrong size and a length table that does not add up; ValueError after the decode for a label >= num_labels
  or an instance value >= 2^31, naming the image."""
  who = 'semantics_decode'
  if not isinstance(items, (list, tuple)) or len(items) == 0:
    raise ValueError('%s: expected a list of per-image [label entry, instance entry] items' % who)
  N = len(items)
  H, W, strip_rows, num_labels = int(H), int(W), int(strip_rows), int(num_labels)
  if min(H, W, strip_rows) < 1 or not 1 <= num_labels <= 256:
    raise ValueError('%s: bad shape %d x %d, strip_rows %d or num_labels %d' % (who, H, W, strip_rows, num_labels))
  mask = None
  for n, item in enumerate(items):
    if not isinstance(item, (list, tuple)) or len(item) != 2 or item[0] is None:
      raise ValueError('%s: item %d is not [label entry, instance entry or None]' % (who, n))
    m = 1 | (2 if item[1] is not None else 0)
    if mask is not None and m != mask:
      raise ValueError('%s: item %d has other planes than item 0' % (who, n))
    mask = m
    for p in range(2):
      if item[p] is not None:
        semantics_check_entry(item[p], p, H, W, strip_rows, '%s: %s plane of image %d' % (who, _SEM_NAMES[p], n))
  # raw planes are checked on the host, before any device work
  raws = {}
  for n, item in enumerate(items):
    for p in range(2):
      if item[p] is not None and item[p][0] == SEM_RAW:
        a = torch.frombuffer(bytearray(item[p][1]), dtype=_SEM_RAW_DTYPE[p]).view(H, W)
        if p == 0 and int(a.max()) >= num_labels:
          raise ValueError('%s: the label map of image %d holds label %d, the label set has %d' % (who, n, int(a.max()), num_labels))
        if p == 1 and int(a.min()) < 0:
          raise ValueError('%s: the instance map of image %d holds a negative value' % (who, n))
        raws[(n, p)] = a
  dev = default_device(device)
  S = semantics_strips(H, strip_rows)
  label = torch.empty((N, 1, H, W), dtype=torch.float32, device=dev)
  inst = torch.empty((N, 1, H, W), dtype=torch.int64, device=dev) if mask & 2 else torch.zeros((N, 1, H, W), dtype=torch.int64, device=dev)
  if len(raws) < N * (2 if mask == 3 else 1):
    # a row holds the coded planes of an image, each as wide as the plane's longest payload (an empty table at least); the
    # [N, 2] sizes travel in front of the rows, in the same upload
    coded = [[e[1] if e is not None and e[0] == SEM_CODED else None for e in item] for item in items]
    head = _head(2 * N)
    host, sizes, offsets, stride = _stage_rows(coded, [4 * S, 4 * S if mask & 2 else 0], who + ': payloads of %d bytes', head)
    host[:8 * N].view(torch.int32).copy_(torch.tensor(sizes, dtype=torch.int32).view(-1))
    inst_off = offsets[1] if mask == 3 else 0
    buf = host.to(dev)
    bad = torch.empty(N, dtype=torch.int32, device=dev)
    check(lib().jpdse_semantics_decode(N, H, W, strip_rows, mask, num_labels, _p(buf[head:]), stride, inst_off, _p(buf),
                                       _p(label), _p(inst) if mask & 2 else ctypes.c_void_p(0), _p(bad), _stream()), who)
    flags = bad.cpu().tolist()
    for n, f in enumerate(flags):
      if f & 1:
        raise ValueError('%s: the label map of image %d decodes to a label outside the set of %d' % (who, n, num_labels))
      if f & 2:
        raise ValueError('%s: the instance map of image %d decodes to a value of 2^31 or more' % (who, n))
  for (n, p), a in raws.items():
    (inst if p else label)[n, 0].copy_(a.to(dev))
  return label, inst


# ---- soft-to-hard vector quantizer: coded index stream (vq_coder.hip; format: DESIGN.md 4.14) -------------------------------
VQ_INDEX_MAX_S = 65535


def vq_index_bits(L):
  """Binary decisions per symbol of an alphabet of L: max(1, bit_length(L - 1))."""
  return max(1, (int(L) - 1).bit_length())


def _vq_index_shape(who, M, L, S):
  M, L, S = int(M), int(L), int(S)
  if not 2 <= L <= VQ_MAX_L:
    raise ValueError('%s: L = %d, the coder takes 2 .. %d' % (who, L, VQ_MAX_L))
  if M < 1 or not 1 <= S <= min(M, VQ_INDEX_MAX_S):
    raise ValueError('%s: M = %d indices in S = %d streams (M >= 1, 1 <= S <= min(M, %d))' % (who, M, S, VQ_INDEX_MAX_S))
  if vq_index_bits(L) * M + 12 * S >= 1 << 31:
    raise ValueError('%s: M = %d indices of %d bits in %d streams are beyond the coder\'s limits (capacity below 2^31 bytes)'
                     % (who, M, vq_index_bits(L), S))
  return M, L, S


def vq_index_encode(index, L, S):
  """The coded payload of the device int32 [M] indices, all in [0, L), in S interleaved streams (jpdse_vq_index_encode):
  `bytes` holding the S little-endian uint32 stream lengths and the S streams.  One device buffer -- the size, the status
  word, then the payload at its capacity -- is copied to the host once.  ValueError for an index outside [0, L) (status
  bit 1), JpdseError if a stream outgrew its derived capacity (bit 0)."""
  assert index.dim() == 1 and index.is_cuda, (tuple(index.shape), index.device)
  M, L, S = _vq_index_shape('vq_index_encode', index.numel(), L, S)
  dev = index.device
  _vq_index(index, M, dev)
  lb = lib()
  cap, n_ws = lb.jpdse_vq_index_capacity(M, L, S), lb.jpdse_vq_index_workspace_size(M, L, S)
  assert cap == vq_index_bits(L) * M + 12 * S and n_ws > 0, (cap, n_ws)
  buf, meta, head = _coder_buffer(2, 1, cap, dev)
  ws = workspace(n_ws, dev)
  args = VqIndexEncodeArgs(M, L, S, index.data_ptr(), buf[head:].data_ptr(), cap, meta[0:].data_ptr(), meta[1:].data_ptr(),
                           ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
  check(lb.jpdse_vq_index_encode(ctypes.byref(args)), 'vq_index_encode')
  host = buf.cpu().numpy()
  size, status = (int(v) for v in host[:8].view('<i4'))
  if status & 2:
    raise ValueError('vq_index_encode: an index outside [0, %d)' % L)
  if status & 1:
    raise JpdseError('vq_index_encode: a stream outgrew its slot of nb * count + 8 bytes (status %d)' % status)
  return host[head:head + size].tobytes()


def vq_index_decode(payload, M, L, S, device=None):
  """The inverse (jpdse_vq_index_decode): a payload as vq_index_encode returns it -> the int32 [M] indices on `device`
  (default: the current device).  ValueError before any library call for a payload that is not `bytes` or whose table of S
  lengths does not add up to the bytes that follow it; ValueError after the decode when a decoded value was >= L (status
  bit 1: the bytes are not a coded stream of this alphabet)."""
  M, L, S = _vq_index_shape('vq_index_decode', M, L, S)
  check_payload(payload, S, 'vq_index_decode', 'vq_index_decode: the payload is %s, not bytes')
  if len(payload) >= 1 << 31:
    raise ValueError('vq_index_decode: a payload of %d bytes' % len(payload))
  dev = torch.device(default_device(device))
  if dev.type != 'cuda':
    raise JpdseError('vq_index_decode: device %s: the JPD-SE HIP path has no CPU fallback' % (dev,))
  # not through _stage_rows: one payload has no padding to zero, and zeroing its 0.8 MB cost 0.01 ms a call
  src = torch.frombuffer(bytearray(payload), dtype=torch.uint8).to(dev)
  index = torch.empty(M, dtype=torch.int32, device=dev)
  status = torch.zeros(1, dtype=torch.int32, device=dev)
  with torch.cuda.device(dev):
    args = VqIndexDecodeArgs(M, L, S, src.data_ptr(), len(payload), index.data_ptr(), status.data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
    check(lib().jpdse_vq_index_decode(ctypes.byref(args)), 'vq_index_decode')
  if int(status.item()) & 2:
    raise ValueError('vq_index_decode: a decoded value outside [0, %d): not a coded stream of this alphabet' % L)
  return index


# ---- soft-to-hard vector quantizer: coded index planes (vq_plane.hip; format: DESIGN.md 4.19) ---------------------------------
def vq_plane_streams(h, G, strip_rows):
  """S = ceil(h / strip_rows) * G: one stream per strip of every group's plane."""
  return (int(h) + int(strip_rows) - 1) // int(strip_rows) * int(G)


def vq_plane_capacity(h, w, G, L, strip_rows):
  """The most a payload can take: (nb + 2) bytes per symbol and 12 per stream (its table entry and its slot's 8)."""
  return (vq_index_bits(L) + 2) * h * w * G + 12 * vq_plane_streams(h, G, strip_rows)


def vq_plane_shape(who, h, w, G, L, strip_rows):
  """The checked (h, w, G, L, strip_rows, S) of a call or a header; ValueError outside the coder's limits.  Host only."""
  h, w, G, L, strip_rows = int(h), int(w), int(G), int(L), int(strip_rows)
  if not 2 <= L <= VQ_MAX_L:
    raise ValueError('%s: L = %d, the coder takes 2 .. %d' % (who, L, VQ_MAX_L))
  if min(h, w, G) < 1:
    raise ValueError('%s: empty plane shape h = %d, w = %d, G = %d (each at least 1)' % (who, h, w, G))
  if strip_rows < 1:
    raise ValueError('%s: strip_rows %d is below 1' % (who, strip_rows))
  S = vq_plane_streams(h, G, strip_rows)
  if S > VQ_INDEX_MAX_S:
    raise ValueError('%s: %d strips of %d groups are S = %d streams, the coder takes at most %d' % (who, S // G, G, S, VQ_INDEX_MAX_S))
  if vq_plane_capacity(h, w, G, L, strip_rows) >= 1 << 31:
    raise ValueError('%s: %d x %d x %d indices of %d bits are beyond the coder\'s limits (capacity below 2^31 bytes)'
                     % (who, h, w, G, vq_index_bits(L)))
  return h, w, G, L, strip_rows, S


def vq_plane_encode(index, h, w, G, L, strip_rows=8):
  """The context-coded payload of one image's device int32 [h * w * G] indices (pixel by pixel, groups ascending inside a
  pixel), all in [0, L), in ceil(h / strip_rows) * G streams (jpdse_vq_plane_encode): `bytes` holding the little-endian uint32
  stream lengths and the streams.  One device buffer -- the size, the status word, then the payload at its capacity -- is
  copied to the host once.  ValueError for an index outside [0, L) (status bit 1), JpdseError if a stream outgrew its derived
  capacity (bit 0)."""
  assert index.dim() == 1 and index.is_cuda, (tuple(index.shape), index.device)
  h, w, G, L, strip_rows, S = vq_plane_shape('vq_plane_encode', h, w, G, L, strip_rows)
  M, dev = h * w * G, index.device
  _vq_index(index, M, dev)
  lb = lib()
  cap, n_ws = lb.jpdse_vq_plane_capacity(h, w, G, L, strip_rows), lb.jpdse_vq_plane_workspace_size(h, w, G, L, strip_rows)
  assert cap == vq_plane_capacity(h, w, G, L, strip_rows) and n_ws > 0, (cap, n_ws)
  buf, meta, head = _coder_buffer(2, 1, cap, dev)
  ws = workspace(n_ws, dev)
  with torch.cuda.device(dev):
    args = VqPlaneEncodeArgs(h, w, G, L, strip_rows, index.data_ptr(), buf[head:].data_ptr(), cap, meta[0:].data_ptr(),
                             meta[1:].data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    check(lb.jpdse_vq_plane_encode(ctypes.byref(args)), 'vq_plane_encode')
  host = buf.cpu().numpy()
  size, status = (int(v) for v in host[:8].view('<i4'))
  if status & 2:
    raise ValueError('vq_plane_encode: an index outside [0, %d)' % L)
  if status & 1:
    raise JpdseError('vq_plane_encode: a stream outgrew its slot of (nb + 2) * count + 8 bytes (status %d)' % status)
  return host[head:head + size].tobytes()


def vq_plane_decode(payload, h, w, G, L, strip_rows=8, device=None):
  """The inverse (jpdse_vq_plane_decode): a payload as vq_plane_encode returns it -> the int32 [h * w * G] indices on `device`
  (default: the current device).  ValueError before any library call for a payload that is not `bytes` or whose table of S
  lengths does not add up to the bytes that follow it; ValueError after the decode when a decoded value was >= L (status
  bit 1: the bytes are not a coded stream of this alphabet)."""
  h, w, G, L, strip_rows, S = vq_plane_shape('vq_plane_decode', h, w, G, L, strip_rows)
  check_payload(payload, S, 'vq_plane_decode', 'vq_plane_decode: the payload is %s, not bytes')
  if len(payload) >= 1 << 31:
    raise ValueError('vq_plane_decode: a payload of %d bytes' % len(payload))
  dev = torch.device(default_device(device))
  if dev.type != 'cuda':
    raise JpdseError('vq_plane_decode: device %s: the JPD-SE HIP path has no CPU fallback' % (dev,))
  src = torch.frombuffer(bytearray(payload), dtype=torch.uint8).to(dev)
  index = torch.empty(h * w * G, dtype=torch.int32, device=dev)
  status = torch.zeros(1, dtype=torch.int32, device=dev)
  with torch.cuda.device(dev):
    args = VqPlaneDecodeArgs(h, w, G, L, strip_rows, src.data_ptr(), len(payload), index.data_ptr(), status.data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
    check(lib().jpdse_vq_plane_decode(ctypes.byref(args)), 'vq_plane_decode')
  if int(status.item()) & 2:
    raise ValueError('vq_plane_decode: a decoded value outside [0, %d): not a coded stream of this alphabet' % L)
  return index


# ---- soft-to-hard vector quantizer: code-length maps of the two coders (vq_cost.hip; definition: DESIGN.md 4.20) ---------------
VQ_COST_MAX_CLASSES = 256


def _vq_cost_label(who, label, n_classes, dev):
  """(H, W, rows of the class tables) of the label map of a cost call, (0, 0, 0) without one.  Host only."""
  if label is None:
    if n_classes:
      raise ValueError('%s: n_classes without a label map' % who)
    return 0, 0, 0
  n_classes = int(n_classes)
  if not torch.is_tensor(label) or label.dtype != torch.float32 or label.dim() != 4 or tuple(label.shape[:2]) != (1, 1):
    raise ValueError('%s: the label map is a float32 [1, 1, H, W] tensor' % who)
  if not label.is_contiguous() or label.device != dev:
    raise ValueError('%s: the label map must be contiguous and on the device of the indices' % who)
  if not 1 <= n_classes <= VQ_COST_MAX_CLASSES:
    raise ValueError('%s: n_classes %d outside [1, %d]' % (who, n_classes, VQ_COST_MAX_CLASSES))
  return int(label.shape[2]), int(label.shape[3]), n_classes + 1


def _vq_cost_run(call, n_ws, head, index, M, G, S, label, n_classes, want_symbols):
  """The outputs of a cost call and the call itself: `head` holds the arguments in front of H of the call's struct, `label`
  (H, W, rows) as _vq_cost_label gave them and the map."""
  dev = index.device
  (H, W, rows), label = label
  new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
  symbol = new(M, torch.int32) if want_symbols else None
  cell, group, units = new(M // G, torch.int64), new(G, torch.int64), new(S, torch.int64)
  decisions, status = new(S, torch.int32), new(1, torch.int32)
  class_units = new(rows, torch.int64) if rows else None
  class_pixels = new(rows, torch.int64) if rows else None
  ptr = lambda t: t.data_ptr() if t is not None else None
  ws = workspace(n_ws, dev)
  with torch.cuda.device(dev):
    args = head + (H, W, ptr(label), int(n_classes) if rows else 0, ptr(symbol), ptr(cell), ptr(group), ptr(units), ptr(decisions),
                   ptr(status), ptr(class_units), ptr(class_pixels), ws.data_ptr(), ws.numel(),
                   torch.cuda.current_stream().cuda_stream)
    call(args)
  return dict(symbol=symbol, cell=cell, group=group, stream_units=units, stream_decisions=decisions, status=status,
              class_units=class_units, class_pixels=class_pixels)


def vq_index_cost(index, L, n_streams, groups=1, label=None, n_classes=0, hw=None, want_symbols=False):
  """Where the bits of a coded index stream go (jpdse_vq_index_cost): the exact cost the adaptive model of vq_index_encode(index,
  L, n_streams) assigns to every index, in units of 2^-16 bit (ops.CODE_COST_UNIT per bit).  index: the device int32 [M] indices
  of ONE image; symbol m belongs to cell m // groups and group m % groups (groups >= 1 divides M).  Returns a dict of device
  tensors: `cell` int64 [M / groups] (the rate map), `group` int64 [groups], `stream_units` int64 [S], `stream_decisions` int32
  [S] (the binary decisions each stream coded), `status` int32 [1] (bit 1: an index outside [0, L) was met and priced, as the
  coder codes it, as 0), `symbol` int32 [M] (None unless want_symbols) and, with `label` (device fp32 [1, 1, H, W]), `n_classes`
  and `hw` = (h, w), the cell grid (h * w * groups == M, H / h == W / w a power of two), `class_units` and `class_pixels` int64
  [n_classes + 1] by the rule of code_cost; both None without a label.  Integer sums throughout: two calls give identical
  tensors.  ValueError, before the library is touched, for a shape outside the limits of vq_index_encode, a group count that
  does not divide M, and a label map or class count the call does not take."""
  who = 'vq_index_cost'
  assert index.dim() == 1 and index.is_cuda, (tuple(index.shape), index.device)
  M, L, S = _vq_index_shape(who, index.numel(), L, n_streams)
  G = int(groups)
  if G < 1 or M % G:
    raise ValueError('%s: groups = %d does not divide M = %d indices' % (who, G, M))
  _vq_index(index, M, index.device)
  h = w = 0
  if label is not None:
    if hw is None or len(hw) != 2 or int(hw[0]) < 1 or int(hw[1]) < 1 or int(hw[0]) * int(hw[1]) * G != M:
      raise ValueError('%s: a label map needs hw = (h, w) with h * w * groups == M = %d, got %r' % (who, M, hw))
    h, w = int(hw[0]), int(hw[1])
  label = _vq_cost_label(who, label, n_classes, index.device), label
  lb = lib()
  n_ws = lb.jpdse_vq_index_cost_workspace_size(M, L, S, G, 0)
  assert n_ws > 0, (M, L, S, G)
  call = lambda a: check(lb.jpdse_vq_index_cost(ctypes.byref(VqIndexCostArgs(*a))), who)
  return _vq_cost_run(call, n_ws, (M, L, S, G, index.data_ptr(), h, w), index, M, G, S, label, n_classes, want_symbols)


def vq_plane_cost(index, shape, L, strip_rows=8, label=None, n_classes=0, want_symbols=False):
  """The same for the context-coded index planes (jpdse_vq_plane_cost): the cost under the model of vq_plane_encode(index, h, w,
  G, L, strip_rows), `shape` = (h, w, G); index: the device int32 [h * w * G] indices of ONE image.  The dict of vq_index_cost:
  `cell` [h * w], `group` [G], the streams' tensors [ceil(h / strip_rows) * G]; stream_decisions depends on the data (flags
  that matched save the literal).  label: device fp32 [1, 1, H, W], H / h == W / w a power of two."""
  who = 'vq_plane_cost'
  assert index.dim() == 1 and index.is_cuda, (tuple(index.shape), index.device)
  if not isinstance(shape, (tuple, list)) or len(shape) != 3:
    raise ValueError('%s: shape is (h, w, G), got %r' % (who, shape))
  h, w, G, L, strip_rows, S = vq_plane_shape(who, shape[0], shape[1], shape[2], L, strip_rows)
  M = h * w * G
  _vq_index(index, M, index.device)
  label = _vq_cost_label(who, label, n_classes, index.device), label
  lb = lib()
  n_ws = lb.jpdse_vq_plane_cost_workspace_size(h, w, G, L, strip_rows, 0)
  assert n_ws > 0, (h, w, G, L, strip_rows)
  call = lambda a: check(lb.jpdse_vq_plane_cost(ctypes.byref(VqPlaneCostArgs(*a))), who)
  return _vq_cost_run(call, n_ws, (h, w, G, L, strip_rows, index.data_ptr()), index, M, G, S, label, n_classes, want_symbols)


# At the end, as is the re-export at the end of ops: whichever of the two modules is imported first finds, half-way through its
# own import, every name of the other that it asks for.
from .ops import Act, workspace, _p, _stream, _vq_index, VQ_MAX_L  # noqa: E402
