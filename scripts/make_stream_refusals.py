"""Pin what the host half of the coded streams accepts and refuses, and how: writes tests/golden/stream_refusals.json, a list of
[case id, exception type or 'returned', full message or a digest of the result].  No GPU and no library: `lib` raises
AssertionError('library touched') wherever a module binds it, and asking torch for the current device raises
AssertionError('device asked for'), with or without a GPU in the machine.  A call that gets past its host checks ends in one
of those two (given device='cpu', it stages its rows and ends at the library) -- recorded like any other outcome, so a check
that moved behind device work, or in front of another check, shows as a changed row.

Covered: the four containers of ctu.utils (bitstream .jpdc, entropy .jpda, semantics .jpds, vqstream .jpdv: writers, readers,
pack / unpack, build_blob / parse_blob, both modes, masks 1 and 3, raw and coded planes) and the payload rules and pre-library
refusals of the device coders' host half (length_table_size, check_length_table, semantics_check_entry, code_entropy_decode,
semantics_decode, semantics_encode, vq_index_decode, vq_index_encode), each with wrong types, empty input, a header one byte
short, a wrong magic / version / mode / mask, empty and oversized shapes, a body one byte short and one byte long, a length
table with one bit flipped, strip_rows 0, L of 1 and 513, S of 0 and M + 1, M of 0, a raw label at or above num_labels, a
negative raw instance value and items with differing planes.  The good payloads come from the CPU coders of tests/ through
the shared *_cases.py helpers, at the smallest shapes of theirs that give both file modes.

The committed fixture was generated on the last commit before jpdse_hip/streams.py and ctu/utils/container.py came in -- this
script runs on either layout -- and is replayed by tests/test_stream_refusals.py; regenerate it only for a deliberate change of
a message, never to make that test pass.

  python scripts/make_stream_refusals.py [--out tests/golden/stream_refusals.json]
"""
import argparse
import hashlib
import json
import os
import struct
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'jpd-se_amd'), os.path.join(ROOT, 'tests')):
  if p not in sys.path:
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ENT_SHAPE, ENT_KINDS = (3, 64, 16, 33), ('ones', 'half')          # coded smaller than the packed row / not smaller
SEM_SHAPE, SEM_CUT_SHAPE = (3, 19, 33, 8), (2, 16, 33, 8)         # 'rects': coded planes; 'iid19': raw planes
VQ_SHAPE, VQ_PACKED_SHAPE = (3000, 100, 7), (4096, 64, 64)        # 'zeros': coded is smaller; 'uniform': the packed indices are


def digest(value):
  """sha256 of bytes and of a tensor's or array's bytes (with dtype and shape), the repr of a number, through lists."""
  if torch.is_tensor(value):
    value = value.detach().cpu().contiguous().numpy()
  if isinstance(value, np.ndarray):
    return '%s%s:%s' % (value.dtype, list(value.shape), hashlib.sha256(np.ascontiguousarray(value).tobytes()).hexdigest()[:16])
  if isinstance(value, (bytes, bytearray)):
    return 'bytes[%d]:%s' % (len(value), hashlib.sha256(bytes(value)).hexdigest()[:16])
  if isinstance(value, (list, tuple)):
    return '[%s]' % ', '.join(digest(v) for v in value)
  return repr(value)


def flip(data, at=0):
  """`data` with the lowest bit of byte `at` flipped."""
  out = bytearray(data)
  out[at] ^= 1
  return bytes(out)


def patch(data, at, fmt, *values):
  out = bytearray(data)
  struct.pack_into(fmt, out, at, *values)
  return bytes(out)


def _bitstream_cases(tmp):
  from ctu.utils import bitstream
  shape = (3, 1, 9)
  row = torch.arange(4, dtype=torch.uint8)
  good = bitstream._HEADER.pack(b'JPDC', 1, *shape) + bytes(range(4))
  out = []

  def write(cid, packed_row, code_shape):
    def call():
      path = os.path.join(tmp, 'w.jpdc')
      n = bitstream.write_code(path, packed_row, code_shape)
      return n, open(path, 'rb').read()
    out.append(('bitstream.write_code/' + cid, call))

  def read(cid, data):
    def call():
      path = os.path.join(tmp, 'r.jpdc')
      with open(path, 'wb') as fh:
        fh.write(data)
      return bitstream.read_code(path)
    out.append(('bitstream.read_code/' + cid, call))
  write('good', row, shape)
  write('good-list', [0, 1, 2, 3], shape)
  write('row-float', row.float(), shape)
  write('row-rank2', row.view(1, 4), shape)
  write('row-short', row[:3], shape)
  write('row-long', torch.zeros(5, dtype=torch.uint8), shape)
  write('row-empty', torch.zeros(0, dtype=torch.uint8), shape)
  write('shape-zero', row, (0, 1, 9))
  write('shape-oversized', row, (1 << 32, 1, 9))
  write('shape-two', row, (3, 9))
  read('good', good)
  read('empty', b'')
  read('header-short', good[:bitstream.HEADER_BYTES - 1])
  read('header-only', good[:bitstream.HEADER_BYTES])
  read('magic', b'JPDA' + good[4:])
  read('version', patch(good, 4, '<I', 2))
  read('shape-zero', patch(good, 12, '<I', 0))
  read('body-short', good[:-1])
  read('body-long', good + b'\0')
  out.append(('bitstream.read_code/missing-file', lambda: bitstream.read_code(os.path.join(tmp, 'none.jpdc'))))
  return out


def _entropy_cases(tmp):
  import entropy_cases
  from ctu.utils import entropy, bitstream
  from jpdse_hip import ops
  _, C, H, W = ENT_SHAPE
  shape = (C, H, W)
  raw = bitstream.payload_bytes(shape)
  row = torch.arange(raw, dtype=torch.int64).to(torch.uint8)
  small, large = (entropy_cases.reference(ENT_SHAPE, kind)[1][0] for kind in ENT_KINDS)
  assert len(small) < raw <= len(large)
  out = []

  def add(name, cid, fn):
    out.append(('%s/%s' % (name, cid), fn))

  def write(cid, payload, packed_row, code_shape):
    def call():
      path = os.path.join(tmp, 'w.jpda')
      n = entropy.write_coded(path, payload, packed_row, code_shape)
      return n, open(path, 'rb').read()
    add('entropy.write_coded', cid, call)

  def read(cid, data):
    def call():
      path = os.path.join(tmp, 'r.jpda')
      with open(path, 'wb') as fh:
        fh.write(data)
      return entropy.read_coded(path)
    add('entropy.read_coded', cid, call)
  payloads = {'good': small, 'good-bytearray': bytearray(small), 'text': 'text', 'none': None, 'tensor': row, 'empty': b'',
              'table-short': small[:4 * C - 1], 'short': small[:-1], 'long': small + b'\0', 'bit-flipped': flip(small, 4)}
  for cid, p in payloads.items():
    add('entropy.check_payload', cid, lambda p=p: entropy.check_payload(p, C))
    add('code_entropy_decode', cid, lambda p=p: ops.code_entropy_decode([small, p], 2, H, W, C, 0))
  add('entropy.check_payload', 'who', lambda: entropy.check_payload(small[:-1], C, 'a name'))
  add('entropy.check_payload', 'channels-off', lambda: entropy.check_payload(small, C - 1))
  for cid, items in (('not-a-list', small), ('items-none', None), ('count-1', [small]), ('count-3', [small] * 3), ('empty-list', []),
                     ('tuple-good', (small, large))):
    add('code_entropy_decode', cid, lambda items=items: ops.code_entropy_decode(items, 2, H, W, C, 0))
  add('code_entropy_decode', 'good-cpu', lambda: ops.code_entropy_decode([small, large], 2, H, W, C, 0, torch.device('cpu')))
  for n in (0, raw - 1, raw, raw + 1):
    add('entropy.mode_of', str(n), lambda n=n: entropy.mode_of(n, shape))
    add('entropy.file_bytes', str(n), lambda n=n: entropy.file_bytes(n, shape))
  write('good-coded', small, row, shape)
  write('good-raw', large, row, shape)
  write('payload-text', 'text', row, shape)
  write('payload-short', small[:-1], row, shape)
  write('payload-bit-flipped', flip(small), row, shape)
  write('row-float', small, row.float(), shape)
  write('row-rank2', small, row.view(1, -1), shape)
  write('row-short', small, row[:-1], shape)
  write('row-long', large, torch.zeros(raw + 1, dtype=torch.uint8), shape)
  write('shape-zero', small, row, (C, 0, W))
  write('shape-oversized', small, row, (C, H, 1 << 32))
  head = lambda mode: entropy._HEADER.pack(b'JPDA', 1, C, H, W, mode)
  coded, rawfile = head(1) + small, head(0) + bytes(row.numpy())
  read('good-coded', coded)
  read('good-raw', rawfile)
  read('empty', b'')
  read('header-short', coded[:entropy.HEADER_BYTES - 1])
  read('header-only-coded', coded[:entropy.HEADER_BYTES])
  read('header-only-raw', rawfile[:entropy.HEADER_BYTES])
  read('magic', b'JPDC' + coded[4:])
  read('version', patch(coded, 4, '<I', 0))
  read('mode-2', patch(coded, 20, '<I', 2))
  read('shape-zero', patch(rawfile, 8, '<I', 0))
  read('raw-short', rawfile[:-1])
  read('raw-long', rawfile + b'\0')
  read('coded-short', coded[:-1])
  read('coded-long', coded + b'\0')
  read('coded-bit-flipped', flip(coded, entropy.HEADER_BYTES))
  read('coded-table-short', coded[:entropy.HEADER_BYTES + 4 * C - 1])
  return out


def _length_table_cases():
  from jpdse_hip import ops
  table = struct.pack('<3I', 2, 0, 1) + b'abc'
  out = []
  for cid, args in (('good', (table, 3, 'who')), ('good-at', (b'xx' + table, 3, 'who', 2)), ('good-bytearray', (bytearray(table), 3, 'who')),
                    ('count-0', (table, 0, 'who')), ('table-short', (table[:11], 3, 'who')), ('table-short-at', (table, 3, 'who', 4)),
                    ('empty', (b'', 1, 'who')), ('text', ('text', 1, 'who'))):
    out.append(('length_table_size/' + cid, lambda args=args: ops.length_table_size(*args)))
  for cid, args in (('good', (table, 3, 'who')), ('short', (table[:-1], 3, 'who')), ('long', (table + b'\0', 3, 'who')),
                    ('bit-flipped', (flip(table), 3, 'who')), ('table-short', (table[:7], 3, 'who')), ('empty', (b'', 2, 'who')),
                    ('count-0-empty', (b'', 0, 'who')), ('count-0-long', (b'\0', 0, 'who'))):
    out.append(('check_length_table/' + cid, lambda args=args: ops.check_length_table(*args)))
  return out


def _semantics_cases(tmp):
  import semantics_cases
  import semantics_ref as sref
  from ctu.utils import semantics
  from jpdse_hip import ops
  _, H, W, sr = SEM_SHAPE
  label, inst, _, _ = semantics_cases.reference(SEM_SHAPE, 'rects')
  lab, ins = sref.entry(label[0], 0, sr), sref.entry(inst[0], 1, sr)
  lab1, ins1 = sref.entry(label[1], 0, sr), sref.entry(inst[1], 1, sr)
  rlab, rins = (0, sref.raw_plane(label[0], 0)), (0, sref.raw_plane(inst[0], 1))
  assert lab[0] == ins[0] == lab1[0] == ins1[0] == 1
  cut_label, cut_inst, _, _ = semantics_cases.reference(SEM_CUT_SHAPE, 'iid19')
  assert sref.entry(cut_label[0], 0, 8)[0] == 0 and sref.entry(cut_inst[0], 1, 8)[0] == 0
  out = []

  def add(name, cid, fn):
    out.append(('%s/%s' % (name, cid), fn))
  entries = {'good-coded': lab, 'good-raw': rlab, 'good-list': list(lab), 'good-bytearray': (1, bytearray(lab[1])), 'none': None,
             'bytes': lab[1], 'triple': (1, lab[1], 0), 'text-payload': (1, 'text'), 'mode-2': (2, lab[1]), 'mode-text': ('1', lab[1]),
             'coded-short': (1, lab[1][:-1]), 'coded-long': (1, lab[1] + b'\0'), 'coded-bit-flipped': (1, flip(lab[1])),
             'coded-table-short': (1, b'\0' * 11), 'coded-empty': (1, b''), 'raw-short': (0, rlab[1][:-1]),
             'raw-long': (0, rlab[1] + b'\0'), 'raw-empty': (0, b'')}
  for cid, e in entries.items():
    add('semantics_check_entry', cid, lambda e=e: ops.semantics_check_entry(e, 0, H, W, sr, 'who'))
    add('semantics.pack', 'label-' + cid, lambda e=e: semantics.pack(H, W, sr, [e, None]))
    add('semantics_decode', 'label-' + cid, lambda e=e: ops.semantics_decode([[lab, ins], [e, ins1]], H, W, sr, 19))
  add('semantics_check_entry', 'instance-raw', lambda: ops.semantics_check_entry(rins, 1, H, W, sr, 'who'))
  add('semantics_check_entry', 'instance-raw-label-size', lambda: ops.semantics_check_entry(rlab, 1, H, W, sr, 'who'))
  add('semantics_check_entry', 'instance-coded', lambda: ops.semantics_check_entry(ins, 1, H, W, sr, 'who'))
  add('semantics_check_entry', 'other-strips', lambda: ops.semantics_check_entry(lab, 0, H, W, 4, 'who'))
  packs = {'mask3-coded': (H, W, sr, [lab, ins]), 'mask3-raw': (H, W, sr, [rlab, rins]), 'mask3-mixed': (H, W, sr, [lab, rins]),
           'mask3-tuple': (H, W, sr, (rlab, ins)), 'planes-none': (H, W, sr, None), 'planes-one': (H, W, sr, [lab]),
           'planes-no-label': (H, W, sr, [None, ins]), 'planes-bytes': (H, W, sr, lab[1]), 'strip_rows-0': (H, W, 0, [rlab, None]),
           'strip_rows-oversized': (H, W, 1 << 32, [rlab, None]), 'H-0': (0, W, sr, [rlab, None]), 'W-oversized': (H, 1 << 32, sr, [rlab, None]),
           'instance-bit-flipped': (H, W, sr, [lab, (1, flip(ins[1]))]), 'instance-raw-short': (H, W, sr, [lab, (0, rins[1][:-1])]),
           'coded-not-smaller': (1, 1, 8, [(1, struct.pack('<I', 0)), None]),
           'cut-shape-raw': (16, 33, 8, [(0, sref.raw_plane(cut_label[0], 0)), (0, sref.raw_plane(cut_inst[0], 1))])}
  for cid, args in packs.items():
    add('semantics.pack', cid, lambda args=args: semantics.pack(*args))
  blobs = {'mask1-coded': semantics.pack(H, W, sr, [lab, None]), 'mask1-raw': semantics.pack(H, W, sr, [rlab, None]),
           'mask3-coded': semantics.pack(H, W, sr, [lab, ins]), 'mask3-raw': semantics.pack(H, W, sr, [rlab, rins]),
           'mask3-mixed': semantics.pack(H, W, sr, [rlab, ins])}
  HB = semantics.HEADER_BYTES
  for cid, blob in list(blobs.items()):
    blobs[cid + '-short'] = blob[:-1]
    blobs[cid + '-long'] = blob + b'\0'
  c3, r3, c1 = blobs['mask3-coded'], blobs['mask3-raw'], blobs['mask1-coded']
  blobs.update({
      'bytearray': bytearray(c3), 'text': 'text', 'none': None, 'array': np.frombuffer(c3, dtype=np.uint8), 'empty': b'',
      'header-short': c3[:HB - 1], 'header-only-coded': c3[:HB], 'header-only-raw': r3[:HB], 'magic': b'JPDV' + c3[4:],
      'version': patch(c3, 4, '<I', 2), 'H-0': patch(r3, 8, '<I', 0), 'W-0': patch(c3, 12, '<I', 0), 'strip_rows-0': patch(r3, 16, '<I', 0),
      'mask-0': patch(c3, 20, '<I', 0), 'mask-2': patch(c3, 20, '<I', 2), 'mask-4': patch(c3, 20, '<I', 4), 'mode0-2': patch(c3, 24, '<I', 2),
      'mode1-2': patch(c3, 28, '<I', 2), 'mask1-mode1-1': patch(c1, 28, '<I', 1), 'label-bit-flipped': flip(c3, HB),
      'instance-bit-flipped': flip(c3, HB + len(lab[1])), 'label-table-short': c1[:HB + 11], 'instance-table-short': c3[:HB + len(lab[1]) + 11],
      'other-strips': patch(c3, 16, '<I', 4)})
  for cid, blob in blobs.items():
    add('semantics.unpack', cid, lambda blob=blob: semantics.unpack(blob))
  add('semantics.unpack', 'who', lambda: semantics.unpack(c3[:-1], 'a name'))

  def write(cid, blob):
    def call():
      path = os.path.join(tmp, 'w.jpds')
      n = semantics.write(path, blob)
      return n, open(path, 'rb').read()
    add('semantics.write', cid, call)

  def read(cid, data):
    def call():
      path = os.path.join(tmp, 'r.jpds')
      with open(path, 'wb') as fh:
        fh.write(data)
      return semantics.read(path)
    add('semantics.read', cid, call)
  for cid in ('mask1-coded', 'mask3-mixed', 'mask3-raw-short', 'mask3-coded-long', 'text', 'empty', 'header-short', 'magic', 'version',
              'mask-2', 'mode0-2', 'strip_rows-0', 'label-bit-flipped'):
    write(cid, blobs[cid])
    if isinstance(blobs[cid], (bytes, bytearray)):
      read(cid, blobs[cid])
  # the device wrappers: everything up to the first library call
  good = [[lab, ins], [lab1, ins1]]
  decodes = {'none': None, 'empty': [], 'item-not-a-list': [lab, ins], 'item-one-entry': [good[0], [lab]], 'item-no-label': [good[0], [None, ins]],
             'other-planes': [good[0], [lab1, None]], 'other-planes-first': [[lab, None], good[1]], 'instance-mode-3': [[lab, (3, ins[1])]],
             'instance-bit-flipped': [[lab, (1, flip(ins[1]))]], 'instance-raw-short': [[lab, (0, rins[1][:-1])]],
             'instance-raw-label-size': [[lab, rlab]], 'good-coded': good, 'good-mask1': [[lab, None], [lab1, None]], 'good-tuple': tuple(good),
             'good-all-raw': [[rlab, rins]], 'good-all-raw-mask1': [[rlab, None]], 'good-mixed': [[rlab, ins], [lab1, rins]]}
  for cid, items in decodes.items():
    add('semantics_decode', cid, lambda items=items: ops.semantics_decode(items, H, W, sr, 19))
  for cid, args in (('H-0', (good, 0, W, sr, 19)), ('W-0', (good, H, 0, sr, 19)), ('strip_rows-0', (good, H, W, 0, 19)),
                    ('num_labels-0', (good, H, W, sr, 0)), ('num_labels-257', (good, H, W, sr, 257)), ('num_labels-256', (good, H, W, sr, 256)),
                    ('good-cpu', (good, H, W, sr, 19, 'cpu')), ('good-mask1-cpu', (decodes['good-mask1'], H, W, sr, 19, 'cpu')),
                    ('good-mixed-cpu', (decodes['good-mixed'], H, W, sr, 19, 'cpu')), ('good-all-raw-cpu', (decodes['good-all-raw'], H, W, sr, 19, 'cpu')),
                    ('good-all-raw-mask1-cpu', (decodes['good-all-raw-mask1'], H, W, sr, 19, torch.device('cpu')))):
    add('semantics_decode', cid, lambda args=args: ops.semantics_decode(*args))
  top = int(label[0].max())
  add('semantics_decode', 'raw-label-at-num_labels', lambda: ops.semantics_decode([[rlab, ins]], H, W, sr, top))
  add('semantics_decode', 'raw-label-below-num_labels', lambda: ops.semantics_decode([[rlab, ins]], H, W, sr, top + 1))
  add('semantics_decode', 'raw-label-200', lambda: ops.semantics_decode([[lab, ins], [(0, bytes([200]) * (H * W)), ins1]], H, W, sr, 19))
  add('semantics_decode', 'raw-instance-negative',
      lambda: ops.semantics_decode([[lab, (0, struct.pack('<i', -1) * (H * W))]], H, W, sr, 19))
  z = torch.zeros(1, 1, 4, 4)
  zi = torch.zeros(1, 1, 4, 4, dtype=torch.int64)
  for cid, args in (('label-float64', (z.double(), None)), ('label-rank3', (z[0], None)), ('label-two-channels', (torch.zeros(1, 2, 4, 4), None)),
                    ('label-list', ([[[[0.0]]]], None)), ('label-strided', (torch.zeros(1, 1, 4, 8)[..., ::2], None)),
                    ('instance-int32', (z, zi.int())), ('instance-other-shape', (z, torch.zeros(1, 1, 4, 5, dtype=torch.int64))),
                    ('instance-list', (z, [0])), ('instance-strided', (z, torch.zeros(1, 1, 4, 8, dtype=torch.int64)[..., ::2])),
                    ('strip_rows-0', (z, None, 0)), ('strip_rows-negative', (z, zi, -8)), ('good', (z, zi)), ('good-no-instance', (z, None, 4))):
    add('semantics_encode', cid, lambda args=args: ops.semantics_encode(*args))
  return out


def _vq_cases(tmp):
  import vq_coder_cases
  from ctu.utils import vqstream
  from jpdse_hip import ops
  M, L, S = VQ_SHAPE
  n, code_len = 30, 100
  nb = vqstream.index_bits(L)
  zeros, small, _ = vq_coder_cases.reference(VQ_SHAPE, 'zeros')
  values, large, _ = vq_coder_cases.reference(VQ_PACKED_SHAPE, 'uniform')
  assert len(small) < vqstream.packed_bytes(M, L) and vqstream.packed_bytes(*VQ_PACKED_SHAPE[:2]) <= len(large)
  out = []

  def add(name, cid, fn):
    out.append(('%s/%s' % (name, cid), fn))
  for cid, args in (('good', ([0, 1, 5, 99, 127], 7)), ('good-one-bit', ([1, 0, 1], 1)), ('good-nine-bits', (np.arange(500, 512), 9)),
                    ('empty', ([], 7)), ('rank2', (np.arange(6).reshape(2, 3), 3)), ('value-at-limit', ([0, 128], 7)),
                    ('value-negative', ([0, -1], 7)), ('text', ('text', 7)), ('none', (None, 7))):
    add('vqstream.pack_indices', cid, lambda args=args: vqstream.pack_indices(*args))
  packed = vqstream.pack_indices([0, 1, 5, 99, 127], 7)
  for cid, args in (('good', (packed, 5, 7)), ('good-bytearray', (bytearray(packed), 5, 7)), ('empty-good', (b'', 0, 7)), ('short', (packed[:-1], 5, 7)),
                    ('long', (packed + b'\0', 5, 7)), ('empty', (b'', 5, 7)), ('padding-set', (patch(packed, 4, 'B', packed[4] | 0x80), 5, 7)),
                    ('M-4', (packed, 4, 7)), ('none', (None, 5, 7))):
    add('vqstream.unpack_indices', cid, lambda args=args: vqstream.unpack_indices(*args))
  builds = {'good-coded': ((n, code_len), L, S, small, zeros), 'good-packed': ((64, 64), 64, 64, large, values),
            'good-bytearray': ((n, code_len), L, S, bytearray(small), zeros.reshape(n, code_len)),
            'shape-zero': ((0, code_len), L, S, small, zeros), 'shape-three': ((n, code_len, 1), L, S, small, zeros),
            'L-1': ((n, code_len), 1, S, small, zeros), 'L-513': ((n, code_len), 513, S, small, zeros),
            'oversized': ((1 << 14, 1 << 14), 512, S, small, zeros), 'S-0': ((n, code_len), L, 0, small, zeros),
            'S-above-M': ((1, 4), L, 5, small, zeros[:4]), 'S-above-65535': ((1 << 10, 1 << 10), L, 65536, small, zeros),
            'payload-text': ((n, code_len), L, S, 'text', zeros), 'payload-none': ((n, code_len), L, S, None, zeros),
            'payload-empty': ((n, code_len), L, S, b'', zeros), 'payload-short': ((n, code_len), L, S, small[:-1], zeros),
            'payload-long': ((n, code_len), L, S, small + b'\0', zeros), 'payload-bit-flipped': ((n, code_len), L, S, flip(small), zeros),
            'payload-other-S': ((n, code_len), L, S + 1, small, zeros), 'indices-short': ((n, code_len), L, S, small, zeros[:-1]),
            'indices-long': ((n, code_len), L, S, small, np.zeros(M + 1)), 'index-negative': ((n, code_len), L, S, small, np.where(np.arange(M) == 3, -1, 0)),
            'index-at-L': ((n, code_len), L, S, small, np.where(np.arange(M) == M - 1, L, 0))}
  for cid, args in builds.items():
    add('vqstream.build_blob', cid, lambda args=args: vqstream.build_blob(*args))
  coded = vqstream.build_blob((n, code_len), L, S, small, zeros)
  pack0 = vqstream.build_blob((64, 64), 64, 64, large, values)
  HB = vqstream.HEADER_BYTES
  blobs = {'good-coded': coded, 'good-packed': pack0, 'good-bytearray': bytearray(coded), 'text': 'text', 'none': None,
           'array': np.frombuffer(coded, dtype=np.uint8), 'empty': b'', 'header-short': coded[:HB - 1], 'header-only-coded': coded[:HB],
           'header-only-packed': pack0[:HB], 'magic': b'JPDS' + coded[4:], 'version': patch(coded, 4, '<I', 3), 'mode-2': patch(coded, 24, '<I', 2),
           'n-0': patch(coded, 8, '<I', 0), 'code_len-0': patch(pack0, 12, '<I', 0), 'L-1': patch(coded, 16, '<I', 1), 'L-513': patch(pack0, 16, '<I', 513), 'packed-L-1': patch(pack0, 16, '<I', 1),
           'oversized': patch(pack0, 8, '<II', 1 << 16, 1 << 16), 'coded-S-0': patch(coded, 20, '<I', 0), 'coded-S-above-M': patch(coded, 20, '<I', M + 1),
           'coded-S-above-65535': patch(patch(coded, 8, '<II', 1 << 10, 1 << 10), 20, '<I', 65536), 'packed-S-7': patch(pack0, 20, '<I', 7),
           'coded-short': coded[:-1], 'coded-long': coded + b'\0', 'coded-bit-flipped': flip(coded, HB), 'coded-table-short': coded[:HB + 4 * S - 1],
           'packed-short': pack0[:-1], 'packed-long': pack0 + b'\0', 'packed-value-at-L': patch(pack0, 16, '<I', 63),
           'packed-other-L': patch(pack0, 16, '<I', 128)}
  for cid, blob in blobs.items():
    add('vqstream.parse_blob', cid, lambda blob=blob: vqstream.parse_blob(blob))
  add('vqstream.parse_blob', 'who', lambda: vqstream.parse_blob(coded[:-1], 'a name'))

  def read(cid, data):
    def call():
      path = os.path.join(tmp, 'r.jpdv')
      with open(path, 'wb') as fh:
        fh.write(data)
      return vqstream.read_indices(path)
    add('vqstream.read_indices', cid, call)
  read('file-header-short', coded[:HB - 1])
  read('file-magic', b'XXXX' + coded[4:])
  read('file-packed-long', pack0 + b'\0')
  read('file-good-coded', coded)
  add('vqstream.read_indices', 'blob-coded-short', lambda: vqstream.read_indices(coded[:-1]))
  add('vqstream.read_indices', 'blob-good-packed-cpu', lambda: vqstream.read_indices(pack0, 'cpu'))
  add('vqstream.read_indices', 'blob-good-coded-cpu', lambda: vqstream.read_indices(bytearray(coded), 'cpu'))
  add('vqstream.read_indices', 'missing-file', lambda: vqstream.read_indices(os.path.join(tmp, 'none.jpdv')))
  code = torch.from_numpy(zeros.astype(np.int64)).view(n, code_len)
  far = code.clone()
  far[0, 0] = -1 - (1 << 32)
  at_l = code.clone()
  at_l[n - 1, 0] = L
  for cid, args in (('list', ([[0, 1]], L)), ('none', (None, L)), ('int32', (code.int(), L)), ('rank1', (code.view(-1), L)), ('rank3', (code.view(n, code_len, 1), L)),
                    ('empty-rows', (code[:0], L)), ('empty-columns', (code[:, :0], L)), ('L-1', (code, 1)), ('L-513', (code, 513)),
                    ('index-at-L', (at_l, L)), ('index-negative', (far, L)), ('good-cpu', (code, L)), ('good-cpu-S-0', (code, L, 0))):
    add('vqstream.write_indices', cid, lambda args=args: vqstream.write_indices(None, *args))
  for cid, args in (('good', (small, M, L, S)), ('good-bytearray', (bytearray(small), M, L, S)), ('good-cpu', (small, M, L, S, 'cpu')),
                    ('L-1', (small, M, 1, S)), ('L-513', (small, M, 513, S)), ('M-0', (small, 0, L, S)), ('S-0', (small, M, L, 0)),
                    ('S-above-M', (small, 4, L, 5)), ('S-above-65535', (small, 1 << 20, L, 65536)), ('oversized', (small, 1 << 28, 512, S)),
                    ('text', ('text', M, L, S)), ('none', (None, M, L, S)), ('tensor', (torch.zeros(4, dtype=torch.uint8), M, L, S)),
                    ('empty', (b'', M, L, S)), ('short', (small[:-1], M, L, S)), ('long', (small + b'\0', M, L, S)),
                    ('bit-flipped', (flip(small), M, L, S)), ('table-short', (small[:4 * S - 1], M, L, S)), ('other-S', (small, M, L, S - 1))):
    add('vq_index_decode', cid, lambda args=args: ops.vq_index_decode(*args))
  flat = torch.zeros(8, dtype=torch.int32)
  for cid, args in (('cpu-tensor', (flat, L, 2)), ('rank2', (flat.view(2, 4), L, 2))):
    add('vq_index_encode', cid, lambda args=args: ops.vq_index_encode(*args))
  for v in (1, 2, 3, 100, 256, 257, 512):
    add('vq_index_bits', str(v), lambda v=v: ops.vq_index_bits(v))
  return out


def _patched_modules():
  """Every module that may bind `lib` at import time."""
  import importlib
  import jpdse_hip
  import jpdse_hip.ops  # noqa: F401
  mods = [jpdse_hip, jpdse_hip.ops]
  try:
    mods.append(importlib.import_module('jpdse_hip.streams'))
  except ImportError:      # the layout before jpdse_hip/streams.py
    pass
  return mods


def run():
  """[[case id, 'returned' or the exception type, digest or message]] on the code this file sits beside."""
  mods = _patched_modules()
  saved = [torch.cuda.is_available, torch.cuda.current_device] + [m.lib for m in mods]
  touched = lambda: (_ for _ in ()).throw(AssertionError('library touched'))
  torch.cuda.is_available = lambda: False
  torch.cuda.current_device = lambda: (_ for _ in ()).throw(AssertionError('device asked for'))
  for m in mods:
    m.lib = touched
  rows = []
  try:
    with tempfile.TemporaryDirectory() as tmp:
      cases = _bitstream_cases(tmp) + _entropy_cases(tmp) + _length_table_cases() + _semantics_cases(tmp) + _vq_cases(tmp)
      for cid, call in cases:
        try:
          rows.append([cid, 'returned', digest(call())])
        except Exception as e:      # every outcome is a row
          rows.append([cid, type(e).__name__, str(e).replace(tmp, '<tmp>')])
  finally:
    torch.cuda.is_available, torch.cuda.current_device = saved[:2]
    for m, lib in zip(mods, saved[2:]):
      m.lib = lib
  return rows


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'stream_refusals.json'))
  args = ap.parse_args()
  rows = run()
  with open(args.out, 'w') as f:
    json.dump(rows, f, indent=0)
    f.write('\n')
  kinds = {}
  for _, kind, _ in rows:
    kinds[kind] = kinds.get(kind, 0) + 1
  print('%d cases -> %s (%s)' % (len(rows), args.out, ', '.join('%s: %d' % kv for kv in sorted(kinds.items()))))


if __name__ == '__main__':
  main()
