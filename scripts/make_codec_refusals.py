"""Pin what the model's codec calls refuse, and how: writes tests/golden/codec_refusals.json, a list of [case id, exception
type, full message].  No GPU: the models are bare ones around a host-built encoder (the tiny configuration of the codec tests:
nef 8, n_downsample_E 2, 16 bottleneck channels, 8 centres of size 4), and everything that would touch the device raises
AssertionError('device work before the refusal') -- recorded like any other outcome, so a check that moved behind device work,
or in front of another check, shows as a changed row.

For no bottleneck, the binarizer and S2HVQ: every public code / decode / file call on a good batch and on a 64 x 30 label map
(no multiple of the down-sampling factor 4); decode and get_eval_metrics_decoded with codes of a wrong type, dtype, rank and
shape; decode_coded with a wrong payload count, a non-list, a non-bytes item, a truncated payload, and .jpdv blobs of another
n_center or index count.  An index outside the code book is refused on the device: scripts/dump_codec_surface.py records it.

The committed fixture was generated on the last commit before the codec objects (ctu.models.codec) came in -- this script
runs on either layout of the model -- and is replayed by tests/test_codec_refusals.py; regenerate it only for a deliberate
change of a message, never to make that test pass.

  python scripts/make_codec_refusals.py [--out tests/golden/codec_refusals.json]
"""
import argparse
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'jpd-se_amd')):
  if p not in sys.path:
    sys.path.insert(0, p)

import torch  # noqa: E402

N, H, W = 2, 64, 32
C, L, D, DOWN = 16, 8, 4, 2
BITS = C * (H >> DOWN) * (W >> DOWN)             # 2048 per image
CODE_LEN = (H >> DOWN) * (W >> DOWN) * (C // D)  # 512 indices per image


def _boom(*a, **k):
  raise AssertionError('device work before the refusal')


def bare_model(quantizer):
  """A Pix2PixHDModel that never ran its constructor, around a host-built encoder (quantizer None: no bottleneck)."""
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  from ctu.models.pix2pixHD_networks.networks import Encoder
  from jpdse_hip import F32
  m = Pix2PixHDModel.__new__(Pix2PixHDModel)
  torch.nn.Module.__init__(m)
  m.netE = Encoder(3, 3, ngf=8, n_downsampling=DOWN, binarize=quantizer is not None, binarizer_out_channels=C,
                   quantizer=quantizer or 'binarizer', vq_n_center=L, vq_center_size=D)
  m.cdtype, m.zero_vis, m.zero_sem, m.zero_ins = F32, False, False, False
  m.opt = argparse.Namespace(no_instance=False, gpu_ids=[0])
  m.__dict__.update(preprocess=_boom, _device=_boom, _encoder_eval=_boom, _semantics=_boom)
  try:                                             # the model either reads a flag ...
    from ctu.models.codec import CODECS
    if quantizer is not None:
      m.codec = CODECS[quantizer](m.netE, m.cdtype)
  except ImportError:                              # ... or (before ctu.models.codec) its use_vq attribute
    m.__dict__['use_vq'] = quantizer == 's2hvq'
  return m


def x_dict(w=W):
  return {'label': torch.zeros(N, 1, H, w), 'instance': torch.zeros(N, 1, H, w, dtype=torch.int64),
          'image': torch.zeros(N, 3, H, w)}


def binary_payload(lengths=None):
  lengths = [1] * C if lengths is None else lengths
  return struct.pack('<%dI' % len(lengths), *lengths) + bytes(sum(lengths))


def vq_blob(count=CODE_LEN, n_center=L):
  from ctu.utils import vqstream
  values = [i % n_center for i in range(count)]
  return vqstream._HEADER.pack(vqstream.MAGIC, vqstream.VERSION, 1, count, n_center, 0, vqstream.MODE_PACKED) + \
      vqstream.pack_indices(values, vqstream.index_bits(n_center))


def cases():
  """[(case id, callable(model))]: the id names the call and the malformed input, the quantizer is added by run()."""
  good, odd = x_dict(), x_dict(30)
  out = []
  for name in ('get_code', 'get_context_rate', 'get_eval_rate', 'get_rate_map', 'get_class_rates', 'get_vq_code', 'get_vq_rate',
               'get_coded', 'get_coded_rate', 'get_total_rate'):
    out.append((name + '/good', lambda m, name=name: getattr(m, name)(good)))
    out.append((name + '/64x30', lambda m, name=name: getattr(m, name)(odd)))
  out.append(('get_code/packed', lambda m: m.get_code(good, packed=True)))
  codes = {
      'uint8-packed': torch.zeros(N, BITS // 8, dtype=torch.uint8), 'float32-bits': torch.zeros(N, BITS),
      'int64-indices': torch.zeros(N, CODE_LEN, dtype=torch.int64), 'int32-indices': torch.zeros(N, CODE_LEN, dtype=torch.int32),
      'float64': torch.zeros(N, BITS, dtype=torch.float64), 'int16': torch.zeros(N, CODE_LEN, dtype=torch.int16),
      'list': [[0] * 8] * N, 'none': None,
      'uint8-rank1': torch.zeros(N * BITS // 8, dtype=torch.uint8), 'float32-rank3': torch.zeros(N, 1, BITS),
      'int64-rank1': torch.zeros(N * CODE_LEN, dtype=torch.int64), 'int64-rank3': torch.zeros(N, CODE_LEN, 1, dtype=torch.int64),
      'uint8-short': torch.zeros(N, BITS // 8 - 1, dtype=torch.uint8), 'uint8-batch3': torch.zeros(3, BITS // 8, dtype=torch.uint8),
      'float32-long': torch.zeros(N, BITS + 1), 'float32-packed-size': torch.zeros(N, BITS // 8),
      'int64-short': torch.zeros(N, CODE_LEN - 1, dtype=torch.int64), 'int64-batch3': torch.zeros(3, CODE_LEN, dtype=torch.int64),
      'int32-long': torch.zeros(N, CODE_LEN + 4, dtype=torch.int32)}
  for call in ('decode', 'get_eval_metrics_decoded'):
    for cid, code in codes.items():
      out.append(('%s/%s' % (call, cid), lambda m, call=call, code=code: getattr(m, call)(code, good)))
      out.append(('%s/%s/64x30' % (call, cid), lambda m, call=call, code=code: getattr(m, call)(code, odd)))
  pay, blob = binary_payload(), vq_blob()
  lists = {
      'payloads-good': [pay, pay], 'blobs-good': [blob, blob], 'count-1': [pay], 'count-3-blobs': [blob] * 3, 'empty': [],
      'tuple-payloads': (pay, pay), 'not-a-list': pay, 'none': None, 'text-item': [pay, 'text'], 'text-item-blob': [blob, 'text'],
      'int-item': [7, pay], 'bytearray-items': [bytearray(pay), bytearray(pay)], 'bytearray-blobs': [bytearray(blob), bytearray(blob)],
      'payload-truncated': [pay, pay[:-1]], 'payload-trailing': [pay + b'\0', pay], 'payload-short-table': [pay[:10], pay],
      'payload-empty': [b'', pay], 'payload-wrong-channels': [binary_payload([1] * (C - 1)), pay],
      'blob-truncated': [blob, blob[:-1]], 'blob-trailing': [blob + b'\0', blob], 'blob-header-cut': [blob[:12], blob],
      'blob-empty': [b'', blob], 'blob-magic': [b'XXXX' + blob[4:], blob], 'blob-n_center-16': [blob, vq_blob(CODE_LEN, 16)],
      'blob-n_center-4': [vq_blob(CODE_LEN, 4), blob], 'blob-count-64': [vq_blob(64), blob], 'blob-count-long': [blob, vq_blob(CODE_LEN + 4)]}
  for cid, items in lists.items():
    out.append(('decode_coded/' + cid, lambda m, items=items: m.decode_coded(items, good)))
    out.append(('decode_coded/%s/64x30' % cid, lambda m, items=items: m.decode_coded(items, odd)))
  out.append(('decode_from_files/no-semantics', lambda m: m.decode_from_files([pay, pay], [])))
  return out


def run():
  """[[case id, exception type, message]] on the code this file sits beside; 'returned' for a call that raised nothing."""
  import jpdse_hip
  import jpdse_hip.ops, jpdse_hip.layers  # noqa: E401,F401
  streams = getattr(jpdse_hip, 'streams', jpdse_hip.ops)      # binds `lib` too, where the layout has it
  saved = torch.cuda.is_available, jpdse_hip.lib, jpdse_hip.ops.lib, streams.lib
  touched = lambda: (_ for _ in ()).throw(AssertionError('library touched'))
  torch.cuda.is_available, jpdse_hip.lib, jpdse_hip.ops.lib, streams.lib = (lambda: False), touched, touched, touched
  rows = []
  try:
    for quantizer in (None, 'binarizer', 's2hvq'):
      model = bare_model(quantizer)      # no call gets far enough to change it
      for cid, call in cases():
        try:
          call(model)
          rows.append(['%s/%s' % (quantizer or 'none', cid), 'returned', ''])
        except Exception as e:      # every outcome is a row
          rows.append(['%s/%s' % (quantizer or 'none', cid), type(e).__name__, str(e)])
  finally:
    torch.cuda.is_available, jpdse_hip.lib, jpdse_hip.ops.lib, streams.lib = saved
  return rows


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'codec_refusals.json'))
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
