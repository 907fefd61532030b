"""GPU: the coded label and instance maps (semantics.hip: jpdse_semantics_encode / _decode, ops.semantics_encode /
semantics_decode, trainer.get_coded_semantics / decode_semantics / decode_from_files / get_total_rate) against the
pure-Python coder tests/semantics_ref.py, which was written from the format text of DESIGN.md 4.9.  The coder is lossless
and deterministic: every comparison is exact."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'jpd-se_amd'), os.path.dirname(os.path.abspath(__file__))):
  if _p not in sys.path:
    sys.path.insert(0, _p)

import semantics_cases as cases  # noqa: E402
import semantics_ref as sref  # noqa: E402
import jpdse_hip  # noqa: E402
from jpdse_hip import ops  # noqa: E402

_shape = dict(argnames='shape', argvalues=cases.SHAPES, ids=cases.shape_id)
DEV = torch.device('cuda', 0)
_P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _maps(label, inst, mask):
  """The device tensors the input builder reads."""
  l = torch.from_numpy(np.array(label)).to(DEV).float().unsqueeze(1).contiguous()
  i = torch.from_numpy(np.array(inst)).to(DEV).unsqueeze(1).contiguous() if mask & 2 else None
  return l, i


def device_encode(label, inst, sr):
  """The C call itself: (sizes [N, 2], status [N, 2], payload[n][plane] bytes) -- cut planes included, which ops hides."""
  L = jpdse_hip.lib()
  N, _, H, W = label.shape
  mask = 1 | (2 if inst is not None else 0)
  cap, off = L.jpdse_semantics_capacity(H, W, sr, mask), L.jpdse_semantics_capacity(H, W, sr, 1)
  out = torch.zeros((N, cap), dtype=torch.uint8, device=DEV)
  meta = torch.full((2, N, 2), -7, dtype=torch.int32, device=DEV)
  ws = torch.empty(L.jpdse_semantics_workspace_size(N, H, W, sr, mask), dtype=torch.uint8, device=DEV)
  jpdse_hip.check(L.jpdse_semantics_encode(N, H, W, sr, mask, _P(label), _P(inst), _P(out), cap, _P(meta[0]), _P(meta[1]),
                                           _P(ws), ws.numel(), None), 'semantics_encode')
  torch.cuda.synchronize()
  sizes, status, rows = meta[0].cpu().numpy(), meta[1].cpu().numpy(), out.cpu().numpy()
  pay = [[rows[n, (off if p else 0):(off if p else 0) + sizes[n, p]].tobytes() if mask >> p & 1 else None for p in range(2)]
         for n in range(N)]
  return sizes, status, pay


def device_decode(rows, sizes, inst_off, N, H, W, sr, mask, num_labels=256, guard=64):
  """The C call itself on a row buffer: (label [N, H, W] float32, inst int64 or None, bad [N]).  The outputs sit between
  guard bands of `guard` elements, which must come back untouched."""
  L = jpdse_hip.lib()
  lab = torch.full((N * H * W + 2 * guard,), -5.0, dtype=torch.float32, device=DEV)
  ins = torch.full((N * H * W + 2 * guard,), -5, dtype=torch.int64, device=DEV) if mask & 2 else None
  rows_d = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV)
  sizes_d = torch.tensor(sizes, dtype=torch.int32, device=DEV).reshape(N, 2).contiguous()
  bad = torch.full((N,), -1, dtype=torch.int32, device=DEV)
  jpdse_hip.check(L.jpdse_semantics_decode(N, H, W, sr, mask, num_labels, _P(rows_d), rows_d.shape[1], inst_off, _P(sizes_d),
                                           _P(lab[guard:]), _P(ins[guard:]) if ins is not None else None, _P(bad), None),
                  'semantics_decode')
  torch.cuda.synchronize()
  for t, fill in ((lab, -5.0), (ins, -5)):
    if t is not None:
      assert bool((t[:guard] == fill).all()) and bool((t[-guard:] == fill).all()), 'a guard band was written'
  body = lambda t: t[guard:-guard].view(N, H, W).cpu().numpy() if t is not None else None
  return body(lab), body(ins), bad.cpu().numpy()


def _rows(payloads, N, S, mask):
  """A row buffer of reference payloads: (uint8 [N, stride], sizes [N][2], inst_off)."""
  longest = [max([len(payloads[n][p]) for n in range(N)] + [4 * S]) if mask >> p & 1 else 0 for p in range(2)]
  off = longest[0] if mask == 3 else 0
  rows = np.zeros((N, off + longest[1] if mask == 3 else longest[0] + longest[1]), dtype=np.uint8)
  sizes = np.zeros((N, 2), dtype=np.int32)
  for n in range(N):
    for p in range(2):
      if mask >> p & 1:
        at = off if p else 0
        rows[n, at:at + len(payloads[n][p])] = np.frombuffer(payloads[n][p], dtype=np.uint8)
        sizes[n, p] = len(payloads[n][p])
  return rows, sizes.tolist(), off


@pytest.mark.parametrize('mask', [1, 3], ids=['label', 'both'])
@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize(**_shape)
def test_device_coder_against_the_reference(shape, kind, mask):
  N, H, W, sr = shape
  S = len(sref.strips(H, sr))
  label, inst, coded, _ = cases.reference(shape, kind)
  l, i = _maps(label, inst, mask)
  planes = [p for p in range(2) if mask >> p & 1]
  # 1. the device encoder's payloads are the reference's, byte for byte, cut ones included; status as predicted
  sizes, status, got = device_encode(l, i, sr)
  for n in range(N):
    for p in planes:
      want, cut = coded[n][p]
      assert status[n, p] == (1 if cut else 0), (n, p, status[n, p], cut)
      assert sizes[n, p] == len(want), (n, p, sizes[n, p], len(want))
      assert got[n][p] == want, 'image %d plane %d: first difference at byte %d' % (
          n, p, next(k for k in range(len(want)) if got[n][p][k] != want[k]))
    if mask == 1:
      assert sizes[n, 1] == -7 and status[n, 1] == -7        # the entries of the absent plane are not written
  # 2. the device decoder on the REFERENCE's uncut payloads and on the device's own: the input, exactly
  whole = [n for n in range(N) if not any(coded[n][p][1] for p in planes)]
  for source in ([[coded[n][0][0], coded[n][1][0]] for n in range(N)], got):
    rows, sz, off = _rows(source, N, S, mask)
    dl, di, bad = device_decode(rows, sz, off, N, H, W, sr, mask)
    for n in whole:
      assert bad[n] == 0
      assert np.array_equal(dl[n], label[n].astype(np.float32))
      if mask & 2:
        assert np.array_equal(di[n], inst[n])
  # 3. through ops: raw where a stream was cut or coding does not pay, and the inverse gives the maps back
  items = ops.semantics_encode(l, i, sr)
  for n in range(N):
    assert items[n][1] is None if mask == 1 else items[n][1] is not None
    for p in planes:
      assert tuple(items[n][p]) == sref.entry((label, inst)[p][n], p, sr), (n, p)
  bl, bi = ops.semantics_decode(items, H, W, sr, 256, DEV)
  assert bl.dtype == torch.float32 and bi.dtype == torch.int64 and tuple(bl.shape) == tuple(bi.shape) == (N, 1, H, W)
  assert torch.equal(bl, l) and torch.equal(bi, i if i is not None else torch.zeros_like(bi))


def test_out_of_range_input_sets_status_bit_1_and_ops_names_the_image():
  shape = (3, 19, 33, 8)
  label, inst, _, _ = cases.reference(shape, 'rects')
  for bad_label, bad_inst in ((2.5, None), (-1.0, None), (256.0, None), (float('nan'), None), (None, -1), (None, 1 << 31)):
    l, i = _maps(label, inst, 3)
    if bad_label is not None:
      l[1, 0, 18, 32] = bad_label
    else:
      i[1, 0, 9, 0] = bad_inst
    _, status, _ = device_encode(l, i, 8)
    p = 0 if bad_label is not None else 1
    assert status[1, p] & 2 and not status[0, p] & 2 and not status[2, p] & 2 and not status[1, 1 - p] & 2
    with pytest.raises(ValueError, match='%s map of image 1' % ('label', 'instance')[p]):
      ops.semantics_encode(l, i, 8)


def test_hostile_payloads_are_survived():
  """Length tables that lie and random bytes: the call returns, the guard bands of the outputs stay untouched (checked in
  device_decode) and the outputs have their shape; nothing else is promised about their content."""
  shape = (3, 19, 33, 8)
  N, H, W, sr = shape
  S = 3
  label, inst, coded, _ = cases.reference(shape, 'rects')
  good = [[coded[n][0][0], coded[n][1][0]] for n in range(N)]
  rows, sizes, off = _rows(good, N, S, 3)
  g = np.random.default_rng(5)
  word = lambda v: np.frombuffer(struct.pack('<I', v), dtype=np.uint8)

  def run(r, sz=sizes, o=off):
    dl, di, bad = device_decode(r, sz, o, N, H, W, sr, 3, num_labels=19)
    assert dl.shape == (N, H, W) and di.shape == (N, H, W)
    return dl, di, bad
  for lie in (0xFFFFFFFF, 0x7FFFFFFF, rows.shape[1], 0, 1):
    for entry in range(S):
      r = rows.copy()
      r[:, 4 * entry:4 * entry + 4] = word(lie)
      r[:, off + 4 * entry:off + 4 * entry + 4] = word(lie)
      run(r)
  run(np.zeros_like(rows))
  run(g.integers(0, 256, rows.shape, dtype=np.uint8))
  run(np.full_like(rows, 255))
  # sizes that lie: longer than the row, negative, shorter than the table
  run(rows, [[1 << 30, 1 << 30]] * N)
  run(rows, [[5, 7]] * N)
  dl, di, _ = run(rows, [[-1, 0]] * N)
  assert (dl == -5.0).all() and (di == -5).all()         # size <= 0: the plane is not coded here, nothing is written
  # and the good rows still decode
  dl, di, bad = run(rows)
  assert np.array_equal(dl, label.astype(np.float32)) and np.array_equal(di, inst) and not bad.any()


def test_labels_outside_the_set_are_reported_and_refused():
  from ctu.utils import semantics
  shape = (3, 19, 33, 8)
  N, H, W, sr = shape
  label, inst, coded, _ = cases.reference(shape, 'rects')
  top = int(label.max())
  assert top >= 3
  good = [[coded[n][0][0], coded[n][1][0]] for n in range(N)]
  rows, sizes, off = _rows(good, N, 3, 3)
  _, _, bad = device_decode(rows, sizes, off, N, H, W, sr, 3, num_labels=top + 1)
  assert not bad.any()
  per_image = [int(label[n].max()) for n in range(N)]
  limit = max(per_image)
  _, _, bad = device_decode(rows, sizes, off, N, H, W, sr, 3, num_labels=limit)
  assert [int(b) for b in bad] == [1 if m >= limit else 0 for m in per_image]
  items = [[(1, good[n][0]), (1, good[n][1])] for n in range(N)]
  first = per_image.index(limit)
  with pytest.raises(ValueError, match='label map of image %d' % first):
    ops.semantics_decode(items, H, W, sr, limit, DEV)
  # an instance literal of 2^31 or more: the stream of the single pixel 2^31 + 5, written by the reference's own coder
  stream = sref.encode_stream([(1 << 31) + 5], 1, 1, 1)
  payload = struct.pack('<I', len(stream)) + stream
  lab1 = sref.encode_plane(np.array([[3]]), 0, 8)[0]
  with pytest.raises(ValueError, match='instance map of image 0'):
    ops.semantics_decode([[(1, lab1), (1, payload)]], 1, 1, 8, 19, DEV)
  # the model refuses the file: decode_semantics raises before the input builder sees the map
  tr = _trainer('fp32')
  blobs = [semantics.pack(H, W, sr, [(1, sref.encode_plane(np.full((H, W), 200), 0, sr)[0]), (1, good[0][1])])]
  assert tr.model._label_set() <= 200
  with pytest.raises(ValueError, match='label map of image 0'):
    tr.decode_semantics(blobs)


def test_real_map_bytes_and_round_trip():
  label, inst, coded = cases.golden()
  l, i = _maps(label[None], inst[None], 3)
  sizes, status, got = device_encode(l, i, 8)
  assert status.tolist() == [[0, 0]]
  assert got[0][0] == coded[0][0] and got[0][1] == coded[1][0]
  items = ops.semantics_encode(l, i)
  assert [e[0] for e in items[0]] == [1, 1]
  bl, bi = ops.semantics_decode(items, 512, 1024, 8, 35, DEV)
  assert torch.equal(bl, l) and torch.equal(bi, i)


# ---- end to end -----------------------------------------------------------------------------------------------------------
_trainers = {}


def _trainer(dtype, **kw):
  from ctu.trainers import get_trainer
  from ctu.utils.synthetic import default_opt
  key = (dtype, tuple(sorted(kw.items())))
  if key not in _trainers:
    opt = default_opt(gpu_ids=[0], print_losses=False, ngf=8, ndf=8, n_blocks_global=1, no_feat_encoding=False,
                      no_encoder_binarization=False, feat_num=3, nef=8, n_downsample_E=4, encoder_binarizer_out_channels=32,
                      compute_dtype=dtype, **kw)
    torch.manual_seed(4321)
    _trainers[key] = get_trainer(opt)(opt, 'train')
  return _trainers[key]


@pytest.mark.parametrize('no_instance', [False, True], ids=['instance', 'no_instance'])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_decode_from_files_and_the_total_rate(dtype, no_instance, tmp_path):
  from ctu.utils import entropy, semantics
  from ctu.utils.synthetic import synthetic_batch
  tr = _trainer(dtype, **(dict(no_instance=True) if no_instance else {}))
  N, H, W = 2, 64, 128
  xd = synthetic_batch(N, H, W, seed=5)
  payloads, blobs = tr.get_coded(xd), tr.get_coded_semantics(xd)
  assert isinstance(blobs, list) and len(blobs) == N and all(isinstance(b, bytes) for b in blobs)
  want = tr.decode_coded(payloads, dict(label=xd['label'], instance=xd['instance']))
  got = tr.decode_from_files(payloads, blobs)
  assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)
  sem = tr.decode_semantics(blobs)
  assert torch.equal(sem['label'].cpu(), xd['label'].float()) and sem['instance'].dtype == torch.int64
  if no_instance:
    assert all(semantics.unpack(b)[3] == 1 for b in blobs) and not bool(sem['instance'].any())
  else:
    assert all(semantics.unpack(b)[3] == 3 for b in blobs) and torch.equal(sem['instance'].cpu(), xd['instance'].long())
  # the blobs are the reference coder's files
  for n in range(N):
    planes = [sref.entry(xd['label'][n, 0].numpy().astype(np.int64), 0, 8),
              None if no_instance else sref.entry(xd['instance'][n, 0].numpy().astype(np.int64), 1, 8)]
    assert blobs[n] == semantics.pack(H, W, 8, planes)
  # the rate is the size of the files
  shape = tr.model.netE.code_shape(H, W)
  packed = tr.get_code(xd, packed=True)
  code_bytes = [entropy.write_coded(str(tmp_path / ('i%d.jpda' % n)), payloads[n], packed[n].cpu(), shape) for n in range(N)]
  sem_bytes = [semantics.write(str(tmp_path / ('i%d.jpds' % n)), blobs[n]) for n in range(N)]
  assert [os.path.getsize(str(tmp_path / ('i%d.jpds' % n))) for n in range(N)] == sem_bytes
  code_bpp, sem_bpp, total = tr.get_total_rate(xd)
  assert code_bpp == sum(8.0 * b / (H * W) for b in code_bytes) / N == tr.get_coded_rate(xd)[0]
  assert sem_bpp == sum(8.0 * b / (H * W) for b in sem_bytes) / N and total == code_bpp + sem_bpp
  assert torch.equal(tr.decode_from_files(payloads, [semantics.read(str(tmp_path / ('i%d.jpds' % n))) for n in range(N)]), want)
