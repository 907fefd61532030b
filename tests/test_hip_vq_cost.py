"""GPU: the code-length maps of the two S2HVQ index coders (vq_cost.hip: ops.vq_index_cost / ops.vq_plane_cost, the trainer's
get_vq_rate_map / get_vq_class_rates) against the pure-Python restatement tests/vq_cost_ref.py, which was written from the
definitions of DESIGN.md 4.20.  Costs are integers: every comparison of costs is exact.  The bound between a stream's model
length and its bytes is checked against the DEVICE coders' payloads, stream by stream.

Trainer level: a 64 x 128 batch.  get_eval_metrics refuses anything below 176 on the shorter side (five MS-SSIM
scales), so the one comparison with its per-class pixel counts runs, on the same trainer, on a synthetic batch of the smallest
size both calls take, 176 x 192; at 64 x 128 the pixel counts are held against the Python reference instead."""
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

import code_cost_cases as ccases  # noqa: E402
import vq_plane_cases as pcases  # noqa: E402
import vq_cost_ref as cref  # noqa: E402
from jpdse_hip import ops  # noqa: E402

DEV = torch.device('cuda', 0)
KEYS = ('symbol', 'cell', 'group', 'stream_units', 'stream_decisions')


def _dev(v):
  return torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32)).to(DEV)


def _host(r):
  return {k: (v.cpu().numpy().astype(np.int64) if v is not None else None) for k, v in r.items()}


def _equal(got, want, what):
  got = _host(got)
  for k in KEYS:
    assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)
  assert int(got['status'][0]) == want['status'], (what, 'status')
  return got


def _bound(payload, got, S, what):
  """Every stream of the device coder's payload within the bound of its own units and decisions; returns the gaps."""
  lens = struct.unpack('<%dI' % S, payload[:4 * S])
  assert sum(lens) == len(payload) - 4 * S
  gaps = [cref.gap_bits(n, int(u)) for n, u in zip(lens, got['stream_units'])]
  assert len(gaps) == S == len(got['stream_decisions'])
  for s, gap in enumerate(gaps):
    assert abs(gap) <= cref.bound_bits(int(got['stream_decisions'][s])), (what, s, gap)
  return gaps


def _index_source(kind, M, L, seed):
  rng = np.random.default_rng([seed, M, L])
  if kind == 'zeros':
    return np.zeros(M, dtype=np.int64)
  if kind == 'uniform':
    return rng.integers(0, L, size=M)
  return np.minimum(rng.integers(0, L, size=M), rng.integers(0, L, size=M)) * (rng.random(M) < 0.7)      # skewed towards 0


# ---- the index walk -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', [1, 63, 64, 65, 1000])
@pytest.mark.parametrize('L', [2, 3, 64, 512])
def test_index_costs_equal_the_reference_and_respect_the_bound(L, M):
  """S = 1, 3, 64, 65 and M: a partly filled wave (idle lanes past the table barrier), more than one wave, one symbol per
  stream; L = 512 takes the LDS opt-in."""
  gaps, ran = [], 0
  for S in sorted({S for S in (1, 3, 64, 65, M) if S <= M}):
    for G in (1, 4):
      if M % G:
        continue
      for kind in ('uniform', 'skew', 'zeros'):
        v = _index_source(kind, M, L, S)
        what = (L, M, S, G, kind)
        first = ops.vq_index_cost(_dev(v), L, S, G, want_symbols=True)
        got = _equal(first, cref.index_cost(v.tolist(), L, S, G), what)
        assert np.array_equal(got['stream_decisions'], [cref.index_bits(L) * ((M - s + S - 1) // S) for s in range(S)])
        gaps += _bound(ops.vq_index_encode(_dev(v), L, S), got, S, what)
        ran += 1
  assert ran >= 3
  print('L %d, M %d: 8 * bytes - bits per stream between %+.2f and %+.2f over %d streams' % (L, M, min(gaps), max(gaps), len(gaps)))


# ---- the plane walk -----------------------------------------------------------------------------------------------------------
def _plane_source(kind, h, w, G, L, seed):
  rng = np.random.default_rng([seed, h, w, G, L])
  if kind == 'constant':
    v = np.full((h, w, G), L - 1)
  elif kind == 'uniform':
    v = rng.integers(0, L, size=(h, w, G))
  else:                                        # repeats its neighbour: every flag branch is taken
    v = pcases.correlated(rng, h, w, G, L)
  return np.ascontiguousarray(v).reshape(-1)


@pytest.mark.parametrize('L', [2, 5, 64, 512])
@pytest.mark.parametrize('plane', [(1, 1, 1), (1, 7, 1), (7, 1, 2), (9, 5, 3), (17, 33, 4)], ids=lambda p: '%dx%dx%d' % p)
def test_plane_costs_equal_the_reference_and_respect_the_bound(plane, L):
  """strip_rows 1 (no upper cell), 8 (a short last strip) and 100 (a single strip)."""
  h, w, G = plane
  gaps = []
  for strip_rows in (1, 8, 100):
    S = (h + strip_rows - 1) // strip_rows * G
    for kind in ('constant', 'uniform', 'correlated'):
      v = _plane_source(kind, h, w, G, L, strip_rows)
      what = (plane, L, strip_rows, kind)
      first = ops.vq_plane_cost(_dev(v), plane, L, strip_rows, want_symbols=True)
      got = _equal(first, cref.plane_cost(v.tolist(), h, w, G, L, strip_rows), what)
      assert got['stream_units'].shape == (S,)
      gaps += _bound(ops.vq_plane_encode(_dev(v), h, w, G, L, strip_rows), got, S, what)
  print('%s, L %d: 8 * bytes - bits per stream between %+.2f and %+.2f over %d streams' % (plane, L, min(gaps), max(gaps), len(gaps)))


# ---- bad indices ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', [5, 64])
def test_a_bad_index_is_priced_as_zero_and_reported(L):
  h, w, G, S = 9, 5, 4, 7
  M = h * w * G
  v = _plane_source('correlated', h, w, G, L, 3)
  bad = v.copy()
  bad[17], bad[M - 3] = -1, L
  as_zero = bad.copy()
  as_zero[17] = as_zero[M - 3] = 0
  for name, call, ref in (('index', lambda t: ops.vq_index_cost(_dev(t), L, S, G, want_symbols=True),
                           lambda t: cref.index_cost(t.tolist(), L, S, G)),
                          ('plane', lambda t: ops.vq_plane_cost(_dev(t), (h, w, G), L, 4, want_symbols=True),
                           lambda t: cref.plane_cost(t.tolist(), h, w, G, L, 4))):
    want = ref(bad)
    assert want['status'] == 2
    got = _equal(call(bad), want, (name, 'bad'))
    clean = _equal(call(as_zero), ref(as_zero), (name, 'as zero'))
    assert int(clean['status'][0]) == 0
    for k in KEYS:                             # nothing else changes
      assert np.array_equal(got[k], clean[k]), (name, k)
    assert int(_host(call(v))['status'][0]) == 0


# ---- class tables -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_classes', [19, 151])
@pytest.mark.parametrize('plane', [(9, 5, 3), (17, 33, 4)], ids=lambda p: '%dx%dx%d' % p)
def test_class_tables_equal_the_reference(plane, n_classes):
  h, w, G = plane
  L, s, S = 64, 4, 6
  v = _plane_source('correlated', h, w, G, L, n_classes)
  label = ccases.make_label(1, s * h, s * w, n_classes, seed=5)           # fractional, negative, out-of-range and NaN labels
  assert np.isnan(label).any()
  dev_label = torch.from_numpy(label).to(DEV)
  for name, first, want in (('index', ops.vq_index_cost(_dev(v), L, S, G, dev_label, n_classes, (h, w)), cref.index_cost(v.tolist(), L, S, G)),
                            ('plane', ops.vq_plane_cost(_dev(v), plane, L, 8, dev_label, n_classes), cref.plane_cost(v.tolist(), h, w, G, L, 8))):
    got = _host(first)
    units, pixels = cref.class_tables(want['cell'].reshape(1, h, w), label, n_classes)
    assert got['class_units'].shape == (n_classes + 1,) and np.array_equal(got['class_units'], units[0]), name
    assert np.array_equal(got['class_pixels'], pixels[0]) and np.array_equal(got['cell'], want['cell']), name
    assert got['class_pixels'][-1] >= 1 and got['class_units'][-1] > 0
    assert int(got['class_units'].sum()) == s * s * int(got['cell'].sum()) and int(got['class_pixels'].sum()) == s * s * h * w
    assert got['symbol'] is None


# ---- determinism ------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_tensors_and_symbols_are_optional():
  h, w, G, L = 17, 33, 4, 512
  v = _dev(_plane_source('correlated', h, w, G, L, 11))
  label = torch.from_numpy(ccases.make_label(1, 2 * h, 2 * w, 19, seed=2)).to(DEV)
  for call in (lambda sym: ops.vq_index_cost(v, L, 65, G, label, 19, (h, w), want_symbols=sym),
               lambda sym: ops.vq_plane_cost(v, (h, w, G), L, 8, label, 19, want_symbols=sym)):
    first, again, bare = call(True), call(True), call(False)
    assert bare['symbol'] is None and first['symbol'].dtype == torch.int32
    for k in first:
      assert torch.equal(first[k], again[k]), k
      if k != 'symbol':
        assert torch.equal(first[k], bare[k]), k


# ---- trainer level: the tiny s2hvq trainer of tests/test_hip_vq_plane.py, 19 labels ------------------------------------------------
N, H, W, C, D, L_VQ, DOWN, LABELS = 2, 64, 128, 16, 4, 8, 2, 19
PLANES = (H >> DOWN, W >> DOWN, C // D)
_shared = {}


def _trainer(**over):
  from ctu.trainers import get_trainer
  from oracle.ctu_cpu import model as omodel
  kw = dict(gpu_ids=[0], print_losses=False, compute_dtype='fp32', ngf=8, ndf=8, n_blocks_global=1, n_downsample_global=2,
            no_feat_encoding=False, no_encoder_binarization=False, feat_num=3, nef=8, n_downsample_E=DOWN, num_labels=LABELS,
            encoder_binarizer_out_channels=C, encoder_quantizer='s2hvq', vq_n_center=L_VQ, vq_center_size=D, vq_sigma=10.0,
            no_vgg_loss=True, no_gan_feat_loss=True, no_g_gan_loss=True, no_d_gan_loss=True, skip_unused_losses=True)
  kw.update(over)
  opt = omodel.default_opt(**kw)
  torch.manual_seed(1234)
  tr = get_trainer(opt)(opt, 'train')
  with torch.no_grad():                          # a code book at the scale of the features: more than one centre in use
    tr.model.netE._vq.vq._code_book.mul_(0.05)
  return tr


def _setup():
  """(flag-off trainer, flag-on trainer with the same weights, batch), built once."""
  if not _shared:
    from oracle.ctu_cpu import model as omodel
    _shared['v'] = (_trainer(), _trainer(vq_context_coder=True), omodel.synthetic_batch(N, H, W, seed=3, num_labels=LABELS))
  return _shared['v']


def _stream_lengths(blob):
  """(coder, the stream byte lengths) of a blob get_coded returned; None for a packed .jpdv blob, which holds no streams."""
  from ctu.utils import vqplane, vqstream
  if blob[:4] == vqplane.MAGIC:
    h, w, G, _, strip_rows, body = vqplane.parse_blob(blob)
    S = (h + strip_rows - 1) // strip_rows * G
    return 'plane', struct.unpack('<%dI' % S, body[:4 * S])
  _, _, _, S, mode, body = vqstream.parse_blob(blob)
  return 'index', (struct.unpack('<%dI' % S, body[:4 * S]) if mode == vqstream.MODE_CODED else None)


def _check_map(tr, xd, coder, want_coders):
  h, w, G = PLANES
  rm = tr.get_vq_rate_map(xd, coder)
  assert set(rm) == {'map', 'per_group', 'bits', 'bpp', 'stream_bits', 'stream_decisions', 'coder'}
  assert rm['map'].shape == (N, h, w) and rm['per_group'].shape == (N, G) and rm['bits'].shape == (N,) and rm['bpp'].shape == (N,)
  assert all(rm[k].dtype == torch.float64 and rm[k].device.type == 'cpu' for k in ('map', 'per_group', 'bits', 'bpp'))
  assert rm['coder'] == want_coders and len(rm['stream_bits']) == len(rm['stream_decisions']) == N
  # all are integers / 65536: the float64 sums are exact
  assert torch.equal(rm['map'].sum(dim=(1, 2)), rm['bits']) and torch.equal(rm['per_group'].sum(dim=1), rm['bits'])
  assert torch.equal(rm['bpp'], rm['bits'] / (H * W))
  code = tr.get_vq_code(xd).cpu().numpy()
  for n in range(N):
    assert rm['stream_bits'][n].dtype == torch.float64 and rm['stream_decisions'][n].dtype == torch.int64
    assert float(rm['stream_bits'][n].sum()) == float(rm['bits'][n])
    if want_coders[n] == 'plane':
      want = cref.plane_cost(code[n].tolist(), h, w, G, L_VQ, 8)
    else:
      want = cref.index_cost(code[n].tolist(), L_VQ, G * 8, G)
    assert np.array_equal((rm['map'][n] * 65536.0).numpy().reshape(-1), want['cell'].astype(np.float64))
    assert np.array_equal((rm['per_group'][n] * 65536.0).numpy(), want['group'].astype(np.float64))
    assert np.array_equal(rm['stream_decisions'][n].numpy(), want['stream_decisions'])
  return rm


def _check_streams(rm, n, coder, lens):
  """Image n: | 8 * payload stream bytes - bits | within the summed per-stream bounds, and every stream within its own."""
  assert coder == rm['coder'][n] and len(lens) == rm['stream_bits'][n].numel()
  gap = 8.0 * sum(lens) - float(rm['bits'][n])
  bound = sum(cref.bound_bits(int(d)) for d in rm['stream_decisions'][n])
  print('image %d (%s): %d stream bytes, model %.3f bits, gap %.3f, summed bound %.3f' % (n, coder, sum(lens), float(rm['bits'][n]),
                                                                                          gap, bound))
  assert abs(gap) <= bound
  for s, nbytes in enumerate(lens):
    assert abs(8.0 * nbytes - float(rm['stream_bits'][n][s])) <= cref.bound_bits(int(rm['stream_decisions'][n][s])), (n, s)


def _check_against_blobs(rm, blobs):
  """The blobs of get_coded against the map, where a blob holds streams of the priced coder; returns how many did."""
  compared = 0
  for n, blob in enumerate(blobs):
    coder, lens = _stream_lengths(blob)
    if coder == rm['coder'][n] and lens is not None:
      _check_streams(rm, n, coder, lens)
      compared += 1
  return compared


def _check_against_index_payloads(tr, xd, rm):
  """The .jpdv model against the coded payload write_indices makes, whether or not the file kept it (at this size the packed
  form is the smaller one)."""
  S = PLANES[2] * 8
  code = tr.get_vq_code(xd)
  for n in range(N):
    payload = ops.vq_index_encode(code[n].to(torch.int32).contiguous(), L_VQ, S)
    _check_streams(rm, n, 'index', struct.unpack('<%dI' % S, payload[:4 * S]))


def test_trainer_rate_map_without_the_context_coder():
  off, _, xd = _setup()
  before = off.get_img(xd).clone(), off.get_coded(xd), off.get_vq_code(xd).clone()
  rm = _check_map(off, xd, None, ['index'] * N)
  forced = _check_map(off, xd, 'index', ['index'] * N)
  assert all(torch.equal(rm[k], forced[k]) for k in ('map', 'per_group', 'bits', 'bpp'))
  blobs = off.get_coded(xd)
  assert all(b[:4] == b'JPDV' for b in blobs)
  assert _check_against_blobs(rm, blobs) == sum(1 for b in blobs if _stream_lengths(b)[1] is not None)
  _check_against_index_payloads(off, xd, rm)
  plane = _check_map(off, xd, 'plane', ['plane'] * N)            # the other model can be forced, whatever file is kept
  assert not torch.equal(plane['bits'], rm['bits'])
  # the existing calls return what they returned before
  assert torch.equal(off.get_img(xd), before[0]) and off.get_coded(xd) == before[1] and torch.equal(off.get_vq_code(xd), before[2])


def test_trainer_rate_map_with_the_context_coder():
  from ctu.utils import vqplane
  off, on, xd = _setup()
  before = on.get_img(xd).clone(), on.get_coded(xd), on.get_vq_code(xd).clone()
  kept = ['plane' if b[:4] == vqplane.MAGIC else 'index' for b in before[1]]
  rm = _check_map(on, xd, None, kept)
  _check_against_blobs(rm, before[1])
  compared = 0
  for coder in ('index', 'plane'):
    forced = _check_map(on, xd, coder, [coder] * N)
    compared += _check_against_blobs(forced, before[1])
    if coder == 'index':
      _check_against_index_payloads(on, xd, forced)
    assert torch.equal(forced['map'], _check_map(off, xd, coder, [coder] * N)['map'])       # the flag changes no price
    for n in range(N):
      if kept[n] == coder:
        assert torch.equal(forced['map'][n], rm['map'][n])
  # every image's kept blob was held against the model it was coded with, unless it is a packed .jpdv (no streams)
  assert compared == sum(1 for b in before[1] if _stream_lengths(b)[1] is not None)
  # both containers against their models, whichever was kept: the .jpdw blobs made directly
  code = on.get_vq_code(xd)
  planes = [vqplane.write_planes(None, code[n], PLANES, L_VQ) for n in range(N)]
  assert _check_against_blobs(_check_map(on, xd, 'plane', ['plane'] * N), planes) == N
  assert torch.equal(on.get_img(xd), before[0]) and on.get_coded(xd) == before[1] and torch.equal(on.get_vq_code(xd), before[2])


@pytest.mark.parametrize('coder', [None, 'index', 'plane'])
def test_trainer_class_rates(coder):
  _, on, xd = _setup()
  h, w, G = PLANES
  rm, cr = on.get_vq_rate_map(xd, coder), on.get_vq_class_rates(xd, coder)
  n_classes = on.model.n_onehot
  assert n_classes == LABELS
  assert set(cr) == {'pixels', 'bits', 'bpp', 'share', 'per_image'} and set(cr['per_image']) == {'pixels', 'bits', 'bpp', 'share'}
  assert cr['bits'].shape == (n_classes + 1,) and cr['per_image']['bits'].shape == (N, n_classes + 1)
  per = cr['per_image']
  assert float(((per['bits'].sum(dim=1) - rm['bits']).abs() / rm['bits']).max()) <= 1e-9
  assert abs(float(cr['share'].sum()) - 1.0) <= 1e-9 and float((per['share'].sum(dim=1) - 1.0).abs().max()) <= 1e-9
  assert int(cr['pixels'].sum()) == N * H * W
  seen = per['pixels'] > 0
  assert bool(torch.isnan(per['bpp'][~seen]).all()) and not bool(torch.isnan(per['bpp'][seen]).any())
  assert torch.equal(per['bpp'][seen], per['bits'][seen] / per['pixels'][seen].to(torch.float64))
  # the reference's class table on the map
  cell = (rm['map'] * 65536.0).numpy().astype(np.int64)
  units, pixels = cref.class_tables(cell, xd['label'].numpy(), n_classes)
  s = H // h
  assert np.array_equal(per['pixels'].numpy(), pixels)
  assert np.array_equal(per['bits'].numpy(), units.astype(np.float64) / (65536.0 * s * s))
  assert int((cr['pixels'] > 0).sum()) >= 2


def test_trainer_class_rows_line_up_with_the_per_class_distortion():
  from oracle.ctu_cpu import model as omodel
  _, on, _ = _setup()
  n, hh, ww = 2, 176, 192
  xd = omodel.synthetic_batch(n, hh, ww, seed=77, num_labels=LABELS)
  cr = on.get_vq_class_rates(xd)
  em = on.get_eval_metrics(xd, per_class=True)['per_class']
  per = cr['per_image']
  assert torch.equal(per['pixels'][:, :-1], em['per_image']['pixels']) and torch.equal(cr['pixels'][:-1], em['pixels'])
  assert int(cr['pixels'][-1]) == em['unlabelled'] and int(cr['pixels'].sum()) == n * hh * ww
  assert int((em['pixels'] > 0).sum()) >= 2


def test_trainer_refusals_on_a_real_model():
  off, _, xd = _setup()
  with pytest.raises(ValueError, match='coder'):
    off.get_vq_rate_map(xd, coder='jpdw')
  with pytest.raises(ValueError, match='coder'):
    off.get_vq_class_rates(xd, coder='both')
  for call in ('get_rate_map', 'get_class_rates'):
    with pytest.raises(ValueError, match='not available with --encoder_quantizer s2hvq'):
      getattr(off, call)(xd)
