"""GPU: the code-length map of the learned codec (code_cost.hip: ops.code_cost, trainer.get_rate_map / get_class_rates)
against the pure-Python restatement tests/code_cost_ref.py, which was written from the definitions of DESIGN.md 4.12.  Every
figure is an integer sum of integer costs: every comparison with the reference is exact.  The bound between the model's
length and the coder's bytes (48 + h * w / 64 bits per stream) is derived in DESIGN.md 4.12 and checked on the CPU in
tests/test_code_cost_host.py; here it is held against the DEVICE coder's stream lengths."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'jpd-se_amd'), os.path.dirname(os.path.abspath(__file__))):
  if _p not in sys.path:
    sys.path.insert(0, _p)

import code_cost_cases as cases  # noqa: E402
import code_cost_ref as ccref  # noqa: E402
from jpdse_hip import F32, BF16, ops  # noqa: E402

_shape = dict(argnames='shape', argvalues=cases.SHAPES, ids=cases.shape_id)
_dtype = dict(argnames='dtype', argvalues=[F32, BF16], ids=['fp32', 'bf16'])
DEV = torch.device('cuda', 0)
KEYS = ('cell', 'channel')


def _act(b, dtype):
  return ops.nchw_to_nhwc(torch.from_numpy(np.array(b)).to(DEV), dtype)


def _host(r):
  return {k: (v.cpu().numpy().astype(np.int64) if v is not None else None) for k, v in r.items()}


@pytest.mark.parametrize(**_dtype)
@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize(**_shape)
def test_costs_equal_the_reference(shape, kind, dtype):
  N, C, h, w = shape
  b, want = cases.reference(shape, kind)
  act = _act(b, dtype)
  if act.Cs > C:
    act.t[..., C:] = 3.0                       # the padding lanes of the code are not streams: never read
  first = ops.code_cost(act, want_symbols=True)
  got = _host(first)
  # 1. exact equality, symbol by symbol and for both aggregates
  assert got['symbol'].shape == (N, h, w, C) and got['cell'].shape == (N, h, w) and got['channel'].shape == (N, C)
  assert first['class_units'] is None and first['class_pixels'] is None
  bad = np.argwhere(got['symbol'] != want['symbol'])
  assert bad.size == 0, 'first wrong symbol at (n, y, x, c) = %s: %d, reference %d' % (
      tuple(bad[0]), got['symbol'][tuple(bad[0])], want['symbol'][tuple(bad[0])])
  for k in KEYS:
    assert np.array_equal(got[k], want[k]), k
  # 2. the identities, on the device's own numbers
  assert np.array_equal(got['channel'].sum(axis=1), got['cell'].sum(axis=(1, 2)))
  assert np.array_equal(got['symbol'].sum(axis=3), got['cell']) and np.array_equal(got['symbol'].sum(axis=(1, 2)), got['channel'])
  # 3. a second call is bit-identical
  again = ops.code_cost(act, want_symbols=True)
  for k in KEYS + ('symbol',):
    assert torch.equal(again[k], first[k]), k
  # 4. the aggregates do not depend on whether the symbols are wanted
  lean = ops.code_cost(act)
  assert lean['symbol'] is None
  for k in KEYS:
    assert torch.equal(lean[k], first[k]), k
  # 5. an image of a batch equals the same image run alone
  for n in range(N if N > 1 else 0):
    alone = ops.code_cost(act.batch_slice(n, n + 1), want_symbols=True)
    for k in KEYS + ('symbol',):
      assert torch.equal(alone[k][0], first[k][n]), (k, n)


@pytest.mark.parametrize(**_dtype)
@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize(**_shape)
def test_bound_against_the_device_coder(shape, kind, dtype):
  """Per stream |8 * bytes - units / 65536| <= 48 + h * w / 64, the bytes being the device coder's (its length tables)."""
  N, C, h, w = shape
  b, _ = cases.reference(shape, kind)
  act = _act(b, dtype)
  channel = ops.code_cost(act)['channel'].cpu().numpy()
  payloads = ops.code_entropy_encode(act)
  lens = np.stack([np.frombuffer(p[:4 * C], dtype='<u4').astype(np.int64) for p in payloads])
  assert lens.shape == (N, C) and all(len(p) == 4 * C + int(lens[n].sum()) for n, p in enumerate(payloads))
  gap = 8.0 * lens - channel / 65536.0
  print('%s %s: 8 * bytes - bits in [%.3f, %.3f], bound %.3f' % (cases.shape_id(shape), kind, gap.min(), gap.max(),
                                                                 ccref.bound_bits(h, w)))
  assert np.abs(gap).max() <= ccref.bound_bits(h, w)


@pytest.mark.parametrize('s,n_classes', [(2, 35), (16, 151)], ids=['s2-35', 's16-151'])
@pytest.mark.parametrize('kind', ['half', 'blob'])
@pytest.mark.parametrize(**_shape)
def test_class_tables_equal_the_reference(shape, kind, s, n_classes):
  N, C, h, w = shape
  b, want = cases.reference(shape, kind)
  label = cases.make_label(N, s * h, s * w, n_classes, seed=s)            # fractional, negative, out-of-range and NaN labels
  assert np.isnan(label).any() or label.size < 8
  want_units, want_pixels = ccref.class_tables(want['cell'], label, n_classes)
  act = _act(b, F32)
  dev_label = torch.from_numpy(label).to(DEV)
  first = ops.code_cost(act, dev_label, n_classes)
  got = _host(first)
  assert got['class_units'].shape == (N, n_classes + 1) and got['class_pixels'].shape == (N, n_classes + 1)
  assert np.array_equal(got['class_pixels'], want_pixels)
  assert np.array_equal(got['class_units'], want_units)
  assert np.array_equal(got['cell'], want['cell']) and np.array_equal(got['channel'], want['channel'])
  # the remainder row is populated, and the rows add up to every cell counted s * s times
  assert (got['class_pixels'][:, -1] >= 1).all() and (got['class_units'][:, -1] > 0).all()
  assert np.array_equal(got['class_units'].sum(axis=1), s * s * got['cell'].sum(axis=(1, 2)))
  assert np.array_equal(got['class_pixels'].sum(axis=1), np.full(N, s * s * h * w))
  # integer atomics: a second call is bit-identical, and so is each image alone
  again = ops.code_cost(act, dev_label, n_classes)
  for k in ('class_units', 'class_pixels'):
    assert torch.equal(again[k], first[k]), k
  for n in range(N if N > 1 else 0):
    alone = ops.code_cost(act.batch_slice(n, n + 1), dev_label[n:n + 1].contiguous(), n_classes)
    for k in ('class_units', 'class_pixels'):
      assert torch.equal(alone[k][0], first[k][n]), (k, n)


def test_wrapper_refusals():
  b, _ = cases.reference((2, 5, 3, 37), 'half')
  act = _act(b, F32)
  with pytest.raises(ValueError, match='n_classes without a label map'):
    ops.code_cost(act, None, 35)
  import jpdse_hip
  label = torch.zeros((2, 1, 9, 111), dtype=torch.float32, device=DEV)     # 3 x: no power of two
  with pytest.raises(jpdse_hip.JpdseError, match='power-of-two multiple'):
    ops.code_cost(act, label, 35)
  label = torch.zeros((2, 1, 6, 74), dtype=torch.float32, device=DEV)
  with pytest.raises(jpdse_hip.JpdseError, match='n_classes 300 outside'):
    ops.code_cost(act, label, 300)
  assert int(ops.code_cost(act, label, 35)['class_pixels'][:, 0].sum()) == 2 * 6 * 74        # and the binding is still usable


# ---- trainer level: the learned_codec_nef8.npz trainer of tests/test_hip_learned_codec_golden.py -------------------------------
@pytest.fixture(scope='module')
def golden(golden_dir, tmp_path_factory):
  import test_hip_learned_codec_golden as tg
  z = np.load(os.path.join(golden_dir, 'learned_codec_nef8.npz'))
  gold = {k: z[k] for k in z.files}
  return tg._test_trainer(gold, tmp_path_factory.mktemp('code_cost')), tg._batch(gold)


def test_trainer_rate_map_and_class_rates(golden):
  te, xd = golden
  N, H, W = int(xd['image'].shape[0]), int(xd['image'].shape[-2]), int(xd['image'].shape[-1])
  C, h, w = te.model.netE.code_shape(H, W)
  rm = te.get_rate_map(xd)
  assert set(rm) == {'map', 'per_channel', 'bits', 'bpp'}
  assert rm['map'].shape == (N, h, w) and rm['per_channel'].shape == (N, C) and rm['bits'].shape == (N,) and rm['bpp'].shape == (N,)
  assert all(v.dtype == torch.float64 and v.device.type == 'cpu' for v in rm.values())
  # map and per_channel sum to bits (all three are integers / 65536: the float64 sums are exact)
  assert torch.equal(rm['map'].sum(dim=(1, 2)), rm['bits']) and torch.equal(rm['per_channel'].sum(dim=1), rm['bits'])
  assert torch.equal(rm['bpp'], rm['bits'] / (H * W))
  # the totals against the payloads behind get_coded_rate: C streams per image, each within its bound
  payloads = te.get_coded(xd)
  for n, p in enumerate(payloads):
    stream_bits = 8.0 * (len(p) - 4 * C)
    gap = stream_bits - float(rm['bits'][n])
    print('image %d: %d stream bytes, model %.3f bits, gap %.3f, summed bound %.3f' % (n, len(p) - 4 * C, float(rm['bits'][n]), gap,
                                                                                        C * ccref.bound_bits(h, w)))
    assert abs(gap) <= C * ccref.bound_bits(h, w)
  # the same code through ops and the reference: the map is the eval-mode code's
  code = te.get_code(xd).cpu().numpy().reshape(N, C, h, w) * 2.0 - 1.0
  want = ccref.code_cost(code)
  assert np.array_equal((rm['map'] * 65536.0).numpy(), want['cell'].astype(np.float64))
  assert np.array_equal((rm['per_channel'] * 65536.0).numpy(), want['channel'].astype(np.float64))
  # per-class rates
  cr = te.get_class_rates(xd)
  n_classes = te.model.n_onehot
  assert set(cr) == {'pixels', 'bits', 'bpp', 'share', 'per_image'} and set(cr['per_image']) == {'pixels', 'bits', 'bpp', 'share'}
  assert cr['bits'].shape == (n_classes + 1,) and cr['per_image']['bits'].shape == (N, n_classes + 1)
  per = cr['per_image']
  rel = (per['bits'].sum(dim=1) - rm['bits']).abs() / rm['bits']
  assert float(rel.max()) <= 1e-9, rel
  assert abs(float(cr['bits'].sum()) - float(rm['bits'].sum())) <= 1e-9 * float(rm['bits'].sum())
  assert abs(float(cr['share'].sum()) - 1.0) <= 1e-9 and float((per['share'].sum(dim=1) - 1.0).abs().max()) <= 1e-9
  assert int(cr['pixels'].sum()) == N * H * W
  seen = per['pixels'] > 0
  assert bool(torch.isnan(per['bpp'][~seen]).all()) and not bool(torch.isnan(per['bpp'][seen]).any())
  assert torch.equal(per['bpp'][seen], per['bits'][seen] / per['pixels'][seen].to(torch.float64))
  # the reference's class table on the reference's cells
  units, pixels = ccref.class_tables(want['cell'], xd['label'].numpy(), n_classes)
  s = H // h
  assert np.array_equal(per['pixels'].numpy(), pixels)
  assert np.array_equal(per['bits'].numpy(), units.astype(np.float64) / (65536.0 * s * s))
  # the forward modes, and the existing figures are untouched by the calls above
  assert torch.equal(te.model(xd, te.opt, mode='get_rate_map')['map'], rm['map'])
  assert torch.equal(te.model(xd, te.opt, mode='get_class_rates')['bits'], cr['bits'])
  assert te.get_coded(xd) == payloads


def test_trainer_class_rows_line_up_with_the_per_class_distortion(golden):
  """get_class_rates' pixels against the per-class pixel counts of get_eval_metrics(per_class=True), same trainer.  The
  fixture's own batch is 64 x 128 and get_eval_metrics refuses anything below 176 on the shorter side (five MS-SSIM scales), so
  this one comparison runs on a synthetic batch of the smallest size both take, 176 x 192 (multiples of the encoder's factor
  16); the golden batch's pixel counts are held against the Python reference in the test above."""
  from oracle.ctu_cpu import model as omodel
  te, _ = golden
  N, H, W = 2, 176, 192
  xd = omodel.synthetic_batch(N, H, W, seed=77)
  cr = te.get_class_rates(xd)
  rm = te.get_rate_map(xd)
  em = te.get_eval_metrics(xd, per_class=True)['per_class']
  per = cr['per_image']
  assert torch.equal(per['pixels'][:, :-1], em['per_image']['pixels']) and torch.equal(cr['pixels'][:-1], em['pixels'])
  assert int(cr['pixels'][-1]) == em['unlabelled'] and int(cr['pixels'].sum()) == N * H * W
  assert int((em['pixels'] > 0).sum()) >= 2                    # a comparison over several classes
  rel = (per['bits'].sum(dim=1) - rm['bits']).abs() / rm['bits']
  assert float(rel.max()) <= 1e-9, rel
  assert torch.equal(rm['map'].sum(dim=(1, 2)), rm['bits']) and torch.equal(rm['per_channel'].sum(dim=1), rm['bits'])
