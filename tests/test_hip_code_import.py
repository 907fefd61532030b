"""GPU: jpdse_code_import (ops.code_import), the receiver's half of the learned codec's bitstream, against the numpy
restatement tests/code_import_ref.py.  The kernel moves bits: every comparison is exact."""
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

import code_import_ref as cref  # noqa: E402
from jpdse_hip import F32, BF16, ops  # noqa: E402

# (N, H, W, C): one element; H*W odd (channels start inside a byte) with one padded lane group; CPAD 16 and bits % 8 != 0;
# the golden fixture's code; 16 lane groups per pixel
SHAPES = [(1, 1, 1, 1), (2, 3, 5, 3), (1, 5, 7, 9), (2, 4, 8, 32), (3, 2, 2, 128)]
DTYPES = [F32, BF16]
_ids = dict(argnames='shape', argvalues=SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))


def _random_b(shape, seed, zeros=False):
  N, H, W, C = shape
  g = np.random.default_rng(seed)
  b = np.where(g.random((N, C, H, W)) < 0.5, -1.0, 1.0).astype(np.float32)
  if zeros:
    b[g.random(b.shape) < 0.25] = 0.0
    b.reshape(-1)[0] = 0.0
  return b


def _import(code, shape, dtype):
  """ops.code_import into a buffer pre-filled with 7.0: (stored tensor as float32 numpy [N, H, W, CPAD(C)], the Act)."""
  N, H, W, C = shape
  out = ops.Act.empty(N, H, W, C, dtype, torch.device('cuda', 0))
  out.t.fill_(7.0)
  b = ops.code_import(torch.as_tensor(code).cuda(), N, H, W, C, dtype, out=out)
  assert b is out and b.dtype == dtype and tuple(b.t.shape) == (N, H, W, cref.cpad(C))
  return b.t.float().cpu().numpy(), b


def _check_lanes(stored, C):
  assert np.all(stored[..., C:] == 0), 'a padding lane is not 0'
  assert np.all(np.abs(stored[..., :C]) == 1), 'a logical lane is neither +1 nor -1'


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('packed', [True, False], ids=['packed', 'fp32code'])
@pytest.mark.parametrize(**_ids)
def test_import_matches_the_numpy_restatement(shape, packed, dtype):
  N, H, W, C = shape
  b = _random_b(shape, seed=sum(shape))
  if packed:
    code = cref.export_packed(b)
    want = cref.import_packed(code, N, C, H, W)
  else:
    code = cref.export_float(b)
    want = cref.import_float(code, N, C, H, W)
  assert np.array_equal(want, b)                      # the yardstick inverts itself on a code without zeros
  stored, act = _import(code, shape, dtype)
  _check_lanes(stored, C)
  assert torch.equal(torch.from_numpy(stored), torch.from_numpy(cref.to_nhwc(want)))
  assert torch.equal(ops.nhwc_to_nchw(act).cpu(), torch.from_numpy(want))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize(**_ids)
def test_unused_trailing_bits_are_ignored_and_images_start_on_a_byte(shape, dtype):
  N, H, W, C = shape
  bits = C * H * W
  b = _random_b(shape, seed=7 + sum(shape))
  b[:, -1, -1, -1] = -1.0                             # the last real bit of every image is 0, right in front of the filler
  clean = cref.export_packed(b)
  dirty = clean.copy()
  unused = (-bits) % 8
  dirty[:, -1] |= (1 << unused) - 1                   # every unused low bit of each image's last byte set
  if unused:
    assert not np.array_equal(dirty, clean)
  want = cref.to_nhwc(cref.import_packed(clean, N, C, H, W))
  for code in (clean, dirty):
    stored, _ = _import(code, shape, dtype)
    assert torch.equal(torch.from_numpy(stored), torch.from_numpy(want))
  if N > 1:
    # image 1 read from its own first byte, not from the tail of image 0: all-ones image 0, all-zero image 1
    code = np.zeros_like(clean)
    code[0] = 0xff
    stored, _ = _import(code, shape, dtype)
    assert np.all(stored[0, ..., :C] == 1) and np.all(stored[1:, ..., :C] == -1)
    _check_lanes(stored, C)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('packed', [True, False], ids=['packed', 'fp32code'])
@pytest.mark.parametrize(**_ids)
def test_import_inverts_export_and_a_zero_comes_back_as_minus_one(shape, packed, dtype):
  N, H, W, C = shape
  dev = torch.device('cuda', 0)
  for zeros in (False, True):
    b = _random_b(shape, seed=11 + sum(shape), zeros=zeros)
    act = ops.nchw_to_nhwc(torch.from_numpy(b).to(dev), dtype)
    code = ops.code_export(act, packed=packed)
    ref = cref.export_packed(b) if packed else cref.export_float(b)
    assert np.array_equal(code.cpu().numpy(), ref)
    back = ops.code_import(code, N, H, W, C, dtype)
    want = np.where(b == 0, np.float32(-1), b)        # the zero rule: stored as a 0 bit (or 0.5), decoded as -1
    assert zeros == bool((b == 0).any())
    assert torch.equal(ops.nhwc_to_nchw(back).cpu(), torch.from_numpy(want))
    if not zeros:
      assert torch.equal(back.t, act.t)               # the stored tensors, padding lanes included
    assert int(ops.code_stats(back)[:, 1].sum()) == 0


@pytest.mark.parametrize('dtype', DTYPES)
def test_fp32_code_threshold_and_nan(dtype):
  vals = np.array([0.5, 0.50001, -3.0, np.nan, 1.0], dtype=np.float32)
  want = [-1.0, 1.0, -1.0, -1.0, 1.0]
  # as five channels of one pixel, and as five pixels of one channel
  for shape in ((1, 1, 1, 5), (1, 1, 5, 1)):
    stored, act = _import(vals[None], shape, dtype)
    assert ops.nhwc_to_nchw(act).cpu().reshape(-1).tolist() == want
    assert cref.import_float(vals[None], 1, shape[3], shape[1], shape[2]).reshape(-1).tolist() == want
    _check_lanes(stored, shape[3])
