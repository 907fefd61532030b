"""GPU tests of the thread-per-vector residual forward (vq_residual.hip: vqres_rows_fwd_kernel; ops.vq_res_rows_fwd; DESIGN.md
4.24).  The contract is bit equality with the group-layout kernel ops.vq_res_fwd on `index` and `y`, for every tail of M (fewer
than one wave, one tile plus one, a ragged last tile under the barrier of the stage loop), every row layout (padded DP, the
non-vector loads, a book in LDS and a book read through L2), every stage count and prefix, fp32 and bf16."""
import ctypes

import pytest
import torch

import jpdse_hip
from jpdse_hip import ops, F32, BF16
import hip_util as hu

pytestmark = pytest.mark.gpu
DEV = hu.DEV
MS = (1, 63, 64, 255, 257, 1000)
SHAPES = [(1, 2), (3, 5), (8, 64), (5, 64), (16, 200), (32, 512)]     # (D, L)
STAGES = (1, 4, 8)
_cache = {}


def _tdtype(dtype):
  return torch.bfloat16 if dtype == BF16 else torch.float32


def _inputs(M, D, L, S, dtype):
  """Seeded x [M, D] in `dtype` and books fp32 [S, L, D] scaled 0.5 ** s, on the device; made once and never modified."""
  key = (M, D, L, S, dtype)
  if key not in _cache:
    g = torch.Generator().manual_seed(2400 + M + 3 * D + 5 * L + 7 * S)
    x = torch.randn(M, D, generator=g).to(_tdtype(dtype))
    books = torch.stack([torch.randn(L, D, generator=g) * 0.5 ** s for s in range(S)])
    _cache[key] = (x.to(DEV), books.to(DEV))
  return _cache[key]


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_rows_forward_is_the_group_kernel_bit_for_bit(shape, dtype):
  D, L = shape
  for M in MS:
    for S in STAGES:
      x, books = _inputs(M, D, L, S, dtype)
      for n in range(1, S + 1):
        want_y, want_index, _, _ = ops.vq_res_fwd(x, books, n_stages=n)
        y, index = ops.vq_res_rows_fwd(x, books, n_stages=n)
        what = (M, D, L, S, n)
        assert y.dtype == x.dtype and tuple(y.shape) == (M, D) and index.dtype == torch.int32 and tuple(index.shape) == (n, M), what
        assert torch.equal(index, want_index), what
        assert torch.equal(y, want_y), what
        dec, status = ops.vq_res_decode(index, books, dtype=x.dtype)
        assert torch.equal(dec, y) and int(status.item()) == 0, what
      y_all, index_all = ops.vq_res_rows_fwd(x, books)                   # the default: all stages; a second call: the same bits
      assert torch.equal(y_all, y) and torch.equal(index_all, index), (M, D, L, S)


def test_unaligned_bf16_rows_take_the_scalar_loads():
  M, D, L, S = 257, 8, 64, 4
  x, books = _inputs(M, D, L, S, BF16)
  buf = torch.empty(M * D + 4, dtype=torch.bfloat16, device=DEV)
  view = buf[4:].view(M, D)                                                # 8 bytes past a 16-byte boundary
  view.copy_(x)
  assert view.data_ptr() % 16 == 8 and view.is_contiguous()
  want_y, want_index = ops.vq_res_rows_fwd(x, books)
  y, index = ops.vq_res_rows_fwd(view, books)
  ref_y, ref_index, _, _ = ops.vq_res_fwd(view, books)
  assert torch.equal(index, want_index) and torch.equal(y, want_y)
  assert torch.equal(index, ref_index) and torch.equal(y, ref_y)


@pytest.mark.parametrize('shape', [(8, 64), (32, 512)], ids=str)
def test_a_tie_goes_to_the_lower_index(shape):
  D, L = shape
  x, books = _inputs(63, D, L, 4, F32)
  books = books.clone()
  books[0, 5] = books[0, 2]                                                # two identical centres in the first book
  books[1, L - 1] = books[1, 0]
  x = x.clone()
  x[:10] = books[0, 2]                                                     # score 0 against centres 2 and 5 alike
  y, index = ops.vq_res_rows_fwd(x, books)
  want_y, want_index, _, _ = ops.vq_res_fwd(x, books)
  assert torch.equal(index, want_index) and torch.equal(y, want_y)
  assert index[0, :10].cpu().tolist() == [2] * 10
  assert not bool((index[0] == 5).any()) and not bool((index[1] == L - 1).any())


def _refused(call, args, field):
  assert call(ctypes.byref(args)) == -1, field
  assert field in jpdse_hip.last_error(), (field, jpdse_hip.last_error())


def test_bad_shapes_are_refused_before_a_launch():
  lib = jpdse_hip.lib()
  x, books = _inputs(64, 8, 64, 4, F32)
  y = torch.full_like(x, 7.0)
  index = torch.full((4, 64), -3, dtype=torch.int32, device=DEV)

  def args(**kw):
    v = dict(dtype=F32, M=64, D=8, L=64, S=4, n_stages=4, x=x.data_ptr(), books=books.data_ptr(), y=y.data_ptr(),
             index=index.data_ptr(), stream=None)
    v.update(kw)
    return jpdse_hip.VqResRowsFwdArgs(**v)

  _refused(lib.jpdse_vq_res_rows_fwd, args(n_stages=0), 'n_stages = 0')
  _refused(lib.jpdse_vq_res_rows_fwd, args(n_stages=5), 'n_stages = 5')
  _refused(lib.jpdse_vq_res_rows_fwd, args(S=9, n_stages=9), 'S = 9 stages')
  _refused(lib.jpdse_vq_res_rows_fwd, args(D=33), 'center_size D = 33')
  _refused(lib.jpdse_vq_res_rows_fwd, args(L=1), 'n_center L = 1')
  _refused(lib.jpdse_vq_res_rows_fwd, args(x=None), 'null pointer')
  torch.cuda.synchronize()
  assert bool((y == 7.0).all()) and bool((index == -3).all()), 'a refused call wrote its outputs'
  with pytest.raises(ValueError, match='n_stages must be in 1 .. 4'):
    ops.vq_res_rows_fwd(x, books, n_stages=0)
