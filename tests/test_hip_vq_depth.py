"""GPU tests of the residual quantizer with a stage depth per cell (vq_residual.hip, the DEP instantiations; ops.vq_res_rows_fwd /
vq_res_decode / vq_res_bwd with depth=, ops.vq_depth_map).  The contracts are exact unless stated: row m is the
plain call at n_stages = n_m bit for bit (y, index, dx), -1 past the depth, uniform depth S is today's call bit for bit (dbooks
included), the decoder is the forward, second calls repeat the bits, refusals leave the outputs untouched, a hostile map is
clamped.  dbooks under a mixed map is held to hu.RTOL / hu.ETOL of the float64 recursion on the device's own indices.
Shapes (M, L, D, S, G): 257 cells with a ragged last tile and the book in LDS; the book through L2 at DP 32; DP 4 with scalar
loads and an odd G; S at its maximum."""
import ctypes

import numpy as np
import pytest
import torch

import jpdse_hip
from jpdse_hip import ops, F32, BF16
import hip_util as hu
import vq_depth_ref as ref

pytestmark = pytest.mark.gpu
DEV = hu.DEV
CASES = [(4112, 64, 8, 4, 16), (304, 512, 32, 2, 16), (771, 16, 3, 3, 3), (2048, 64, 16, 8, 8)]
MAPS = ('uniform_S', 'uniform_1', 'random', 'tiles', 'in_wave')
_cache = {}


def _tdtype(dtype):
  return torch.bfloat16 if dtype == BF16 else torch.float32


def _sigma(D):
  return 1.0 / D


def _inputs(case, dtype):
  """Seeded x, dy [M, D] in `dtype` and books fp32 [S, L, D] on the device; made once and never modified."""
  key = (case, dtype)
  if key not in _cache:
    M, L, D, S, G = case
    g = torch.Generator().manual_seed(2700 + M + L + 7 * S)
    x = torch.randn(M, D, generator=g).to(_tdtype(dtype))
    books = torch.stack([(torch.rand(L, D, generator=g) * 2 - 1) * 0.5 ** s for s in range(S)])
    dy = torch.randn(M, D, generator=g).to(_tdtype(dtype))
    _cache[key] = (x.to(DEV), books.to(DEV), dy.to(DEV))
  return _cache[key]


def _depth(case, kind):
  """int32 [M / G] on the host.  tiles: the cells of the first 256-vector tile at depth 1, those of the next at S, then alternating
  per tile; in_wave: the depth changes from cell to cell, so inside every wave of 64 vectors."""
  M, L, D, S, G = case
  cells = M // G
  if kind == 'uniform_S':
    d = np.full(cells, S)
  elif kind == 'uniform_1':
    d = np.ones(cells)
  elif kind == 'random':
    d = np.random.RandomState(M + S).randint(1, S + 1, size=cells)
    d[0], d[-1] = S, 1
  elif kind == 'tiles':
    d = np.where((np.arange(cells) * G // 256) % 2 == 0, 1, S)
  else:
    d = 1 + np.arange(cells) % S
  return d.astype(np.int32)


def _plain_by_depth(x, books, S):
  """[(y, index)] of the existing op at n_stages = 1 .. S: computed once per (case, dtype)."""
  key = ('plain', x.data_ptr())
  if key not in _cache:
    _cache[key] = [ops.vq_res_rows_fwd(x, books, n) for n in range(1, S + 1)]
  return _cache[key]


@pytest.mark.parametrize('dtype', hu.DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', CASES, ids=str)
def test_forward_and_decoder_are_the_plain_calls_row_by_row(case, dtype):
  M, L, D, S, G = case
  x, books, _ = _inputs(case, dtype)
  plain = _plain_by_depth(x, books, S)
  for kind in MAPS:
    d = _depth(case, kind)
    dd = torch.from_numpy(d).to(DEV)
    for n in sorted({S, max(1, S - 1)}):
      nm = ref.row_stages(d, G, n, S).to(DEV)
      y, index = ops.vq_res_rows_fwd(x, books, n, depth=dd, groups=G)
      what = (case, kind, n)
      assert y.dtype == x.dtype and tuple(y.shape) == (M, D) and index.dtype == torch.int32 and tuple(index.shape) == (n, M), what
      for v in range(1, n + 1):
        rows = nm == v
        yv, iv = plain[v - 1]
        assert torch.equal(y[rows], yv[rows]), what + (v, 'y')
        assert torch.equal(index[:v][:, rows], iv[:, rows]), what + (v, 'index')
        assert bool((index[v:][:, rows] == -1).all()), what + (v, '-1 past the depth')
      # n_stages below the map's maximum = the map clamped to it
      yc, ic = ops.vq_res_rows_fwd(x, books, n, depth=dd.clamp(max=n), groups=G)
      assert torch.equal(yc, y) and torch.equal(ic, index), what
      # the decoder: the forward's y; garbage past the depth is ignored, and a second call repeats the bits
      dec, status = ops.vq_res_decode(index, books, n, dtype=x.dtype, depth=dd, groups=G)
      assert torch.equal(dec, y) and int(status.item()) == 0, what
      junk = torch.where(index < 0, torch.full_like(index, 1 << 30), index)
      dec2, status2 = ops.vq_res_decode(junk, books, n, dtype=x.dtype, depth=dd, groups=G)
      assert torch.equal(dec2, y) and int(status2.item()) == 0, what
      y2, index2 = ops.vq_res_rows_fwd(x, books, n, depth=dd, groups=G)
      assert torch.equal(y2, y) and torch.equal(index2, index), what
    if kind == 'uniform_S':                                    # today's call, bit for bit
      assert torch.equal(y, plain[S - 1][0]) and torch.equal(index, plain[S - 1][1]), case


@pytest.mark.parametrize('dtype', hu.DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', CASES, ids=str)
def test_decoder_flags_a_bad_index_inside_the_depth(case, dtype):
  M, L, D, S, G = case
  x, books, _ = _inputs(case, dtype)
  d = _depth(case, 'in_wave')
  dd = torch.from_numpy(d).to(DEV)
  y, index = ops.vq_res_rows_fwd(x, books, S, depth=dd, groups=G)
  nm = ref.row_stages(d, G, S, S)
  m = int(torch.nonzero(nm == S)[0])                           # a row that reaches the last stage
  bad = index.clone()
  bad[S - 1, m] = L
  dec, status = ops.vq_res_decode(bad, books, S, dtype=x.dtype, depth=dd, groups=G)
  assert int(status.item()) == 1
  zero = index.clone()
  zero[S - 1, m] = 0                                           # reads as centre 0
  want, _ = ops.vq_res_decode(zero, books, S, dtype=x.dtype, depth=dd, groups=G)
  assert torch.equal(dec, want)


@pytest.mark.parametrize('dtype', hu.DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', CASES, ids=str)
def test_backward_rows_are_the_plain_calls_and_dbooks_matches_fp64(case, dtype):
  M, L, D, S, G = case
  x, books, dy = _inputs(case, dtype)
  sigma = _sigma(D)
  plain = _plain_by_depth(x, books, S)
  plain_dx = [ops.vq_res_bwd(dy, x, books, plain[v - 1][1], sigma, want_dc=False)[0] for v in range(1, S + 1)]
  x64, b64, dy64 = x.double().cpu(), books.double().cpu(), dy.double().cpu()
  for kind in MAPS:
    d = _depth(case, kind)
    dd = torch.from_numpy(d).to(DEV)
    nm = ref.row_stages(d, G, S, S)
    y, index = ops.vq_res_rows_fwd(x, books, S, depth=dd, groups=G)
    dx, dc = ops.vq_res_bwd(dy, x, books, index, sigma, groups=G, depth=dd)
    what = (case, kind)
    assert dx.dtype == x.dtype and dc.dtype == torch.float32 and tuple(dc.shape) == (S, L, D), what
    for v in range(1, S + 1):
      rows = (nm == v).to(DEV)
      assert torch.equal(dx[rows], plain_dx[v - 1][rows]), what + (v, 'dx')
    top = int(nm.max())
    assert not bool(dc[top:].any()), what + ('a book beyond every depth got a gradient',)
    if kind == 'uniform_S':                                    # today's call, bit for bit
      dx0, dc0 = ops.vq_res_bwd(dy, x, books, plain[S - 1][1], sigma)
      assert torch.equal(dx, dx0) and torch.equal(dc, dc0), what
    elif kind == 'uniform_1':
      assert bool(dc[0].any()) and not bool(dc[1:].any()), what
    if kind in ('random', 'tiles', 'in_wave'):
      _, dc64 = ref.bwd(dy64, x64, b64, index.cpu().long(), sigma, nm)
      hu.assert_close(dc.double().cpu(), dc64, hu.RTOL[F32], 'vq_res_bwd(depth) dbooks', detail=kind)
    # either output alone, and a second call: the same bits
    only_dx, none = ops.vq_res_bwd(dy, x, books, index, sigma, want_dc=False, groups=G, depth=dd)
    none2, only_dc = ops.vq_res_bwd(dy, x, books, index, sigma, want_dx=False, groups=G, depth=dd)
    assert none is None and none2 is None and torch.equal(only_dx, dx) and torch.equal(only_dc, dc), what


def test_an_out_of_range_depth_is_clamped():
  case = CASES[0]
  M, L, D, S, G = case
  x, books, dy = _inputs(case, F32)
  d = _depth(case, 'random').astype(np.int64)
  wild = d.copy()
  wild[d == 1] = -5
  wild[d == S] = 1 << 20
  wild[3] = 0
  d[3] = 1
  dd, ww = torch.from_numpy(d.astype(np.int32)).to(DEV), torch.from_numpy(wild.astype(np.int32)).to(DEV)
  y, index = ops.vq_res_rows_fwd(x, books, S, depth=dd, groups=G)
  yw, iw = ops.vq_res_rows_fwd(x, books, S, depth=ww, groups=G)
  assert torch.equal(yw, y) and torch.equal(iw, index)
  dec, status = ops.vq_res_decode(index, books, S, depth=ww, groups=G)
  assert torch.equal(dec, y) and int(status.item()) == 0
  dx, dc = ops.vq_res_bwd(dy, x, books, index, _sigma(D), groups=G, depth=dd)
  dxw, dcw = ops.vq_res_bwd(dy, x, books, index, _sigma(D), groups=G, depth=ww)
  assert torch.equal(dxw, dx) and torch.equal(dcw, dc)


def _refused(call, args, field):
  assert call(ctypes.byref(args)) == -1, field
  assert field in jpdse_hip.last_error(), (field, jpdse_hip.last_error())


def test_refusals_leave_the_outputs_untouched():
  lib = jpdse_hip.lib()
  x, books, dy = _inputs((64, 64, 8, 4, 16), F32)
  depth = torch.ones(4, dtype=torch.int32, device=DEV)
  y, dx = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
  index = torch.full((4, 64), -3, dtype=torch.int32, device=DEV)
  dc = torch.full_like(books, 7.0)
  status = torch.full((1,), 5, dtype=torch.int32, device=DEV)

  def fwd(G=16, dp=depth.data_ptr(), **kw):
    v = dict(dtype=F32, M=64, D=8, L=64, S=4, n_stages=4, x=x.data_ptr(), books=books.data_ptr(), y=y.data_ptr(),
             index=index.data_ptr(), stream=None)
    v.update(kw)
    return jpdse_hip.VqResRowsFwdDepthArgs(jpdse_hip.VqResRowsFwdArgs(**v), G, dp)

  def dec(G=16, dp=depth.data_ptr(), **kw):
    v = dict(dtype=F32, M=64, D=8, L=64, S=4, n_stages=4, index=index.data_ptr(), books=books.data_ptr(), y=y.data_ptr(),
             status=status.data_ptr(), stream=None)
    v.update(kw)
    return jpdse_hip.VqResDecodeDepthArgs(jpdse_hip.VqResDecodeArgs(**v), G, dp)

  def bwd(G=16, dp=depth.data_ptr(), **kw):
    v = dict(dtype=F32, M=64, D=8, L=64, S=4, n_stages=4, sigma=0.125, dy=dy.data_ptr(), x=x.data_ptr(), books=books.data_ptr(),
             index=index.data_ptr(), dx=dx.data_ptr(), dbooks=dc.data_ptr(), ws=None, ws_bytes=0, stream=None)
    v.update(kw)
    return jpdse_hip.VqResBwdDepthArgs(jpdse_hip.VqResBwdArgs(**v), G, dp)

  for make, call in ((fwd, lib.jpdse_vq_res_rows_fwd_depth), (dec, lib.jpdse_vq_res_decode_depth), (bwd, lib.jpdse_vq_res_bwd_depth)):
    _refused(call, make(n_stages=0), 'n_stages = 0')
    _refused(call, make(n_stages=5), 'n_stages = 5')
    _refused(call, make(D=33), 'center_size D = 33')
    _refused(call, make(G=0), 'G = 0 vectors per cell')
    _refused(call, make(G=5), 'G = 5 does not divide M = 64')
    _refused(call, make(dp=None), 'null pointer (depth)')
    _refused(call, make(books=None), 'null pointer')
  _refused(lib.jpdse_vq_res_bwd_depth, bwd(), 'workspace too small')
  torch.cuda.synchronize()
  assert bool((y == 7.0).all()) and bool((dx == 7.0).all()) and bool((dc == 7.0).all()) and bool((index == -3).all()) and \
      int(status.item()) == 5, 'a refused call wrote its outputs'
  with pytest.raises(ValueError, match='groups must divide the 64 vectors'):
    ops.vq_res_rows_fwd(x, books, depth=depth, groups=5)
  with pytest.raises(ValueError, match='depth must be a contiguous int32 tensor of 4 cells'):
    ops.vq_res_rows_fwd(x, books, depth=depth.long(), groups=16)
  with pytest.raises(ValueError, match='depth and dhist cannot be combined'):
    ops.vq_res_bwd(dy, x, books, index, 0.125, groups=16, depth=depth, dhist=torch.zeros(4, 16, 64, device=DEV))


def _labels(N, H, W, seed, n_classes):
  rs = np.random.RandomState(seed)
  lab = rs.randint(0, n_classes + 4, size=(N, 1, H, W)).astype(np.float32)      # some classes outside the table
  lab[rs.rand(N, 1, H, W) < 0.02] = -1.0
  lab[rs.rand(N, 1, H, W) < 0.02] = 2.5
  lab[0, 0, 0, 0] = float('nan')
  return lab


@pytest.mark.parametrize('shape', [(1, 8, 16, 4), (2, 64, 32, 4), (2, 64, 32, 1), (1, 8, 16, 8)], ids=str)
def test_depth_map_equals_the_numpy_rule(shape):
  N, H, W, step = shape
  n_classes = 6
  table = np.array([3, 1, 2, 1, 3, 2], dtype=np.int32)
  lab = _labels(N, H, W, 31 + H, n_classes)
  if (H, W) == (8, 16):                                        # hand-placed: a cell of one class, a cell lifted by one pixel
    lab[0, 0, :4, :4] = 1
    lab[0, 0, :4, 4:8] = 1
    lab[0, 0, 3, 7] = 0
    lab[0, 0, 4:, 8:12] = 9                                    # outside the table: the default
  for default in (1, 3):
    got = ops.vq_depth_map(torch.from_numpy(lab).to(DEV), torch.from_numpy(table).to(DEV), default, step)
    want = ref.depth_map(lab, table, default, step)
    assert got.dtype == torch.int32 and tuple(got.shape) == (N, H // step, W // step)
    assert np.array_equal(got.cpu().numpy(), want), (shape, default)
  if (H, W, step) == (8, 16, 4):
    assert want[0, 0, 0] == 1 and want[0, 0, 1] == 3 and want[0, 1, 2] == 3
  # an empty table: the default everywhere
  got = ops.vq_depth_map(torch.from_numpy(lab).to(DEV), torch.zeros(0, dtype=torch.int32, device=DEV), 2, step)
  assert bool((got == 2).all())
  with pytest.raises(ValueError, match='step must divide'):
    ops.vq_depth_map(torch.from_numpy(lab).to(DEV), torch.from_numpy(table).to(DEV), 1, 3)


@pytest.mark.parametrize('dtype', hu.DTYPES, ids=['fp32', 'bf16'])
def test_module_and_stream_round_trip(dtype):
  """ResidualS2HVQ with depth= / groups=: quantize's y is decode's, the gradients are the ops', and the .jpdm stream and its
  truncations decode to the forward at min(depth, n')."""
  from ctu.quantizers import ResidualS2HVQ
  from ctu.utils import vqdepth
  case = (4112, 64, 8, 4, 16)
  M, L, D, S, G = case
  x, books, dy = _inputs(case, dtype)
  d = _depth(case, 'random')
  dd = torch.from_numpy(d).to(DEV)
  rvq = ResidualS2HVQ(books.clone(), sigma=_sigma(D)).to(DEV)
  rvq.train()
  xin = x.clone().view(M // 2, 2 * D).requires_grad_(True)      # code_len 2
  y, code = rvq.quantize(xin, 2, depth=dd, groups=G)
  want_y, want_index = ops.vq_res_rows_fwd(x, books, S, depth=dd, groups=G)
  assert torch.equal(y.detach().view(M, D), want_y) and torch.equal(code.view(S, M), want_index.long())
  y.backward(dy.view_as(y))
  dx, dc = ops.vq_res_bwd(dy, x, books, want_index, _sigma(D), groups=G, depth=dd)
  assert torch.equal(xin.grad.view(M, D), dx) and torch.equal(rvq.code_books.grad, dc)
  rvq.eval()
  assert torch.equal(rvq.encode(xin.detach(), 2, depth=dd, groups=G), code)
  if dtype == F32:                                             # decode gives float32: the forward's bits where x is float32
    assert torch.equal(rvq.decode(code, depth=dd, groups=G).view(M, D), want_y)
  blob = vqdepth.write_depth_stages(None, code, d, L, groups=G)
  counts = vqdepth.stage_counts(d, S)
  assert vqdepth.parse_depth_stages(blob, depth=d)[4] == counts and sum(counts) == int(d.sum())
  back = vqdepth.read_depth_stages(blob, d, DEV)
  assert torch.equal(back, code)
  for keep in (1, 2):
    cut = vqdepth.truncate_depth_stages(blob, keep)
    part = vqdepth.read_depth_stages(cut, d, DEV)
    assert torch.equal(part, code[:keep])
    if dtype == F32:
      got = vqdepth.reconstruct_depth_stages(rvq, cut, d)
      assert torch.equal(got.view(M, D), ops.vq_res_rows_fwd(x, books, keep, depth=dd, groups=G)[0])
  other = d.copy()
  other[other == 1] = 2
  with pytest.raises(ValueError, match='the depth map implies'):
    vqdepth.read_depth_stages(blob, other, DEV)


@pytest.mark.parametrize('dtype', hu.DTYPES, ids=['fp32', 'bf16'])
def test_layer_with_a_depth_is_the_composed_chain(dtype):
  """HipResidualVQBottleneck.depth: fwd, code, decode and bwd hand the map to the depth calls with groups = cout / center_size;
  unset, every call is the one it was."""
  from jpdse_hip.layers import HipResidualVQBottleneck
  from jpdse_hip.ops import Act
  N, C, L, D, S = 2, 16, 8, 4, 3
  torch.manual_seed(5)
  layer = HipResidualVQBottleneck(32, C, L, D, S, sigma=1.0 / D, dtype=dtype, device=DEV)
  g = torch.Generator().manual_seed(5)
  x = ops.nchw_to_nhwc((4.0 * torch.randn(N, 32, 16, 32, generator=g)).to(DEV), dtype)
  dy = ops.nchw_to_nhwc(torch.randn(N, C, 16, 32, generator=g).to(DEV), dtype)
  layer.train()
  layer.ensure_grads()
  G = layer.groups
  books = layer.vq._code_books.detach().clone()
  h, c_conv = layer.conv.fwd(x)
  hm = h.t.view(-1, D)
  depth = torch.from_numpy((1 + np.arange(N * 16 * 32) % S).astype(np.int32)).to(DEV)
  plain_y, plain_ctx = layer.fwd(x)
  layer.depth = depth
  y, ctx = layer.fwd(x)
  want_y, want_index = ops.vq_res_rows_fwd(hm, books, S, depth=depth, groups=G)
  assert torch.equal(y.t, want_y.view(h.t.shape)) and torch.equal(ctx.items[2], want_index) and not torch.equal(y.t, plain_y.t)
  code = layer.code(x)
  assert torch.equal(code, want_index.view(S, N, -1).transpose(0, 1)) and bool((code == -1).any())
  back, status = layer.decode(code, N, h.H, h.W, dtype)
  assert torch.equal(back.t, y.t) and int(status.item()) == 0
  two, _ = layer.decode(code[:, :2].contiguous(), N, h.H, h.W, dtype)              # a code prefix: min(depth, 2)
  assert torch.equal(two.t, ops.vq_res_rows_fwd(hm, books, 2, depth=depth, groups=G)[0].view(h.t.shape))
  dx = layer.bwd(ctx, dy)
  got_dc, got_dw = layer.vq._code_books.grad.clone(), layer.conv.weight.grad.clone()
  dh, dc = ops.vq_res_bwd(dy.t.view(-1, D), hm, books, want_index, 1.0 / D, groups=G, depth=depth)
  want_dx = layer.conv.bwd(c_conv, Act(dh.view(h.t.shape), h.C), True, True)
  assert torch.equal(dx.t, want_dx.t) and torch.equal(got_dc, dc) and torch.equal(got_dw, layer.conv.weight.grad)
  layer.rate_scale, layer.rate_denom = 1.0, 64.0
  with pytest.raises(ValueError, match='depth and rate_scale cannot be combined'):
    layer.fwd(x)
  layer.rate_scale = None
  layer.depth = None                                           # unset: the call it was
  again, ctx2 = layer.fwd(x)
  assert torch.equal(again.t, plain_y.t) and len(ctx2.items) == 3 and torch.equal(ctx2.items[2], plain_ctx.items[2])
