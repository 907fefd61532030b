"""Host-only checks of the stage depth per cell: the restated per-row recursion against float64 autograd of the
surrogate, the depth-map rule, every refusal of the four C entry points by field name (never-dereferenced pointers), and the .jpdm
container (ctu.utils.vqdepth) on hand-made inner blobs: build / parse / truncate round trips, every header refusal, and the older
readers refusing the new magic.  Nothing here launches a kernel."""
import ctypes
import os
import struct

import numpy as np
import pytest
import torch

import jpdse_hip
from jpdse_hip import F32
from ctu.utils import vqdepth, vqstages, vqstream
import vq_depth_ref as ref
import vq_residual_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the mathematics -------------------------------------------------------------------------------------------------------------
def _draw(M, L, D, S, seed):
  g = torch.Generator().manual_seed(seed)
  x = torch.randn(M, D, generator=g, dtype=torch.float64)
  books = torch.rand(S, L, D, generator=g, dtype=torch.float64) * 2 - 1
  dy = torch.randn(M, D, generator=g, dtype=torch.float64)
  return x, books, dy


@pytest.mark.parametrize('case', [(24, 5, 3, 3, 4), (30, 7, 2, 4, 3), (16, 4, 4, 2, 2), (12, 6, 1, 5, 1)], ids=str)
def test_per_row_recursion_equals_fp64_autograd(case):
  M, L, D, S, G = case
  x, books, dy = _draw(M, L, D, S, 700 + M + L)
  sigma = 1.0 / D
  depth = torch.randint(1, S + 1, (M // G,), generator=torch.Generator().manual_seed(M)).numpy()
  depth[0], depth[-1] = 1, S                                  # both ends of the range are there
  for n in (S, max(1, S - 1)):
    nm = ref.row_stages(depth, G, n, S)
    assert tuple(nm.shape) == (M,) and int(nm.max()) == n and int(nm.min()) == 1
    y, index, _ = ref.forward(x, books, nm)
    assert tuple(index.shape) == (n, M)
    for s in range(n):
      assert bool(((index[s] == -1) == (nm <= s)).all())
    # row m is the plain forward at n_stages = n_m
    for v in range(1, n + 1):
      yv, iv = vq_residual_ref.forward(x, books, v)[:2]
      assert torch.equal(y[nm == v], yv[nm == v]) and torch.equal(index[:v][:, nm == v], iv[:, nm == v])
    dx, dbooks = ref.bwd(dy, x, books, index, sigma, nm)
    dx_auto, dbooks_auto = ref.grads(dy, x, books, sigma, nm)
    assert torch.allclose(dx, dx_auto, rtol=1e-9, atol=1e-12)
    assert torch.allclose(dbooks, dbooks_auto[:n], rtol=1e-9, atol=1e-12) and not bool(dbooks_auto[n:].any())
    # a row's dx is the plain recursion's at its own depth
    for v in range(1, n + 1):
      dxv = vq_residual_ref.grads(dy, x, books, sigma, v)[0]
      assert torch.allclose(dx[nm == v], dxv[nm == v], rtol=1e-9, atol=1e-12)
  # uniform depth: the plain quantizer
  nm = ref.row_stages(np.full(M // G, S), G, S, S)
  dx, dbooks = ref.bwd(dy, x, books, ref.forward(x, books, nm)[1], sigma, nm)
  dx0, dbooks0 = vq_residual_ref.grads(dy, x, books, sigma)
  assert torch.allclose(dx, dx0, rtol=1e-9, atol=1e-12) and torch.allclose(dbooks, dbooks0, rtol=1e-9, atol=1e-12)


def test_a_stage_no_row_reaches_gets_zeros():
  x, books, dy = _draw(12, 4, 2, 3, 5)
  nm = ref.row_stages(np.array([1, 2, 1, 2]), 3, 3, 3)
  index = ref.forward(x, books, nm)[1]
  assert tuple(index.shape) == (2, 12)
  _, dbooks = ref.bwd(dy, x, books, torch.cat([index, torch.full((1, 12), -1)]), 0.5, nm)
  assert bool(dbooks[:2].any()) and not bool(dbooks[2].any())


def test_depth_map_rule():
  table = [3, 1, 2]
  lab = np.zeros((1, 1, 4, 8), dtype=np.float32)
  lab[0, 0, :, :] = 1                                         # class 1 -> 1
  lab[0, 0, 0, 0] = 0                                         # one pixel of class 0 -> 3 lifts its cell
  lab[0, 0, 2, 2] = 7                                         # outside the table -> default
  lab[0, 0, 3, 4] = 1.5                                       # no integer -> default
  lab[0, 0, 2, 6] = float('nan')
  lab[0, 0, 1, 7] = -1
  got = ref.depth_map(lab, table, 2, 2)
  assert got.tolist() == [[[3, 1, 1, 2], [1, 2, 2, 2]]]
  assert ref.depth_map(lab, [], 5, 4).tolist() == [[[5, 5]]]
  assert ref.depth_map(lab, table, 2, 1)[0, 0, :2].tolist() == [3, 1]


# ---- the library -------------------------------------------------------------------------------------------------------------------
P = 0x1000      # never dereferenced: every call below is refused first


def _plain(kind, **kw):
  v = dict(dtype=F32, M=64, D=8, L=64, S=4, n_stages=4, stream=None)
  if kind == 'fwd':
    v.update(x=P, books=P, y=P, index=P)
    cls = jpdse_hip.VqResRowsFwdArgs
  elif kind == 'dec':
    v.update(index=P, books=P, y=P, status=P)
    cls = jpdse_hip.VqResDecodeArgs
  else:
    v.update(sigma=0.125, dy=P, x=P, books=P, index=P, dx=P, dbooks=None, ws=None, ws_bytes=0)
    cls = jpdse_hip.VqResBwdArgs
  v.update(kw)
  return cls(**v)


CALLS = {'fwd': ('jpdse_vq_res_rows_fwd_depth', jpdse_hip.VqResRowsFwdDepthArgs, 'x'),
         'dec': ('jpdse_vq_res_decode_depth', jpdse_hip.VqResDecodeDepthArgs, 'index'),
         'bwd': ('jpdse_vq_res_bwd_depth', jpdse_hip.VqResBwdDepthArgs, 'dy')}
COMMON_REFUSALS = [
    (dict(dtype=7), 'bad dtype'), (dict(M=0), 'M = 0'), (dict(D=33), 'center_size D = 33'), (dict(D=0), 'center_size D = 0'),
    (dict(L=1), 'n_center L = 1'), (dict(L=513), 'n_center L = 513'), (dict(M=1 << 23, L=512), 'M * L'),
    (dict(S=9), 'S = 9 stages'), (dict(S=0), 'S = 0 stages'), (dict(n_stages=0), 'n_stages = 0'), (dict(n_stages=5), 'n_stages = 5'),
    (dict(G=0), 'G = 0 vectors per cell'), (dict(G=-2), 'G = -2 vectors per cell'), (dict(G=5), 'G = 5 does not divide M = 64'),
    (dict(depth=None), 'null pointer (depth)'), (dict(books=None), 'null pointer'),
]


@pytest.mark.parametrize('kind', sorted(CALLS))
@pytest.mark.parametrize('over,field', COMMON_REFUSALS, ids=[str(o) for o, _ in COMMON_REFUSALS])
def test_depth_calls_refuse_on_the_host_by_field(kind, over, field):
  name, cls, first = CALLS[kind]
  lib = jpdse_hip.lib()
  assert name in jpdse_hip.SIGNATURES
  over = dict(over)
  G, depth = over.pop('G', 16), over.pop('depth', P)
  call = getattr(lib, name)
  assert call(ctypes.byref(cls(_plain(kind, **over), G, depth))) == -1, field
  assert field in jpdse_hip.last_error() and name[len('jpdse_'):] in jpdse_hip.last_error(), (field, jpdse_hip.last_error())
  assert call(ctypes.byref(cls(_plain(kind, **{first: None}), 16, P))) == -1 and 'null pointer' in jpdse_hip.last_error()


def test_backward_refuses_sigma_and_workspace():
  lib = jpdse_hip.lib()
  for over, field in ((dict(sigma=0.0), 'sigma is 0'), (dict(sigma=float('nan')), 'sigma is nan'), (dict(dbooks=P), 'workspace too small'),
                      (dict(dbooks=P, ws=P, ws_bytes=16), 'workspace too small')):
    args = jpdse_hip.VqResBwdDepthArgs(_plain('bwd', **over), 16, P)
    assert lib.jpdse_vq_res_bwd_depth(ctypes.byref(args)) == -1, field
    assert field in jpdse_hip.last_error() and 'vq_res_bwd_depth' in jpdse_hip.last_error(), (field, jpdse_hip.last_error())


MAP_REFUSALS = [
    (dict(N=0), 'N, H, W = 0, 8, 16'), (dict(H=0), 'N, H, W = 2, 0, 16'), (dict(W=-1), 'N, H, W = 2, 8, -1'),
    (dict(step=0), 'step = 0'), (dict(step=3), 'step = 3 does not divide H = 8 and W = 16'), (dict(step=16), 'step = 16 does not divide'),
    (dict(N=1 << 12, H=1 << 10, W=1 << 10, step=4), 'N * H * W'), (dict(n_classes=-1), 'n_classes = -1'),
    (dict(n_classes=65537), 'n_classes = 65537'), (dict(label=None), 'null pointer'), (dict(depth=None), 'null pointer'),
    (dict(table=None), 'null pointer'),
]


@pytest.mark.parametrize('over,field', MAP_REFUSALS, ids=[str(o) for o, _ in MAP_REFUSALS])
def test_depth_map_refuses_on_the_host_by_field(over, field):
  v = dict(N=2, H=8, W=16, step=4, n_classes=35, default_depth=1, label=P, table=P, depth=P, stream=None)
  v.update(over)
  lib = jpdse_hip.lib()
  assert lib.jpdse_vq_depth_map(ctypes.byref(jpdse_hip.VqDepthMapArgs(**v))) == -1, field
  assert field in jpdse_hip.last_error() and 'vq_depth_map' in jpdse_hip.last_error(), (field, jpdse_hip.last_error())


def test_null_structs_the_abi_version_and_the_struct_layouts():
  lib = jpdse_hip.lib()
  assert lib.jpdse_version() == 2
  header = open(os.path.join(ROOT, 'include', 'jpdse.h')).read()
  dev = ctypes.CDLL(jpdse_hip.DEV_LIB_PATH)
  for name in ('jpdse_vq_res_rows_fwd_depth', 'jpdse_vq_res_decode_depth', 'jpdse_vq_res_bwd_depth', 'jpdse_vq_depth_map'):
    assert getattr(lib, name)(None) == -1 and 'null argument struct' in jpdse_hip.last_error(), name
    assert 'int %s(const %s_args* args);' % (name, name) in header, name
    assert name in jpdse_hip.SIGNATURES and hasattr(dev, name), name
  for cls, inner in ((jpdse_hip.VqResRowsFwdDepthArgs, jpdse_hip.VqResRowsFwdArgs), (jpdse_hip.VqResDecodeDepthArgs, jpdse_hip.VqResDecodeArgs),
                     (jpdse_hip.VqResBwdDepthArgs, jpdse_hip.VqResBwdArgs)):
    assert ctypes.sizeof(cls) == ctypes.sizeof(inner) + 16 and cls._fields_[0][1] is inner and getattr(cls, cls._fields_[0][0]).offset == 0
  assert 'DESIGN.md 4.27' in header


# ---- the container -----------------------------------------------------------------------------------------------------------------
def _inner(count, G, L, seed):
  """A packed (mode 0) .jpdv blob of a (count, G) code, made on the host: (blob, indices)."""
  idx = np.random.RandomState(seed).randint(0, L, size=count * G)
  nb = vqstream.index_bits(L)
  blob = vqstream._HEADER.pack(vqstream.MAGIC, vqstream.VERSION, count, G, L, 0, vqstream.MODE_PACKED) + vqstream.pack_indices(idx, nb)
  assert vqstream.parse_blob(blob)[:3] == (count, G, L)
  return blob, idx


DEPTH = np.array([3, 1, 2, 3, 1, 1], dtype=np.int64)          # 6 cells: counts 6, 3, 2
G_, L_ = 4, 16


def _file():
  counts = vqdepth.stage_counts(DEPTH, 3)
  assert counts == [6, 3, 2]
  inners = [_inner(c, G_, L_, 10 + s) for s, c in enumerate(counts)]
  blob = vqdepth.build_depth_stages([b for b, _ in inners], counts, 2, 12, L_)      # 2 rows of 12 indices = 6 cells of 4
  return blob, counts, inners


def test_build_parse_truncate_round_trip():
  blob, counts, inners = _file()
  assert blob[:4] == b'JPDM' and vqdepth.SUFFIX == '.jpdm' and vqdepth.VERSION == 1
  assert len(blob) == 24 + 8 * 3 + sum(len(b) for b, _ in inners) and vqdepth.coded_bits(blob) == 8 * len(blob)
  S, n, code_len, L, got_counts, blobs = vqdepth.parse_depth_stages(blob, depth=DEPTH)
  assert (S, n, code_len, L, got_counts) == (3, 2, 12, L_, counts) and blobs == [b for b, _ in inners]
  assert vqdepth.parse_depth_stages(blob)[4] == counts                            # without a map: the header's own checks
  for keep in (1, 2, 3):
    cut = vqdepth.truncate_depth_stages(blob, keep)
    S2, n2, c2, L2, counts2, blobs2 = vqdepth.parse_depth_stages(cut, depth=DEPTH)  # the same map: min(depth, keep)
    assert (S2, n2, c2, L2) == (keep, 2, 12, L_) and counts2 == counts[:keep] and blobs2 == blobs[:keep]
    assert vqdepth.coded_bits(blob, keep) == 8 * len(cut) == 8 * (24 + 8 * keep + sum(len(b) for b in blobs[:keep]))
    assert vqdepth.truncate_depth_stages(cut, keep) == cut
  assert vqdepth.truncate_depth_stages(blob, 3) == blob
  # a stage without a cell: length 0, no blob
  d1 = np.ones(6, dtype=np.int64)
  one = vqdepth.build_depth_stages([inners[0][0], b'', b''], [6, 0, 0], 2, 12, L_)
  assert len(one) == 24 + 24 + len(inners[0][0])
  assert vqdepth.parse_depth_stages(one, depth=d1)[4:] == ([6, 0, 0], [inners[0][0], b'', b''])
  # an out-of-range map value is clamped as the kernels clamp it
  assert vqdepth.stage_counts(np.array([0, 9, 2, -4]), 3) == [4, 2, 1]


def _patched(blob, offset, value):
  return blob[:offset] + struct.pack('<I', value) + blob[offset + 4:]


def test_every_header_refusal_names_its_field():
  blob, counts, inners = _file()
  first = 24 + 24                                                                  # offset of stage 0's blob
  cases = [
      (b'JPDR' + blob[4:], {}, 'not a coded depth-stage file'),
      (_patched(blob, 4, 2), {}, 'format version 2'),
      (_patched(blob, 8, 9), {}, 'S = 9 stages'),
      (_patched(blob, 8, 0), {}, 'S = 0 stages'),
      (_patched(blob, 12, 0), {}, 'empty code shape'),
      (_patched(blob, 20, 1), {}, 'n_center L = 1'),
      (blob[:40], {}, 'shorter than the header and its two tables'),
      (blob[:10], {}, 'shorter than the 24-byte header'),
      (blob + b'\0', {}, 'beyond'),
      (blob[:-1], {}, 'truncated'),
      (_patched(blob, 24, 8), {}, 'length table: stage 0 takes 8 bytes'),
      (_patched(blob, 24 + 4, 0), {}, 'stage 1: count table says 3 cells, length table says 0 bytes'),
      (_patched(blob, 36 + 8, 0), {}, 'stage 2: count table says 0 cells'),
      (_patched(blob, 36 + 4, 7), {}, 'count table: stage 1 codes 7 cells, more than the 6 of the stage before'),
      (_patched(blob, 36, 25), {}, 'count table: stage 0 codes 25 cells, more than the 24 indices'),
      (blob, dict(stages=0), 'stages = 0'),
      (blob, dict(stages=4), 'stages = 4'),
      (blob, dict(depth=np.array([3, 1, 2, 3, 1, 2])), 'count table: stage 1 codes 3 cells, the depth map implies 4'),
      (blob, dict(depth=np.array([1, 1, 2, 3, 1])), 'the depth map has 5 cells'),
      (blob, dict(depth=np.array([3, 1, 2, 2, 1, 1])), 'count table: stage 2 codes 2 cells, the depth map implies 1'),
      (blob, dict(depth=np.array([3.0, 1.0])), 'the depth map is a non-empty integer array'),
      (_patched(blob, first + 8, 5), dict(depth=DEPTH), 'stage 0'),               # the inner blob's own n
      (_patched(blob, first + 16, 8), dict(depth=DEPTH), 'stage 0'),              # its n_center
      (vqdepth.build_depth_stages([_inner(6, 2, L_, 1)[0]], [6], 2, 12, L_), dict(depth=np.ones(6, dtype=np.int64)),
       'its code_len = 2, the container says 4'),
      (blob[:first] + b'XXXX' + blob[first + 4:], {}, 'stage 0'),
  ]
  for data, kw, text in cases:
    with pytest.raises(ValueError) as err:
      vqdepth.parse_depth_stages(data, **kw)
    assert text in str(err.value), (text, str(err.value))
  with pytest.raises(ValueError, match='a .jpdm blob is bytes'):
    vqdepth.parse_depth_stages('x')
  for bad, text in ((([b'a'] * 9, [1] * 9), 'S = 9 stages'), (([b'a'], [1, 1]), '2 counts for 1 stages'), (([b''], [1]), 'stage 0: count = 1'),
                    (([b'a'], [0]), 'stage 0: count = 0')):
    with pytest.raises(ValueError) as err:
      vqdepth.build_depth_stages(bad[0], bad[1], 2, 12, L_)
    assert text in str(err.value), (text, str(err.value))
  # the reader refuses on the host, before it asks for a device
  with pytest.raises(ValueError, match='the depth map implies 4'):
    vqdepth.read_depth_stages(blob, np.array([3, 1, 2, 3, 1, 2]), device='cuda:0')
  with pytest.raises(ValueError, match='the code is an int64'):
    vqdepth.write_depth_stages(None, torch.zeros(2, 3), DEPTH, L_)


def test_the_older_readers_refuse_the_new_magic_and_the_new_one_theirs():
  blob, _, inners = _file()
  with pytest.raises(ValueError, match='not a coded stage file'):
    vqstages.parse_stages(blob)
  with pytest.raises(ValueError, match='not a coded index file'):
    vqstream.parse_blob(blob)
  jpdr = vqstages.build_stages([inners[0][0]], 6, G_, L_)
  with pytest.raises(ValueError, match='not a coded depth-stage file'):
    vqdepth.parse_depth_stages(jpdr)
  assert vqstages.parse_stages(jpdr)[:4] == (1, 6, G_, L_)


def test_a_packed_file_reads_back_without_a_kernel():
  """Mode-0 inner blobs need no device call: the dense code with -1 past the depth, on the CPU."""
  blob, counts, inners = _file()
  code = vqdepth.read_depth_stages(blob, DEPTH, device='cpu')
  assert tuple(code.shape) == (3, 2, 12) and code.dtype == torch.int64
  cells = code.view(3, 6, G_)
  for s in range(3):
    on = torch.from_numpy(DEPTH > s)
    assert bool((cells[s][~on] == -1).all())
    assert cells[s][on].reshape(-1).tolist() == inners[s][1].tolist()
  two = vqdepth.read_depth_stages(blob, DEPTH, device='cpu', stages=2)
  assert torch.equal(two, code[:2])
  assert torch.equal(vqdepth.read_depth_stages(vqdepth.truncate_depth_stages(blob, 2), DEPTH, device='cpu'), code[:2])


# ---- the module: refused before any device work ------------------------------------------------------------------------------------
def test_module_depth_arguments_refuse_on_the_host():
  from ctu.quantizers import ResidualS2HVQ
  vq = ResidualS2HVQ(torch.zeros(3, 8, 4))
  x = torch.zeros(6, 8)                         # code_len 2: M = 12
  d = torch.ones(4, dtype=torch.int64)
  for bad in (0, 5, -1, True, 2.0):
    with pytest.raises(ValueError, match='groups must be an int that divides'):
      vq.encode(x, 2, depth=d, groups=bad)
  with pytest.raises(ValueError, match='groups is the number of vectors of a depth cell'):
    vq.quantize(x, 2, groups=3)
  for bad in (torch.ones(5, dtype=torch.int64), torch.ones(4), [1, 1, 1, 1]):
    with pytest.raises(ValueError, match='depth must be an int32 or int64 tensor of'):
      vq.quantize(x, 2, depth=bad, groups=3)
  with pytest.raises(ValueError, match='depth must be an int32 or int64 tensor of'):
    vq.decode(torch.zeros(3, 6, 2, dtype=torch.int64), depth=torch.ones(5, dtype=torch.int64), groups=3)
  with pytest.raises(jpdse_hip.JpdseError, match='no CPU fallback'):     # a good call gets as far as the device check
    vq.encode(x, 2, depth=d, groups=3)


# ---- the option: opt.vq_class_stages -------------------------------------------------------------------------------------------------
import importlib.util  # noqa: E402

from ctu.models.model_options import parse_vq_class_stages, resolve_model_options, resolve_vq_class_stages  # noqa: E402
from oracle.ctu_cpu import model as omodel  # noqa: E402


def _load(name):
  spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'scripts', name + '.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


MAKER = _load('make_model_option_refusals')


def _opt(*dicts, **over):
  kw = dict(MAKER.NET)
  for d in dicts:
    kw.update(d)
  kw.update(over)
  return omodel.default_opt(**kw)


def test_class_stages_parse_and_the_star_default():
  table, default = parse_vq_class_stages('24:3,26:3,*:1', 3, 35)
  assert default == 1 and len(table) == 35 and table[24] == 3 and table[26] == 3 and sum(table) == 33 + 6
  table, default = parse_vq_class_stages(' 0:1 , 34:2 ', 4, 35)            # '*' absent: vq_stages
  assert default == 4 and table[0] == 1 and table[34] == 2 and table[1] == 4
  assert parse_vq_class_stages('*:3', 3, 5) == ((3, 3, 3, 3, 3), 3)
  assert parse_vq_class_stages(None, 3, 5) is None
  with MAKER.hidden_device():
    got = resolve_vq_class_stages(_opt(MAKER.S2HVQ, vq_stages=3, vq_class_stages='1:2,*:1'))
    n = len(got[0])
    assert got == (tuple(2 if k == 1 else 1 for k in range(n)), 1) and n in (35, 36)


CLASS_STAGE_REFUSALS = [
    (dict(vq_stages=3, vq_class_stages='1:4'), 'vq_class_stages: depth 4 of \'1\' is outside 1 .. vq_stages = 3'),
    (dict(vq_stages=3, vq_class_stages='1:0'), 'vq_class_stages: depth 0 of \'1\' is outside 1 .. vq_stages = 3'),
    (dict(vq_stages=3, vq_class_stages='*:9'), 'vq_class_stages: depth 9 of \'*\' is outside 1 .. vq_stages = 3'),
    (dict(vq_stages=3, vq_class_stages='1-2'), "vq_class_stages: malformed entry '1-2'"),
    (dict(vq_stages=3, vq_class_stages='1:2,,3:1'), "vq_class_stages: malformed entry ''"),
    (dict(vq_stages=3, vq_class_stages='a:2'), "vq_class_stages: malformed entry 'a:2'"),
    (dict(vq_stages=3, vq_class_stages='1:2.5'), "vq_class_stages: malformed entry '1:2.5'"),
    (dict(vq_stages=3, vq_class_stages='1:2,1:3'), 'class 1 is named twice'),
    (dict(vq_stages=3, vq_class_stages='*:2,*:3'), "'*' is named twice"),
    (dict(vq_stages=3, vq_class_stages='999:2'), 'class 999 is outside the'),
    (dict(vq_stages=3, vq_class_stages=''), 'vq_class_stages must be a string such as'),
    (dict(vq_stages=3, vq_class_stages=3), 'vq_class_stages must be a string such as'),
    (dict(vq_stages=1, vq_class_stages='*:1'), 'vq_class_stages sets the stage depth of the residual bottleneck per class: it needs'),
    (dict(vq_class_stages='*:1'), 'vq_class_stages sets the stage depth of the residual bottleneck per class: it needs'),
    (dict(vq_stages=3, vq_class_stages='*:1', lambda_vq_stage_rate=0.5), 'vq_class_stages cannot be combined with lambda_vq_stage_rate > 0'),
    (dict(vq_stages=3, vq_class_stages='*:1', zero_sem=True), 'vq_class_stages cannot be combined with --zero_sem'),
]


@pytest.mark.parametrize('over,text', CLASS_STAGE_REFUSALS, ids=[str(o) for o, _ in CLASS_STAGE_REFUSALS])
def test_class_stages_are_refused_by_name(over, text):
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  with MAKER.hidden_device():
    with pytest.raises(ValueError) as err:
      resolve_model_options(_opt(MAKER.S2HVQ, over))
    assert text in str(err.value) and 'vq_class_stages' in str(err.value), str(err.value)
    with pytest.raises(ValueError) as err2:                   # the constructor refuses before any network exists
      Pix2PixHDModel(_opt(MAKER.S2HVQ, over))
    assert str(err2.value) == str(err.value)


def test_class_stages_absent_or_none_resolve_to_todays_options():
  with MAKER.hidden_device():
    for base in ({}, MAKER.CODEC, MAKER.S2HVQ, dict(MAKER.S2HVQ, vq_stages=3), dict(MAKER.S2HVQ, vq_stages=2, vq_train_stages='uniform')):
      assert not hasattr(_opt(base), 'vq_class_stages')
      plain = resolve_model_options(_opt(base))
      assert plain == resolve_model_options(_opt(base, vq_class_stages=None)) and resolve_vq_class_stages(_opt(base)) is None
      assert plain._fields[-3:] == ('lambda_vq_stage_rate', 'vq_stages', 'vq_train_stages') and 'vq_class_stages' not in plain._fields
    # with the field the record is still today's: the value travels apart
    assert resolve_model_options(_opt(MAKER.S2HVQ, vq_stages=3, vq_class_stages='1:2')) == resolve_model_options(_opt(MAKER.S2HVQ, vq_stages=3))


def test_the_depth_codec_and_the_host_rule():
  from ctu.models.codec import VQDepthCodec, VQStagesCodec
  assert issubclass(VQDepthCodec, VQStagesCodec) and VQDepthCodec.RATE_OPTION == 'lambda_vq_stage_rate'
  assert VQDepthCodec.truncate is vqdepth.truncate_depth_stages and VQStagesCodec.truncate is vqstages.truncate_stages
  lab = np.random.RandomState(2).randint(0, 9, size=(2, 1, 8, 16)).astype(np.float32)
  lab[0, 0, 0, 0] = float('nan')
  table = [3, 1, 2, 1, 3, 2]
  for step in (1, 4):
    assert np.array_equal(vqdepth.depth_map_host(torch.from_numpy(lab), table, 2, step), ref.depth_map(lab, table, 2, step))
