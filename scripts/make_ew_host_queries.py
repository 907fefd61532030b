#!/usr/bin/env python3
"""Writes tests/golden/ew_host_queries.json: what the host layer of norm.hip, elementwise.hip, binarize.hip and metrics.hip
answers without a device (tests/test_host_ew_queries.py replays it).  Two parts:

  answers   the workspace-size / partial-count queries: jpdse_inorm_workspace_size for every InstanceNorm of the three bench
            configurations (GlobalGenerator ngf 64 at 1024x512 batch 4; LocalEnhancer ngf 32 at 1024x512 batch 1; 512x256
            batch 1), both PatchGAN scales, the same at 2048x1024, and the norm shapes tests/test_hip_ops.py parametrises (read
            from that file, not imported), in bf16 and fp32; jpdse_channel_sum_workspace_size, jpdse_loss_workspace_size,
            jpdse_loss_partial_count, jpdse_quant_loss_workspace_size, jpdse_code_stats_workspace_size and
            jpdse_eval_metrics_workspace_size over a range of arguments;
  refusals  for every launching entry point of the four files, calls that must be refused BEFORE any launch (bad dtype, null
            pointer, non-positive extent, count that is not a vector multiple, workspace one byte short, has_residual without a
            residual, zero slots): the return code and the text of jpdse_last_error().

  python scripts/make_ew_host_queries.py [OUT.json]        (JPDSE_HIP_LIB=<libjpdse_hip.so of another build> to record that one)

Nothing is launched; run as a script it also hides every GPU from the process first, so a call that a broken build fails to
refuse ends as a launch error and never reaches a device with the placeholder pointers used here.  Regenerate the fixture ONLY
with a change that means to resize a workspace or to reword a refusal, and say so in that change."""
import ast
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'jpd-se_amd'))

import jpdse_hip                                                               # noqa: E402
from jpdse_hip import InormDesc, LossTerm, F32, BF16                           # noqa: E402

ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
SLOPE, EPS = 0.2, 1e-5
P = 0x1000                 # placeholder for a non-null device pointer: a refused call never reads it


# ---- InstanceNorm shapes -----------------------------------------------------------------------------------------------------
def generator_norms(N, H, W, ngf, n_down, n_blocks=9):
  """(N, H, W, C, act, has_residual) of the norms of a GlobalGenerator without its head."""
  out = [(N, H, W, ngf, ACT_RELU, 0)]
  c, h, w = ngf, H, W
  for _ in range(n_down):
    c, h, w = 2 * c, h // 2, w // 2
    out.append((N, h, w, c, ACT_RELU, 0))
  out += [(N, h, w, c, ACT_RELU, 0), (N, h, w, c, ACT_NONE, 1)] * n_blocks       # ResnetBlock: norm + ReLU, norm + residual
  for _ in range(n_down):
    c, h, w = c // 2, 2 * h, 2 * w
    out.append((N, h, w, c, ACT_RELU, 0))
  return out


def local_enhancer_norms(N, H, W, ngf, n_down_global):
  out = generator_norms(N, H // 2, W // 2, 2 * ngf, n_down_global)
  out += [(N, H, W, ngf, ACT_RELU, 0), (N, H // 2, W // 2, 2 * ngf, ACT_RELU, 0)]
  out += [(N, H // 2, W // 2, 2 * ngf, ACT_RELU, 0), (N, H // 2, W // 2, 2 * ngf, ACT_NONE, 1)] * 3
  out.append((N, H, W, ngf, ACT_RELU, 0))
  return out


def patchgan_norms(N, H, W, ndf=64):
  out = []
  for scale in range(2):
    h, w = H >> scale, W >> scale
    for j in range(4):
      st = 2 if j < 3 else 1
      h, w = (h + 4 - 4) // st + 1, (w + 4 - 4) // st + 1
      if j > 0:
        out.append((N, h, w, ndf << j, ACT_LRELU, 0))
  return out


def test_shapes():
  """The norm shapes of tests/test_hip_ops.py, evaluated from its source: FUSED_NORM_SHAPES, the `shape` lists of the norm
  tests' parametrize decorators, and the conv outputs of FUSED_MOMENT_CASES / FUSED_MOMENT_FULL (conv -> norm stages)."""
  tree = ast.parse(open(os.path.join(ROOT, 'tests', 'test_hip_ops.py')).read())
  out = []
  for node in tree.body:
    name = getattr(node.targets[0], 'id', '') if isinstance(node, ast.Assign) else ''
    if name == 'FUSED_NORM_SHAPES':
      for _, (N, C, H, W), res in ast.literal_eval(node.value):
        out.append((N, H, W, C, ACT_RELU, int(res)))
    elif name in ('FUSED_MOMENT_CASES', 'FUSED_MOMENT_FULL'):
      for case in node.value.elts:
        call, (N, _, H, W) = case.elts[1].body, ast.literal_eval(case.elts[2])
        _, cout, k, st, pad = [ast.literal_eval(a) for a in call.args[:5]]
        if any(kw.arg == 'transposed' for kw in call.keywords):
          out.append((N, 2 * H, 2 * W, cout, ACT_RELU, 0))
        else:
          out.append((N, (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1, cout, ACT_RELU, 0))
    elif isinstance(node, ast.FunctionDef) and 'norm' in node.name:
      for dec in node.decorator_list:
        if isinstance(dec, ast.Call) and isinstance(dec.args[0], ast.Constant) and dec.args[0].value == 'shape':
          for (N, C, H, W) in ast.literal_eval(dec.args[1]):
            out.append((N, H, W, C, ACT_LRELU, 0))
  assert len(out) >= 18, 'norm shape lists of tests/test_hip_ops.py not found'
  return out


def inorm_descriptors():
  shapes = []
  for H, W in ((512, 1024), (1024, 2048)):
    for N in (1, 4):
      shapes += generator_norms(N, H, W, 64, 4) + local_enhancer_norms(N, H, W, 32, 4)
    for N in (1, 2, 4, 8):                                   # real + fake halves run as one batch
      shapes += patchgan_norms(N, H, W)
  shapes += generator_norms(1, 256, 512, 64, 4) + local_enhancer_norms(1, 256, 512, 32, 4)
  for N in (1, 2):
    shapes += patchgan_norms(N, 256, 512)
  shapes += test_shapes()
  seen, out = set(), []
  for dt in (BF16, F32):
    for s in shapes:
      key = (dt,) + s
      if key not in seen:
        seen.add(key)
        out.append(key)
  return out


def ndesc(dtype, N, H, W, C, act=ACT_RELU, has_residual=0):
  return InormDesc(dtype, N, H, W, C, act, SLOPE, EPS, has_residual)


# ---- answers -----------------------------------------------------------------------------------------------------------------
def answer_keys():
  """[query name, argument list] of every recorded answer."""
  keys = [['jpdse_inorm_workspace_size', list(k)] for k in inorm_descriptors()]
  keys += [['jpdse_inorm_workspace_size', list(k)] for k in ((2, 1, 8, 8, 8, ACT_RELU, 0), (BF16, 0, 8, 8, 8, ACT_RELU, 0),
                                                             (BF16, 1, 8, 8, 0, ACT_RELU, 0), (BF16, 1, 8, 8, 8, 3, 0))]   # refused: 0
  keys += [['jpdse_channel_sum_workspace_size', [npix, C]] for npix in (1, 255, 4096, 524288, 1 << 22)
           for C in (1, 3, 8, 39, 64, 100, 512, 1024)]
  work = (-1, 0, 1, 255, 256, 257, 65536, 262143, 262144, 262145, 1 << 24, 1 << 33)
  keys += [['jpdse_loss_workspace_size', [n]] for n in work]
  keys += [['jpdse_loss_partial_count', [n]] for n in work]
  keys += [['jpdse_quant_loss_workspace_size', []]]
  keys += [['jpdse_code_stats_workspace_size', [dt, N, H, W, C]] for dt in (BF16, F32, 2)
           for (N, H, W, C) in ((1, 8, 16, 8), (4, 64, 128, 8), (4, 64, 128, 16), (2, 33, 65, 3), (1, 128, 256, 32),
                                (8, 256, 512, 8), (0, 8, 8, 8), (1, 8, 8, 0))]
  keys += [['jpdse_eval_metrics_workspace_size', [N, H, W, C]] for (N, H, W, C) in (
      (1, 176, 176, 3), (1, 256, 512, 3), (1, 512, 1024, 3), (4, 512, 1024, 3), (2, 1024, 2048, 3), (3, 177, 301, 3),
      (1, 175, 512, 3), (1, 512, 1024, 4), (0, 512, 1024, 3), (21846, 176, 176, 3))]
  return keys


def answer(L, name, args):
  if name == 'jpdse_inorm_workspace_size':
    d = ndesc(*args)
    return L.jpdse_inorm_workspace_size(ctypes.byref(d))
  return getattr(L, name)(*args)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
# An argument is an int / float passed as is, or a tagged list the replay turns into a host object:
#   ['desc', dtype, N, H, W, C, act, has_residual]   jpdse_inorm_desc (['desc']: null)   ['f64', ...]   host array of doubles
#   ['ptrs', ...]   host array of pointers           ['terms', [partial, n, out], ...]       host array of jpdse_loss_term
def refusals():
  """[entry point, what is wrong, argument list] of every recorded refusal."""
  D = ['desc', BF16, 2, 16, 32, 64, ACT_RELU, 0]
  DR = ['desc', BF16, 2, 16, 32, 64, ACT_NONE, 1]
  ws = answer(jpdse_hip.lib(), 'jpdse_inorm_workspace_size', D[1:])
  sums_ws = 2 * 64 * 2 * 4                          # [N][CPAD(C)][2] floats, already a multiple of 256
  out = []

  def add(fn, what, *args):
    out.append([fn, what, list(args)])

  bad_desc = (('bad dtype', ['desc', 2, 2, 16, 32, 64, ACT_RELU, 0]), ('non-positive extent', ['desc', BF16, 2, 0, 32, 64, ACT_RELU, 0]),
              ('unsupported activation', ['desc', BF16, 2, 16, 32, 64, 3, 0]))
  for what, d in bad_desc:
    add('jpdse_inorm_fwd', what, d, P, 0, P, P, P, ws, 0)
    add('jpdse_inorm_bwd', what, d, P, P, P, P, P, ws, 0)
    add('jpdse_inorm_bwd_from_sums', what, d, P, P, P, P, 8, P, P, ws, 0)
    add('jpdse_inorm_fwd_from_moments', what, d, P, P, 8, 0, P, P, 0)
  add('jpdse_inorm_fwd', 'null descriptor', ['desc'], P, 0, P, P, P, ws, 0)
  add('jpdse_inorm_fwd', 'null pointer', D, 0, 0, P, P, P, ws, 0)
  add('jpdse_inorm_fwd', 'has_residual without a residual', DR, P, 0, P, P, P, ws, 0)
  add('jpdse_inorm_fwd', 'workspace one byte short', D, P, 0, P, P, P, ws - 1, 0)
  add('jpdse_inorm_fwd', 'null workspace', D, P, 0, P, P, 0, ws, 0)
  add('jpdse_inorm_bwd', 'null pointer', D, P, P, 0, P, P, ws, 0)
  add('jpdse_inorm_bwd', 'workspace one byte short', D, P, P, P, P, P, ws - 1, 0)
  add('jpdse_inorm_bwd_from_sums', 'null pointer', D, P, P, P, 0, 8, P, P, ws, 0)
  add('jpdse_inorm_bwd_from_sums', 'zero slots', D, P, P, P, P, 0, P, P, ws, 0)
  add('jpdse_inorm_bwd_from_sums', 'workspace one byte short', D, P, P, P, P, 8, P, P, sums_ws - 1, 0)
  add('jpdse_inorm_fwd_from_moments', 'null pointer', D, P, 0, 8, 0, P, P, 0)
  add('jpdse_inorm_fwd_from_moments', 'zero slots', D, P, P, 0, 0, P, P, 0)
  add('jpdse_inorm_fwd_from_moments', 'has_residual without a residual', DR, P, P, 8, 0, P, P, 0)

  for fn in ('jpdse_avgpool3s2_fwd', 'jpdse_avgpool3s2_bwd', 'jpdse_maxpool2_fwd'):
    add(fn, 'bad dtype', 2, 1, 8, 8, 8, P, P, 0)
    add(fn, 'null pointer', BF16, 1, 8, 8, 8, P, 0, 0)
    add(fn, 'non-positive extent', BF16, 1, 8, 8, 0, P, P, 0)
  add('jpdse_maxpool2_fwd', 'height below 2', F32, 1, 1, 8, 8, P, P, 0)
  add('jpdse_maxpool2_bwd', 'bad dtype', 2, 1, 8, 8, 8, P, P, P, 0)
  add('jpdse_maxpool2_bwd', 'null pointer', BF16, 1, 8, 8, 8, P, 0, P, 0)
  add('jpdse_maxpool2_bwd', 'width below 2', BF16, 1, 8, 1, 8, P, P, P, 0)

  add('jpdse_act_bwd', 'bad dtype', 2, 64, ACT_RELU, SLOPE, P, P, P, 0)
  add('jpdse_act_bwd', 'null pointer', BF16, 64, ACT_RELU, SLOPE, P, 0, P, 0)
  add('jpdse_act_bwd', 'non-positive extent', BF16, 0, ACT_RELU, SLOPE, P, P, P, 0)
  add('jpdse_act_bwd', 'not a vector multiple (bf16)', BF16, 60, ACT_RELU, SLOPE, P, P, P, 0)
  add('jpdse_act_bwd', 'not a vector multiple (fp32)', F32, 62, ACT_RELU, SLOPE, P, P, P, 0)
  add('jpdse_add', 'bad dtype', -1, 64, P, P, P, 0)
  add('jpdse_add', 'null pointer', F32, 64, P, P, 0, 0)
  add('jpdse_add', 'not a vector multiple (bf16)', BF16, 68, P, P, P, 0)
  add('jpdse_add', 'not a vector multiple (fp32)', F32, 66, P, P, P, 0)
  add('jpdse_zero', 'bad dtype', 2, 64, P, 0)
  add('jpdse_zero', 'null pointer', F32, 64, 0, 0)
  add('jpdse_zero', 'negative count', F32, -1, P, 0)

  csum_ws = answer(jpdse_hip.lib(), 'jpdse_channel_sum_workspace_size', [4096, 39])
  add('jpdse_channel_sum', 'bad dtype', 2, 4096, 39, P, P, P, csum_ws, 0)
  add('jpdse_channel_sum', 'null pointer', BF16, 4096, 39, P, 0, P, csum_ws, 0)
  add('jpdse_channel_sum', 'non-positive extent', BF16, 0, 39, P, P, P, csum_ws, 0)
  add('jpdse_channel_sum', 'workspace one byte short', BF16, 4096, 39, P, P, P, csum_ws - 1, 0)
  add('jpdse_channel_sum', 'null workspace', BF16, 4096, 39, P, P, 0, csum_ws, 0)
  add('jpdse_channel_copy', 'bad dtype', 2, 64, P, 16, 0, P, 16, 0, 8, 0)
  add('jpdse_channel_copy', 'null pointer', BF16, 64, 0, 16, 0, P, 16, 0, 8, 0)
  add('jpdse_channel_copy', 'non-positive extent', BF16, 64, P, 16, 0, P, 16, 0, 0, 0)
  add('jpdse_channel_copy', 'channel range out of bounds', BF16, 64, P, 16, 12, P, 16, 0, 8, 0)
  add('jpdse_concat_channels', 'bad dtype', 2, 64, P, 40, P, 8, 36, 3, P, 0)
  add('jpdse_concat_channels', 'null pointer', BF16, 64, P, 40, 0, 8, 36, 3, P, 0)
  add('jpdse_concat_channels', 'non-positive extent', BF16, 0, P, 40, P, 8, 36, 3, P, 0)
  add('jpdse_concat_channels', 'channel range out of bounds', BF16, 64, P, 40, P, 8, 38, 3, P, 0)
  add('jpdse_concat_channels', 'storage not a multiple of 8', F32, 64, P, 39, P, 8, 36, 3, P, 0)
  add('jpdse_insert_channels', 'bad dtype', 2, 64, P, 40, P, 8, 36, 3, 0)
  add('jpdse_insert_channels', 'null pointer', BF16, 64, P, 40, 0, 8, 36, 3, 0)
  add('jpdse_insert_channels', 'non-positive extent', BF16, 0, P, 40, P, 8, 36, 3, 0)
  add('jpdse_insert_channels', 'channel range out of bounds', BF16, 64, P, 40, P, 8, 38, 3, 0)
  add('jpdse_copy', 'null pointer', 64, 0, P, 0)
  add('jpdse_copy', 'not a multiple of 16 bytes', 72, P, P, 0)
  add('jpdse_copy', 'non-positive extent', 0, P, P, 0)
  add('jpdse_copy', 'misaligned pointer', 64, P + 8, P, 0)
  add('jpdse_cast', 'same dtype', F32, F32, 64, P, P, 0)
  add('jpdse_cast', 'bad dtype', F32, 2, 64, P, P, 0)
  add('jpdse_cast', 'null pointer', F32, BF16, 64, 0, P, 0)
  add('jpdse_cast', 'not a multiple of 8', BF16, F32, 60, P, P, 0)

  for fn in ('jpdse_nchw_to_nhwc', 'jpdse_nhwc_to_nchw'):
    add(fn, 'bad dtype', 2, 1, 3, 8, 8, P, P, 0)
    add(fn, 'null pointer', BF16, 1, 3, 8, 8, 0, P, 0)
    add(fn, 'non-positive extent', BF16, 1, 0, 8, 8, P, P, 0)
  add('jpdse_onehot_edge', 'bad dtype', 2, 1, 8, 8, 35, P, P, P, 40, 0)
  add('jpdse_onehot_edge', 'null pointer', BF16, 1, 8, 8, 35, P, 0, P, 40, 0)
  add('jpdse_onehot_edge', 'non-positive extent', BF16, 1, 0, 8, 35, P, P, P, 40, 0)
  add('jpdse_onehot_edge', 'labels fill the storage', BF16, 1, 8, 8, 40, P, P, P, 40, 0)
  add('jpdse_onehot_edge', 'storage not a multiple of 8', BF16, 1, 8, 8, 35, P, P, P, 39, 0)
  two = ['ptrs', P, P]
  add('jpdse_input_builder', 'bad dtype', 2, 1, 8, 8, 35, P, P, 2, two, two, 40, 8, 36, 3, 0)
  add('jpdse_input_builder', 'null pointer', BF16, 1, 8, 8, 35, 0, P, 2, two, two, 40, 8, 36, 3, 0)
  add('jpdse_input_builder', 'non-positive extent', BF16, 0, 8, 8, 35, P, P, 2, two, two, 40, 8, 36, 3, 0)
  add('jpdse_input_builder', 'four destinations', BF16, 1, 8, 8, 35, P, P, 4, two, two, 40, 8, 36, 3, 0)
  add('jpdse_input_builder', 'bad channel counts', BF16, 1, 8, 8, 40, P, P, 2, two, two, 40, 8, 36, 3, 0)
  add('jpdse_input_builder', 'image channels outside the storage', BF16, 1, 8, 8, 35, P, P, 2, two, two, 40, 8, 38, 3, 0)
  add('jpdse_input_builder', 'null destination', BF16, 1, 8, 8, 35, P, P, 2, ['ptrs', P, 0], two, 40, 8, 36, 3, 0)
  add('jpdse_input_builder', 'unsupported storage width (bf16)', BF16, 1, 8, 8, 35, P, P, 2, two, two, 72, 8, 36, 3, 0)
  add('jpdse_input_builder', 'unsupported storage width (fp32)', F32, 1, 8, 8, 35, P, P, 2, two, two, 72, 8, 36, 3, 0)

  lws = answer(jpdse_hip.lib(), 'jpdse_loss_workspace_size', [1024])
  for fn in ('jpdse_l1_fwd', 'jpdse_mse_fwd'):
    add(fn, 'bad dtype', 2, 1024, 1000, P, P, P, P, lws, 0)
    add(fn, 'null pointer', BF16, 1024, 1000, 0, P, P, P, lws, 0)
    add(fn, 'null b', BF16, 1024, 1000, P, 0, P, P, lws, 0)
    add(fn, 'non-positive extent', BF16, 0, 1000, P, P, P, P, lws, 0)
    add(fn, 'non-positive count', BF16, 1024, 0, P, P, P, P, lws, 0)
    add(fn, 'not a vector multiple (bf16)', BF16, 1020, 1000, P, P, P, P, lws, 0)
    add(fn, 'not a vector multiple (fp32)', F32, 1022, 1000, P, P, P, P, lws, 0)
    add(fn, 'workspace one byte short', BF16, 1024, 1000, P, P, P, P, lws - 1, 0)
    add(fn, 'null workspace', BF16, 1024, 1000, P, P, P, 0, lws, 0)
  for fn in ('jpdse_l1_bwd', 'jpdse_l1_bwd_relu', 'jpdse_mse_bwd'):
    add(fn, 'bad dtype', 2, 1024, 1000, P, P, P, 1.0, P, 0)
    add(fn, 'null pointer', BF16, 1024, 1000, P, P, 0, 1.0, P, 0)
    add(fn, 'null b', BF16, 1024, 1000, P, 0, P, 1.0, P, 0)
    add(fn, 'not a vector multiple (bf16)', BF16, 1020, 1000, P, P, P, 1.0, P, 0)
    add(fn, 'non-positive count', F32, 1024, 0, P, P, P, 1.0, P, 0)
  add('jpdse_l1_fwd_bwd', 'bad dtype', 2, 1024, 1000, P, P, P, 1.0, 0, P, P, lws, 0)
  add('jpdse_l1_fwd_bwd', 'null pointer', BF16, 1024, 1000, P, P, P, 1.0, 0, 0, P, lws, 0)
  add('jpdse_l1_fwd_bwd', 'non-positive count', BF16, 1024, 0, P, P, P, 1.0, 0, P, P, lws, 0)
  add('jpdse_l1_fwd_bwd', 'not a vector multiple (fp32)', F32, 1022, 1000, P, P, P, 1.0, 0, P, P, lws, 0)
  add('jpdse_l1_fwd_bwd', 'workspace one byte short', BF16, 1024, 1000, P, P, P, 1.0, 1, P, P, lws - 1, 0)
  add('jpdse_mse_const_fwd', 'bad dtype', 2, 1024, 8, 1.0, P, P, P, lws, 0)
  add('jpdse_mse_const_fwd', 'bad storage', BF16, 1024, 0, 1.0, P, P, P, lws, 0)
  add('jpdse_mse_const_fwd', 'null pointer', BF16, 1024, 8, 1.0, 0, P, P, lws, 0)
  add('jpdse_mse_const_fwd', 'non-positive extent', BF16, 0, 8, 1.0, P, P, P, lws, 0)
  add('jpdse_mse_const_fwd', 'workspace one byte short', BF16, 1024, 8, 1.0, P, P, P, lws - 1, 0)
  add('jpdse_mse_const_bwd', 'bad dtype', 2, 1024, 8, 1.0, P, P, 1.0, P, 0)
  add('jpdse_mse_const_bwd', 'bad storage', BF16, 1024, -8, 1.0, P, P, 1.0, P, 0)
  add('jpdse_mse_const_bwd', 'null pointer', BF16, 1024, 8, 1.0, P, 0, 1.0, P, 0)
  add('jpdse_mse_const_bwd', 'non-positive extent', BF16, 0, 8, 1.0, P, P, 1.0, P, 0)
  add('jpdse_loss_finalize', 'null pointer', 0, 1, 0)
  add('jpdse_loss_finalize', 'no terms', ['terms', [P, 4, P]], 0, 0)
  add('jpdse_loss_finalize', 'term without partials', ['terms', [0, 4, P]], 1, 0)
  add('jpdse_loss_finalize', 'term with too many partials', ['terms', [P, 1025, P]], 1, 0)
  add('jpdse_adam_step', 'null pointer', 0, 1, 1, 2e-4, 0.5, 0.999, 1e-8, 1, 1.0, 0)
  add('jpdse_adam_step', 'no entries', P, 0, 1, 2e-4, 0.5, 0.999, 1e-8, 1, 1.0, 0)
  add('jpdse_adam_step', 'step zero', P, 1, 1, 2e-4, 0.5, 0.999, 1e-8, 0, 1.0, 0)

  ms = ['f64', 0.5, 0.5, 0.5]
  qws = answer(jpdse_hip.lib(), 'jpdse_quant_loss_workspace_size', [])
  add('jpdse_quant_loss', 'bad dtype of a', 2, F32, 4096, 3, P, P, ms, ms, 0, P, P, qws, 0)
  add('jpdse_quant_loss', 'bad dtype of b', BF16, 2, 4096, 3, P, P, ms, ms, 0, P, P, qws, 0)
  add('jpdse_quant_loss', 'null pointer', BF16, F32, 4096, 3, P, 0, ms, ms, 0, P, P, qws, 0)
  add('jpdse_quant_loss', 'non-positive extent', BF16, F32, 0, 3, P, P, ms, ms, 0, P, P, qws, 0)
  add('jpdse_quant_loss', 'nine channels', BF16, F32, 4096, 9, P, P, ms, ms, 0, P, P, qws, 0)
  add('jpdse_quant_loss', 'workspace one byte short', BF16, F32, 4096, 3, P, P, ms, ms, 1, P, P, qws - 1, 0)

  add('jpdse_binarize_fwd', 'bad dtype', 2, 1, 8, 8, 8, P, P, 1, 7, 0, 0, 0, 0)
  add('jpdse_binarize_fwd', 'null pointer', BF16, 1, 8, 8, 8, 0, P, 1, 7, 0, 0, 0, 0)
  add('jpdse_binarize_fwd', 'non-positive extent', BF16, 1, 8, 0, 8, P, P, 1, 7, 0, 0, 0, 0)
  add('jpdse_binarize_fwd', 'negative image index', BF16, 1, 8, 8, 8, P, P, 1, 7, 0, -1, 0, 0)
  add('jpdse_binarize_fwd', 'image index beyond 32 bits', BF16, 1, 8, 8, 8, P, P, 1, 7, 0, 0xffffffff, 0, 0)
  cws = answer(jpdse_hip.lib(), 'jpdse_code_stats_workspace_size', [BF16, 4, 64, 128, 8])
  add('jpdse_code_stats', 'bad dtype', 2, 4, 64, 128, 8, P, P, P, cws, 0)
  add('jpdse_code_stats', 'null pointer', BF16, 4, 64, 128, 8, P, 0, P, cws, 0)
  add('jpdse_code_stats', 'non-positive extent', BF16, 0, 64, 128, 8, P, P, P, cws, 0)
  add('jpdse_code_stats', 'more than 2^31 bits per image', BF16, 1, 32768, 32768, 2, P, P, P, 1 << 20, 0)
  add('jpdse_code_stats', 'workspace one byte short', BF16, 4, 64, 128, 8, P, P, P, cws - 1, 0)
  add('jpdse_code_export', 'bad dtype', 2, 1, 8, 8, 8, P, 0, P, 0)
  add('jpdse_code_export', 'null pointer', BF16, 1, 8, 8, 8, P, 1, 0, 0)
  add('jpdse_code_export', 'non-positive extent', BF16, 1, 8, 8, 0, P, 1, P, 0)

  ews = answer(jpdse_hip.lib(), 'jpdse_eval_metrics_workspace_size', [1, 256, 512, 3])
  add('jpdse_eval_metrics', 'bad dtype of fake', 2, F32, 1, 256, 512, 3, P, P, ms, ms, P, P, ews, 0)
  add('jpdse_eval_metrics', 'bf16 real', BF16, BF16, 1, 256, 512, 3, P, P, ms, ms, P, P, ews, 0)
  add('jpdse_eval_metrics', 'null pointer', BF16, F32, 1, 256, 512, 3, 0, P, ms, ms, P, P, ews, 0)
  add('jpdse_eval_metrics', 'non-positive extent', BF16, F32, 0, 256, 512, 3, P, P, ms, ms, P, P, ews, 0)
  add('jpdse_eval_metrics', 'four channels', BF16, F32, 1, 256, 512, 4, P, P, ms, ms, P, P, ews, 0)
  add('jpdse_eval_metrics', 'side below 176', BF16, F32, 1, 175, 512, 3, P, P, ms, ms, P, P, ews, 0)
  add('jpdse_eval_metrics', 'workspace one byte short', BF16, F32, 1, 256, 512, 3, P, P, ms, ms, P, P, ews - 1, 0)
  add('jpdse_eval_metrics', 'misaligned workspace', BF16, F32, 1, 256, 512, 3, P, P, ms, ms, P, P + 4, ews, 0)
  return out


def refuse(L, fn, args):
  """[return code, jpdse_last_error()] of one call that must be refused."""
  keep, real = [], []
  for a in args:
    if isinstance(a, list) and a[0] == 'desc':
      keep.append(ndesc(*a[1:]) if len(a) > 1 else None)           # ['desc'] alone: a null descriptor
      real.append(ctypes.byref(keep[-1]) if len(a) > 1 else None)
    elif isinstance(a, list) and a[0] == 'f64':
      real.append((ctypes.c_double * (len(a) - 1))(*a[1:]))
    elif isinstance(a, list) and a[0] == 'ptrs':
      real.append((ctypes.c_void_p * (len(a) - 1))(*a[1:]))
    elif isinstance(a, list) and a[0] == 'terms':
      keep.append((LossTerm * (len(a) - 1))(*[LossTerm(p, n, 1.0, o) for p, n, o in a[1:]]))
      real.append(ctypes.cast(keep[-1], ctypes.c_void_p))
    else:
      real.append(a)
  rc = getattr(L, fn)(*real)
  msg = L.jpdse_last_error().decode('utf-8', 'replace')
  assert rc in (-1, -2), '%s %s: not refused as a bad argument or a short workspace (%d: %s)' % (fn, args, rc, msg)
  return [rc, msg]


def record():
  L = jpdse_hip.lib()
  return {'slope': SLOPE, 'eps': EPS,
          'answers': [[n, a, answer(L, n, a)] for n, a in answer_keys()],
          'refusals': [[fn, what, args] + refuse(L, fn, args) for fn, what, args in refusals()]}


def main(path):
  fix = record()
  with open(path, 'w') as f:
    f.write('{"slope": %s, "eps": %s,\n "answers": [\n' % (fix['slope'], fix['eps']))
    f.write(',\n'.join(json.dumps(c, separators=(',', ':')) for c in fix['answers']))
    f.write('\n],\n "refusals": [\n')
    f.write(',\n'.join(json.dumps(c, separators=(',', ':')) for c in fix['refusals']))
    f.write('\n]}\n')
  print('%d answers, %d refusals -> %s (library: %s)' % (len(fix['answers']), len(fix['refusals']), path, jpdse_hip.LIB_PATH))


if __name__ == '__main__':
  os.environ['HIP_VISIBLE_DEVICES'] = '-1'         # before the runtime loads: see the module docstring
  main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'ew_host_queries.json'))
