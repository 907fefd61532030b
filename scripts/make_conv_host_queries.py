#!/usr/bin/env python3
"""Writes tests/golden/conv_host_queries.json: what the host-side query entry points of the library answer for the
conv / ConvTranspose layers of the product (tests/test_host_conv_queries.py replays it).  None of them launches anything, so
this runs without a GPU.

  python scripts/make_conv_host_queries.py [OUT.json]        (JPDSE_HIP_LIB=<libjpdse_hip.so of another build> to record that one)

The answers -- plan, workspace / panel sizes, moment and norm-sum slot counts, repack-table length -- are computed by the
predicates that choose a layer's kernel, so the fixture holds the dispatch conditions still: regenerate it ONLY with a change
that means to move a layer to another kernel or to change a workspace layout, and say so in that change.

Layers: every conv of the three bench configurations (GlobalGenerator ngf 64 at 1024x512 batch 4; LocalEnhancer ngf 32 at
1024x512 batch 1; 512x256 batch 1), of both PatchGAN scales and of VGG19, in bf16 and fp32; the same at 2048x1024; and the
shapes the conv tests of tests/test_hip_ops.py parametrise (read from that file, not imported)."""
import ast
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'jpd-se_amd'))

import jpdse_hip                                                               # noqa: E402
from jpdse_hip import ConvDesc, F32, BF16, PAD_ZERO, PAD_REFLECT               # noqa: E402

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3
DESC_FIELDS = ['dtype', 'N', 'H', 'W', 'C', 'K', 'R', 'S', 'stride', 'pad', 'pad_mode', 'act']
SLOPE = 0.2


def generator_layers(N, H, W, ngf, n_down, cin=39, head=True):
  """(N, H, W, C, K, k, stride, pad, mode, act) of a GlobalGenerator; H, W of the underlying Conv2d's input."""
  out = [(N, H, W, cin, ngf, 7, 1, 3, PAD_REFLECT, ACT_NONE)]
  c, h, w = ngf, H, W
  for _ in range(n_down):
    out.append((N, h, w, c, 2 * c, 3, 2, 1, PAD_ZERO, ACT_NONE))
    c, h, w = 2 * c, h // 2, w // 2
  out.append((N, h, w, c, c, 3, 1, 1, PAD_REFLECT, ACT_NONE))                  # ResnetBlock convs
  for _ in range(n_down):                                                      # ConvTranspose2d = data gradient of this conv
    out.append((N, 2 * h, 2 * w, c // 2, c, 3, 2, 1, PAD_ZERO, ACT_NONE))
    c, h, w = c // 2, 2 * h, 2 * w
  if head:
    out.append((N, H, W, ngf, 3, 7, 1, 3, PAD_REFLECT, ACT_TANH))
  return out


def local_enhancer_layers(N, H, W, ngf, n_down_global):
  out = generator_layers(N, H // 2, W // 2, 2 * ngf, n_down_global, head=False)
  out += [(N, H, W, 39, ngf, 7, 1, 3, PAD_REFLECT, ACT_NONE), (N, H, W, ngf, 2 * ngf, 3, 2, 1, PAD_ZERO, ACT_NONE),
          (N, H // 2, W // 2, 2 * ngf, 2 * ngf, 3, 1, 1, PAD_REFLECT, ACT_NONE),
          (N, H, W, ngf, 2 * ngf, 3, 2, 1, PAD_ZERO, ACT_NONE), (N, H, W, ngf, 3, 7, 1, 3, PAD_REFLECT, ACT_TANH)]
  return out


def patchgan_layers(N, H, W, ndf=64):
  out = []
  for scale in range(2):
    h, w = H >> scale, W >> scale
    chans = [39, ndf, 2 * ndf, 4 * ndf, 8 * ndf, 1]
    for j in range(5):
      st = 2 if j < 3 else 1
      out.append((N, h, w, chans[j], chans[j + 1], 4, st, 2, PAD_ZERO, ACT_LRELU if j == 0 else ACT_NONE))
      if j == 0:
        out.append((N, h, w, 3, ndf, 4, st, 2, PAD_ZERO, ACT_NONE))            # data gradient w.r.t. the image channels only
      h, w = (h + 4 - 4) // st + 1, (w + 4 - 4) // st + 1
  return out


def vgg_layers(N, H, W):
  out, cin, h, w = [], 3, H, W
  for item in [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 256, 'M', 512, 512, 512, 512, 'M', 512]:
    if item == 'M':
      h, w = h // 2, w // 2
      continue
    out.append((N, h, w, cin, item, 3, 1, 1, PAD_ZERO, ACT_RELU))
    cin = item
  return out


def test_cases():
  """The conv case tables of tests/test_hip_ops.py, evaluated from its source."""
  names = dict(PAD_ZERO=PAD_ZERO, PAD_REFLECT=PAD_REFLECT, ACT_NONE=ACT_NONE, ACT_RELU=ACT_RELU, ACT_LRELU=ACT_LRELU,
               ACT_TANH=ACT_TANH)
  tree = ast.parse(open(os.path.join(ROOT, 'tests', 'test_hip_ops.py')).read())
  out = []
  for node in tree.body:
    if isinstance(node, ast.Assign) and getattr(node.targets[0], 'id', '') in ('CONV_CASES', 'FUSED_RELU_CASES', 'LRELU_CASES',
                                                                               'FULL_SIZE_LAYERS'):
      for case in eval(compile(ast.Expression(node.value), 'test_hip_ops.py', 'eval'), names):
        out.append(tuple(case[1:10]) + ((case[10],) if len(case) > 10 else (ACT_NONE,)))
  assert len(out) > 100, 'case tables of tests/test_hip_ops.py not found'
  return out


def all_descriptors():
  layers = []
  for H, W in ((512, 1024), (1024, 2048)):
    for N in (1, 4):
      layers += generator_layers(N, H, W, 64, 4)
      layers += local_enhancer_layers(N, H, W, 32, 4)
    for N in (1, 2, 4, 8):                                   # real + fake halves run as one batch
      layers += patchgan_layers(N, H, W) + vgg_layers(N, H, W)
  layers += generator_layers(1, 256, 512, 64, 4) + local_enhancer_layers(1, 256, 512, 32, 4)
  for N in (1, 2):
    layers += patchgan_layers(N, 256, 512) + vgg_layers(N, 256, 512)
  layers += test_cases()
  seen, out = set(), []
  for dt in (BF16, F32):
    for (N, H, W, C, K, k, st, pad, mode, act) in layers:
      key = (dt, N, H, W, C, K, k, k, st, pad, mode, act)
      if key not in seen:
        seen.add(key)
        out.append(key)
  return out


def query(L, key):
  """The answers for one descriptor, as a flat list of ints (-1 / zeros where the descriptor is refused)."""
  d = ConvDesc(*key, SLOPE)
  plan = (ctypes.c_int32 * 54)()
  rc = L.jpdse_conv_plan_query(ctypes.byref(d), plan, 54)
  ents = (jpdse_hip.PackEntry * 8)()
  n_ent = L.jpdse_conv_pack_entries(ctypes.byref(d), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x10000000), ents, 8)
  return [rc] + list(plan) + [L.jpdse_conv_workspace_size(ctypes.byref(d)), L.jpdse_conv_fwd_pack_size(ctypes.byref(d)),
                              L.jpdse_conv_dgrad_pack_size(ctypes.byref(d)), L.jpdse_conv_moment_slots(ctypes.byref(d)),
                              L.jpdse_convT_moment_slots(ctypes.byref(d)), L.jpdse_conv_dgrad_nsum_slots(ctypes.byref(d)), n_ent]


ANSWER_FIELDS = ['plan_query_rc'] + ['plan[%d]' % i for i in range(54)] + [
    'workspace_size', 'fwd_pack_size', 'dgrad_pack_size', 'moment_slots', 'convT_moment_slots', 'dgrad_nsum_slots', 'pack_entries']


def main(path):
  L = jpdse_hip.lib()
  cases = [[list(k), query(L, k)] for k in all_descriptors()]
  with open(path, 'w') as f:
    f.write('{"descriptor_fields": %s,\n "slope": %s,\n "answer_fields": %s,\n "cases": [\n'
            % (json.dumps(DESC_FIELDS), SLOPE, json.dumps(ANSWER_FIELDS)))
    f.write(',\n'.join(json.dumps(c, separators=(',', ':')) for c in cases))
    f.write('\n]}\n')
  print('%d descriptors -> %s (library: %s)' % (len(cases), path, jpdse_hip.LIB_PATH))


if __name__ == '__main__':
  main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'conv_host_queries.json'))
