#!/usr/bin/env python3
"""Writes tests/golden/conv_routes.json: the route (jpd-se_amd/csrc/conv_route.h: the kernel family) that the forward, the data
gradient and the weight gradient of every layer of scripts/make_conv_host_queries.py take under the shipped dispatch, by name
(tests/test_host_conv_routes.py replays it).  Asked of the developer build (jpdse_debug_conv_route, mode 1, no wants); nothing
is launched, so this runs without a GPU.

  python scripts/make_conv_routes.py [OUT.json]

The file holds the dispatch still, layer by layer: regenerate it ONLY with a change that means to move a layer to another
kernel, and say so in that change."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'jpd-se_amd'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

import jpdse_hip                                                               # noqa: E402
import make_conv_host_queries as gen                                           # noqa: E402

# jpdse_debug_conv_route flags (include/jpdse_dev.h)
FWD_MOMENTS, FWD_POOL, DGRAD_MASK, DGRAD_ADDEND, DGRAD_LRELU, DGRAD_MOMENTS, DGRAD_NSUMS = 1, 2, 4, 8, 16, 32, 64


def routes(dev, key, flags=0):
  """[forward, data-gradient, weight-gradient] route names of one descriptor under the developer library's current mode."""
  d = jpdse_hip.ConvDesc(*key, gen.SLOPE)
  out = (ctypes.c_int32 * 3)()
  jpdse_hip.check(dev.jpdse_debug_conv_route(ctypes.byref(d), flags, out), 'jpdse_debug_conv_route')
  return [dev.jpdse_debug_route_name(i, out[i]).decode() for i in range(3)]


def main(path):
  with jpdse_hip.dev_mode(1) as dev:
    cases = [[list(k), routes(dev, k)] for k in gen.all_descriptors()]
  with open(path, 'w') as f:
    f.write('{"descriptor_fields": %s,\n "route_fields": ["fwd", "dgrad", "wgrad"],\n "cases": [\n' % json.dumps(gen.DESC_FIELDS))
    f.write(',\n'.join(json.dumps(c, separators=(',', ':')) for c in cases))
    f.write('\n]}\n')
  print('%d descriptors -> %s' % (len(cases), path))


if __name__ == '__main__':
  main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'conv_routes.json'))
