"""CPU-only guard of the host-side conv decisions: for every conv / ConvTranspose layer of the product (the three bench
configurations, both PatchGAN scales, VGG19, the 2048x1024 sizes, the shapes tests/test_hip_ops.py parametrises; bf16 and
fp32) the library's query entry points must answer what tests/golden/conv_host_queries.json recorded -- plan, workspace and
panel sizes, moment / norm-sum slot counts, repack-table length.  Those answers come from the predicates that choose a layer's
kernel (halo_ok, taps4_shape_ok, taps9_splits, thin1_shape_ok, the dry run of the weight-gradient dispatch, ...), so a change
of the host layer that moves a layer to another kernel or resizes a workspace region shows up here, without a GPU.  The
fixture is written by scripts/make_conv_host_queries.py; nothing is launched."""
import json
import os
import sys

import jpdse_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))


def test_conv_host_queries_match_the_recorded_answers():
  import make_conv_host_queries as gen
  fix = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'conv_host_queries.json')))
  assert fix['descriptor_fields'] == gen.DESC_FIELDS and fix['answer_fields'] == gen.ANSWER_FIELDS and fix['slope'] == gen.SLOPE
  # the fixture covers the list the generator would write today (a layer added there needs a regenerated fixture)
  assert [tuple(c[0]) for c in fix['cases']] == gen.all_descriptors()
  assert len(fix['cases']) >= 600
  L = jpdse_hip.lib()
  wrong = []
  for key, want in fix['cases']:
    got = gen.query(L, tuple(key))
    if got != want:
      diff = ['%s: %d, recorded %d' % (n, g, w) for n, g, w in zip(gen.ANSWER_FIELDS, got, want) if g != w]
      wrong.append('%s: %s' % (dict(zip(gen.DESC_FIELDS, key)), '; '.join(diff)))
  assert not wrong, '%d of %d descriptors answer differently:\n%s' % (len(wrong), len(fix['cases']), '\n'.join(wrong[:20]))
