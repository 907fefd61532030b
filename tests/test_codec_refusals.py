"""Host test: the refusals of the model's code / decode / file calls are those pinned in tests/golden/codec_refusals.json
(scripts/make_codec_refusals.py, generated on the commit before the codec objects of DESIGN.md 4.17): for no bottleneck, the
binarizer and S2HVQ, every case raises the same exception type with the same full message -- or gets as far as device work,
exactly where it did.  No GPU."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
  spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'scripts', name + '.py'))
  module = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(module)
  return module


@pytest.fixture(scope='module')
def tables():
  with open(os.path.join(ROOT, 'tests', 'golden', 'codec_refusals.json')) as f:
    pinned = [tuple(row) for row in json.load(f)]
  return pinned, [tuple(row) for row in _load('make_codec_refusals').run()]


def test_every_case_is_replayed(tables):
  pinned, got = tables
  assert [row[0] for row in got] == [row[0] for row in pinned] and len(set(row[0] for row in pinned)) == len(pinned)
  kinds = {row[1] for row in pinned}
  assert {'ValueError', 'AssertionError'} <= kinds and 'returned' not in kinds      # nothing runs through on a bare model


@pytest.mark.parametrize('quantizer', ['none', 'binarizer', 's2hvq'])
def test_refusals_are_the_pinned_ones(tables, quantizer):
  pinned, got = tables
  want = [row for row in pinned if row[0].startswith(quantizer + '/')]
  have = [row for row in got if row[0].startswith(quantizer + '/')]
  assert len(want) > 100
  different = [(w, h) for w, h in zip(want, have) if w != h]
  assert not different, 'first of %d: pinned %r, got %r' % (len(different), different[0][0], different[0][1])
