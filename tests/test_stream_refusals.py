"""Host test: what the host half of the coded streams accepts and refuses is what tests/golden/stream_refusals.json pins
(scripts/make_stream_refusals.py, generated on the commit before jpdse_hip/streams.py and ctu/utils/container.py of DESIGN.md
4.18): the four containers and the payload rules and pre-library refusals of the three device coders -- every case raises the
same exception type with the same full message, returns the same bytes, or gets as far as the device or the library, exactly
where it did.  No GPU."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'stream_refusals.json')
SURFACES = ['bitstream.', 'entropy.', 'semantics.', 'vqstream.', 'length_table_size/', 'check_length_table/', 'semantics_check_entry/',
            'code_entropy_decode/', 'semantics_decode/', 'semantics_encode/', 'vq_index_decode/', 'vq_index_encode/', 'vq_index_bits/']


def _load(name):
  spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'scripts', name + '.py'))
  module = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(module)
  return module


@pytest.fixture(scope='module')
def tables():
  with open(GOLDEN) as f:
    pinned = [tuple(row) for row in json.load(f)]
  return pinned, [tuple(row) for row in _load('make_stream_refusals').run()]


def test_every_case_is_replayed(tables):
  pinned, got = tables
  assert [row[0] for row in got] == [row[0] for row in pinned] and len(set(row[0] for row in pinned)) == len(pinned)
  assert len(pinned) >= 150 and all(any(row[0].startswith(s) for s in SURFACES) for row in pinned)
  kinds = {row[1] for row in pinned}
  assert {'ValueError', 'returned'} <= kinds
  assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'codec_refusals.json'))


@pytest.mark.parametrize('surface', SURFACES)
def test_outcomes_are_the_pinned_ones(tables, surface):
  pinned, got = tables
  want = [row for row in pinned if row[0].startswith(surface)]
  have = [row for row in got if row[0].startswith(surface)]
  assert len(want) > 0 and len(want) == len(have)
  different = [(w, h) for w, h in zip(want, have) if w != h]
  assert not different, 'first of %d: pinned %r, got %r' % (len(different), different[0][0], different[0][1])
