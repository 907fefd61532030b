#!/usr/bin/env python3
"""Compares the dispatch lists of two `rocprofv3 --kernel-trace` runs of the same program (two builds of the library): the
ordered list of (kernel name, grid, workgroup size, LDS bytes) must be identical.  This sees every launch geometry the host
layer computes, which a comparison of the code objects (scripts/diff_code_objects.py) cannot.

  python scripts/compare_kernel_traces.py [--rename FILE] A_kernel_trace.csv B_kernel_trace.csv

--rename FILE: the output of `scripts/diff_code_objects.py --match-by-content` (its `renamed:<TAB>old<TAB>new` lines); side A's
kernel names are translated through that table before the comparison.

Dispatches are ordered by dispatch id (the order the host enqueued them).  Exit status 0 when the lists are equal, 1 otherwise."""
import csv
import sys


def dispatches(path):
  with open(path, newline='') as f:
    rows = list(csv.DictReader(f))
  assert rows, path + ': no dispatches'
  cols = list(rows[0].keys())
  low = {c.lower(): c for c in cols}
  order = low.get('dispatch_id') or low['start_timestamp']
  geometry = [c for c in cols if c.lower().startswith(('grid_size', 'workgroup_size'))] + [low['lds_block_size']]
  assert len(geometry) == 7, 'unexpected columns: %s' % cols
  rows.sort(key=lambda r: int(r[order]))
  return [(r[low['kernel_name']],) + tuple(int(r[c]) for c in geometry) for r in rows], geometry


def main(a_path, b_path, rename_path=None):
  a, cols = dispatches(a_path)
  if rename_path:
    with open(rename_path) as f:
      table = dict(l.rstrip('\n').split('\t')[1:3] for l in f if l.startswith('renamed:\t'))
    stem = lambda n: n[:-3] if n.endswith('.kd') else n           # some rocprofv3 versions keep the descriptor suffix
    print('%d of %d dispatches of A renamed' % (sum(stem(d[0]) in table for d in a), len(a)))
    a = [(table.get(stem(d[0]), stem(d[0])) + d[0][len(stem(d[0])):],) + d[1:] for d in a]
  b, _ = dispatches(b_path)
  print('%d dispatches in A, %d in B, %d distinct kernels in A; compared: name, %s' % (len(a), len(b), len({d[0] for d in a}), ', '.join(cols)))
  bad = [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y]
  for i, x, y in bad[:20]:
    print('  dispatch %d differs:\n    A %s\n    B %s' % (i, x, y))
  same = not bad and len(a) == len(b)
  print('dispatch lists: ' + ('IDENTICAL (order, kernel, grid, workgroup, LDS)' if same else '%d differences' % (len(bad) + abs(len(a) - len(b)))))
  return 0 if same else 1


if __name__ == '__main__':
  args = sys.argv[1:]
  rename = args.pop(args.index('--rename') + 1) if '--rename' in args[:-1] else None
  args = [a for a in args if a != '--rename']
  if len(args) != 2:
    sys.exit(__doc__)
  sys.exit(main(args[0], args[1], rename))
