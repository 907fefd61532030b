#!/usr/bin/env python3
"""Compares the dispatch lists of two `rocprofv3 --kernel-trace` runs of the same program (two builds of the library): the
ordered list of (kernel name, grid, workgroup size, LDS bytes) must be identical.  This sees every launch geometry the host
layer computes, which a comparison of the code objects (scripts/diff_code_objects.py) cannot.

  python scripts/compare_kernel_traces.py A_kernel_trace.csv B_kernel_trace.csv

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


def main(a_path, b_path):
  a, cols = dispatches(a_path)
  b, _ = dispatches(b_path)
  print('%d dispatches in A, %d in B, %d distinct kernels in A; compared: name, %s' % (len(a), len(b), len({d[0] for d in a}), ', '.join(cols)))
  bad = [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y]
  for i, x, y in bad[:20]:
    print('  dispatch %d differs:\n    A %s\n    B %s' % (i, x, y))
  same = not bad and len(a) == len(b)
  print('dispatch lists: ' + ('IDENTICAL (order, kernel, grid, workgroup, LDS)' if same else '%d differences' % (len(bad) + abs(len(a) - len(b)))))
  return 0 if same else 1


if __name__ == '__main__':
  if len(sys.argv) != 3:
    sys.exit(__doc__)
  sys.exit(main(sys.argv[1], sys.argv[2]))
