"""Generate tests/golden/s2hvq.npz from the REAL reference's S2HVQ (build container only: it needs the reference tree; its
ctu/quantizers/s2h_vq.py is loaded by path, the module imports nothing but numpy and torch).  Torch-CPU, float32.

Per configuration i (n, d, code_len, L, sigma), all seeded:
  c{i}_cfg                      the five numbers
  c{i}_x, c{i}_code_book        inputs
  c{i}_soft, c{i}_hard          encode(train=True / False, raw=True)
  c{i}_soft_code, c{i}_hard_code   encode(raw=False), int64
  c{i}_decode, c{i}_decode_hard decode(soft) / decode(hard)
  c{i}_pmf, c{i}_pmf_hard       get_pmf(soft) / get_pmf(hard)
  c{i}_xent                     get_cross_entropy(pmf, pmf) and get_cross_entropy(pmf_hard, pmf)
  c{i}_r, c{i}_q                upstream weights of the loss sum(soft * r) + sum(decode(soft) * q)
  c{i}_gx, c{i}_gc, c{i}_gpmf_x the gradients of that loss in x and the code book, and of sum(get_pmf(soft) * arange(L)) in x

Inputs are normal deviates times (sigma * D)^-1/2, so the logits sigma * d are of order 1: the regime the soft assignment is
trained in.  A float32 logit carries an absolute error of about 6e-8 * sigma * d, which is the relative error of every small
entry of the softmax and of the gradients; with unit-variance inputs at sigma = 10 the reference's own float32 result is
only good to 1e-5, and a fixture cannot pin another grouping of the same operations to 1e-6 there.

Run:  python scripts/make_golden_s2hvq.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from oracle import _refbridge  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 's2hvq.npz')
# (n, d, code_len, L, sigma)
CONFIGS = [(5, 15, 3, 10, 1.0), (2, 8, 8, 2, 10.0), (3, 48, 3, 7, 10.0), (4, 12, 4, 10, 1.0)]


def reference_class():
  if not _refbridge.available():
    raise RuntimeError('reference tree not present (expected only in the build container)')
  path = os.path.join(_refbridge.REFERENCE_ROOT, 'ctu', 'quantizers', 's2h_vq.py')
  spec = importlib.util.spec_from_file_location('_ref_s2h_vq', path)
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod.S2HVQ


def main():
  S2HVQ = reference_class()
  torch.set_num_threads(1)
  out = {}
  for i, (n, d, code_len, L, sigma) in enumerate(CONFIGS):
    g = torch.Generator().manual_seed(4100 + i)
    D = d // code_len
    scale = (sigma * D) ** -0.5
    x = torch.randn(n, d, generator=g) * scale
    book = torch.randn(L, D, generator=g) * scale
    r = torch.randn(n, code_len, L, generator=g)
    q = torch.randn(n, d, generator=g)
    vq = S2HVQ(book.clone(), sigma=sigma)
    xg = x.clone().requires_grad_(True)
    soft = vq.encode(xg, code_len)
    dec = vq.decode(soft)
    loss = (soft * r).sum() + (dec * q).sum()
    loss.backward()
    gx, gc = xg.grad.clone(), vq.code_book.grad.clone()
    xg2 = x.clone().requires_grad_(True)
    pm = S2HVQ.get_pmf(vq.encode(xg2, code_len))
    (pm * torch.arange(L, dtype=torch.float32)).sum().backward()
    with torch.no_grad():
      hard = vq.encode(x, code_len, train=False)
      pmf_hard = S2HVQ.get_pmf(hard)
      rec = {'cfg': np.array([n, d, code_len, L, sigma], dtype=np.float64), 'x': x, 'code_book': book, 'soft': soft, 'hard': hard,
             'soft_code': vq.encode(x, code_len, raw=False), 'hard_code': vq.encode(x, code_len, train=False, raw=False),
             'decode': dec, 'decode_hard': vq.decode(hard), 'pmf': pm, 'pmf_hard': pmf_hard,
             'xent': torch.stack([S2HVQ.get_cross_entropy(pm, pm), S2HVQ.get_cross_entropy(pmf_hard, pm)]),
             'r': r, 'q': q, 'gx': gx, 'gc': gc, 'gpmf_x': xg2.grad}
    for k, v in rec.items():
      out['c%d_%s' % (i, k)] = v.detach().numpy() if torch.is_tensor(v) else v
  np.savez_compressed(OUT, **out)
  print('wrote %s: %d arrays, %d bytes' % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == '__main__':
  main()
