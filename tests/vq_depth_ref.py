"""Reference of the residual quantizer with a stage depth per cell (include/jpdse.h, "a stage depth per cell"),
restated on tests/vq_residual_ref.py: the depth-map rule in numpy, the per-row forward, the per-row recursion of the backward with
its masked code-book sums, and the surrogate whose autograd is that recursion's oracle.  Works in the dtype of its inputs; the GPU
tests use float64."""
import numpy as np
import torch

import vq_bottleneck_ref
import vq_residual_ref


def depth_map(label, table, default, step):
  """int64 numpy [N, H / step, W / step]: the maximum over a cell's step x step pixels of table[class]; the class of a pixel is its
  label when that is an integer in [0, len(table)), any other pixel (NaN included) takes `default`."""
  lab = np.asarray(label, dtype=np.float32)
  N, _, H, W = lab.shape
  table = np.asarray(table, dtype=np.int64)
  with np.errstate(invalid='ignore'):
    inside = (lab >= 0) & (lab < np.float32(len(table))) & (lab == np.floor(lab))
  k = np.where(inside, lab, 0).astype(np.int64)
  per_pixel = np.where(inside, table[k] if len(table) else 0, int(default))[:, 0]
  return per_pixel.reshape(N, H // step, step, W // step, step).max(axis=(2, 4)).astype(np.int64)


def row_stages(depth, G, n, S):
  """int64 tensor [M]: n_m = min(n, depth[m // G] clamped to 1 .. S)."""
  d = torch.as_tensor(np.asarray(depth).reshape(-1), dtype=torch.int64).clamp(1, S).clamp(max=n)
  return d.repeat_interleave(G)


def forward(x_m, books, nm, follow=None):
  """(y, index int64 [n, M] with -1 past a row's depth, decided [M]), n = max(nm): row m by vq_residual_ref.forward with n_stages
  = nm[m], one call per depth value on the rows that have it."""
  n = int(nm.max())
  M = x_m.shape[0]
  y = torch.zeros_like(x_m)
  index = torch.full((n, M), -1, dtype=torch.int64)
  decided = torch.ones(M, dtype=torch.bool)
  for v in sorted(set(nm.tolist())):
    rows = nm == v
    yv, iv, _, _, dv = vq_residual_ref.forward(x_m[rows], books, v, None if follow is None else follow[:v][:, rows])
    y[rows], decided[rows] = yv, dv
    index[:v, rows] = iv
  return y, index, decided


def bwd(dy, x_m, books, index, sigma, nm):
  """(dx, dbooks [n, L, D]) by the stated recursion (no autograd), n = index.shape[0]: stages descending, h = 0 above a row's
  depth, a_s = dy - h_{s+1}, the one-stage backward (vq_bottleneck_ref.quantize_bwd) at r_s over the rows with nm > s ONLY,
  h_s = h_{s+1} + u_s on those rows, dx = h_1.  A stage without a row gets zeros."""
  n = index.shape[0]
  h = torch.zeros_like(x_m)
  dbooks = torch.zeros((n,) + tuple(books.shape[1:]), dtype=x_m.dtype)
  for s in reversed(range(n)):
    rows = nm > s
    if not bool(rows.any()):
      continue
    r = x_m[rows].clone()
    for u in range(s):
      r = r - books[u][index[u][rows]]
    a = dy[rows] - h[rows]
    us, dbooks[s] = vq_bottleneck_ref.quantize_bwd(a, r, books[s], sigma)
    h[rows] = h[rows] + us
  return h, dbooks


def surrogate(x_m, books, sigma, nm):
  """y of the straight-through surrogate with a depth per row: stage s adds its q and hands r - q on only where nm > s."""
  r = x_m
  y = torch.zeros_like(x_m)
  for s in range(int(nm.max())):
    on = (nm > s).to(x_m.dtype).unsqueeze(1)
    d = ((r.unsqueeze(1) - books[s]) ** 2).sum(-1)
    q_soft = torch.softmax(-sigma * d, -1) @ books[s]
    q = (q_soft + (books[s][d.argmin(-1)] - q_soft).detach()) * on
    y = y + q
    r = r - q
  return y


def grads(dy, x_m, books, sigma, nm):
  """(dx, dbooks [S, L, D]) of surrogate() for the upstream gradient dy, by autograd."""
  x = x_m.clone().requires_grad_(True)
  c = books.clone().requires_grad_(True)
  surrogate(x, c, sigma, nm).backward(dy)
  return x.grad, c.grad if c.grad is not None else torch.zeros_like(books)
