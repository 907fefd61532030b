"""Torch-CPU reference of the residual vector quantizer (include/jpdse.h, "residual vector quantizer"): the plain
forward and the surrogate whose autograd is the gradient's oracle.  Works in the dtype of its inputs; the GPU tests use float64.
x_m is the [M, D] matrix of vectors, books the [S, L, D] code books."""
import torch

import vq_util

GAP = 1e-5      # the rule of tests/test_hip_vq_bottleneck.py: a row whose two best scores differ by less than GAP * the best is undecided


def forward(x_m, books, n_stages=None, follow=None):
  """(y, index [n, M], sse [n], residual, decided [M]) of the first n_stages stages.  decided[m]: at every stage the nearest
  centre of row m is ahead of the runner-up by more than GAP times its score; a row is undecided from the first stage where
  it is not.  follow (int64 [n, M]): take these indices instead of the arg-min on the rows that are NOT decided -- what the
  sums over all rows (sse) are measured against, the device's choice on an undecided row being as good as any."""
  n = books.shape[0] if n_stages is None else int(n_stages)
  r = x_m.clone()
  y = torch.zeros_like(x_m)
  decided = torch.ones(x_m.shape[0], dtype=torch.bool)
  index, sse = [], []
  for s in range(n):
    d = vq_util.scores(r, books[s])
    k = vq_util.hard_index(r, books[s])
    two = torch.topk(d, 2, dim=-1, largest=False).values
    decided = decided & ((two[:, 1] - two[:, 0]) > GAP * two[:, 0])
    if follow is not None:
      k = torch.where(decided, k, follow[s])
    c = books[s][k]
    y = y + c
    r = r - c
    index.append(k)
    sse.append((r ** 2).sum())
  if n == 0:
    return y, torch.zeros((0, x_m.shape[0]), dtype=torch.int64), torch.zeros(0, dtype=x_m.dtype), r, decided
  return y, torch.stack(index), torch.stack(sse), r, decided


def surrogate(x_m, books, sigma, n_stages=None):
  """y of the straight-through surrogate: the hard forward's value, the soft form's gradient at every stage."""
  n = books.shape[0] if n_stages is None else int(n_stages)
  r = x_m
  y = torch.zeros_like(x_m)
  for s in range(n):
    d = ((r.unsqueeze(1) - books[s]) ** 2).sum(-1)
    q_soft = torch.softmax(-sigma * d, -1) @ books[s]
    q = q_soft + (books[s][d.argmin(-1)] - q_soft).detach()
    y = y + q
    r = r - q
  return y


def grads(dy, x_m, books, sigma, n_stages=None):
  """(dx, dbooks) of surrogate() for the upstream gradient dy, by autograd; dbooks is zero beyond n_stages."""
  x = x_m.clone().requires_grad_(True)
  c = books.clone().requires_grad_(True)
  surrogate(x, c, sigma, n_stages).backward(dy)
  return x.grad, c.grad if c.grad is not None else torch.zeros_like(books)
