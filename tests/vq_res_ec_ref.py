"""A torch-CPU restatement of the entropy-constrained residual code, for the tests that have no device oracle.

    r_1 = x (widened to fp32 once);  cost_s[k] = d(r_s, C_s[k]) + bias[s][m % G][k];  k_s = argmin_k cost_s[k]
    r_{s+1} = r_s - C_s[k_s];  y = C_1[k_1] + .. + C_n[k_n]

d: components ascending, one fused multiply-add each -- emulated as the fp64 value t * t + d (t * t is exact in fp64) rounded to
fp32.  The arg-min is a strict <: the lowest index keeps a tie, a +inf cost never replaces anything, a row of +inf alone gives
index 0.  Histograms by bincount, sse in fp64.  Written from the definition; the reference project has no such code."""
import math

import torch


def scores(r, book):
  """fp32 [M, L]: d(r[m], book[k]) with the kernels' rounding.  r fp32 [M, D], book fp32 [L, D]."""
  M, D = r.shape
  d = torch.zeros(M, book.shape[0], dtype=torch.float32)
  for j in range(D):
    t = (r[:, j:j + 1] - book[:, j].view(1, -1)).to(torch.float64)       # the fp32 difference, widened
    d = (t * t + d.to(torch.float64)).to(torch.float32)
  return d


def argmin_strict(cost):
  """int64 [M]: the first index whose cost is below everything before it, 0 when none is below +inf (NaN-free input)."""
  M, L = cost.shape
  best = torch.full((M,), float('inf'), dtype=cost.dtype)
  bk = torch.zeros(M, dtype=torch.int64)
  for k in range(L):
    better = cost[:, k] < best
    best = torch.where(better, cost[:, k], best)
    bk = torch.where(better, torch.full_like(bk, k), bk)
  return bk


def assign(x, books, bias=None, groups=1, n_stages=None):
  """(y fp32 [M, D], index int64 [n, M], hist int64 [n, G, L], sse fp64 [n, G]) of x [M, D] (any float dtype, widened once),
  books fp32 [S, L, D], bias fp32 [n, G, L] or None."""
  S, L, D = books.shape
  n = S if n_stages is None else n_stages
  M, G = x.shape[0], groups
  r = x.to(torch.float32).clone()
  g = torch.arange(M) % G
  y = None
  index = torch.zeros(n, M, dtype=torch.int64)
  hist = torch.zeros(n, G, L, dtype=torch.int64)
  sse = torch.zeros(n, G, dtype=torch.float64)
  for s in range(n):
    d = scores(r, books[s])
    cost = d if bias is None else d + bias[s][g]
    k = argmin_strict(cost)
    index[s] = k
    hist[s] = torch.bincount(g * L + k, minlength=G * L).view(G, L)
    sse[s] = torch.zeros(G, dtype=torch.float64).index_add_(0, g, d.gather(1, k.view(-1, 1)).view(-1).to(torch.float64))
    c = books[s][k]
    r = r - c
    y = c.clone() if s == 0 else y + c
  return y, index, hist, sse


def lengths(hist, lam):
  """(bias fp32 [.., L], bits fp64 [..]) of counts [.., L]: bias = lam * log2(n / hist) computed in fp64, +inf on an empty bin, exact
  zeros at lam == 0; bits = sum hist * log2(n / hist): ops.vq_ec_lengths, plane by plane."""
  h = hist.to(torch.float64)
  n = h.sum(dim=-1, keepdim=True)
  lgn = torch.where(n > 0, torch.log2(n.clamp(min=1.0)), torch.zeros_like(n))
  ln = lgn - torch.log2(h.clamp(min=1.0))
  bits = torch.where(h > 0, h * ln, torch.zeros_like(h)).sum(dim=-1)
  if lam == 0:
    return torch.zeros(hist.shape, dtype=torch.float32), bits
  bias = torch.where(h > 0, (lam * ln).to(torch.float32), torch.full(hist.shape, float('inf'), dtype=torch.float32))
  return bias, bits


def entropy_bits(hist):
  """Python float per leading index: sum_g sum_k hist log2(n_g / hist) of counts [.., G, L], in fp64 on the host."""
  return lengths(hist, 0.0)[1].sum(dim=-1)


def encode_ec(x, books, lam, groups=1, n_iter=2, n_stages=None):
  """(index int64 [n, M], report, hist) by the rounds of ResidualS2HVQ.encode_ec."""
  _, index, hist, sse = assign(x, books, None, groups, n_stages)
  dist, bits = [sse.sum(1).tolist()], []
  for _ in range(n_iter):
    bias, b = lengths(hist, lam)
    bits.append(b.sum(1).tolist())
    _, index, hist, sse = assign(x, books, bias, groups, n_stages)
    dist.append(sse.sum(1).tolist())
  bits.append(lengths(hist, lam)[1].sum(1).tolist())
  cost = [d[-1] + lam * math.fsum(b) for d, b in zip(dist, bits)]
  return index, dict(distortion=dist, bits=bits, cost=cost), hist
