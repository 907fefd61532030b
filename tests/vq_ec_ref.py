"""float64 torch restatement of the entropy-constrained assignment: the cost, the arg-min with the lowest index
on equal cost, the code lengths of a histogram, and the iteration of S2HVQ.encode_ec.  CPU only; what tests/test_hip_vq_ec.py
and tests/test_vq_ec_host.py compare against."""
import math

import torch

INF = float('inf')


def scores(x, c):
  """d[m][k] = sum_j (x[m][j] - c[k][j])^2 in float64."""
  x, c = x.to(torch.float64), c.to(torch.float64)
  return ((x[:, None, :] - c[None, :, :]) ** 2).sum(dim=-1)


def cost(x, c, bias, G):
  """J[m][k] = d[m][k] + bias[m % G][k] in float64; bias None: zeros."""
  d = scores(x, c)
  if bias is None:
    return d
  g = torch.arange(d.shape[0]) % G
  return d + bias.to(torch.float64)[g]


def argmin_lowest(J):
  """The column of the smallest entry of every row, the lowest on a tie; a row of +inf alone gives 0."""
  low = J.min(dim=-1, keepdim=True).values
  L = J.shape[1]
  cols = torch.arange(L).expand_as(J)
  return torch.where(J == low, cols, torch.full_like(cols, L)).min(dim=-1).values


def hist_of(index, G, L):
  """int64 [G, L]: the counts of index per group m % G."""
  g = torch.arange(index.numel()) % G
  return torch.bincount(g * L + index.to(torch.int64), minlength=G * L).view(G, L)


def sse_of(x, c, index, G):
  """float64 [G]: the sum of the chosen d per group."""
  d = scores(x, c).gather(1, index.to(torch.int64)[:, None])[:, 0]
  g = torch.arange(index.numel()) % G
  return torch.zeros(G, dtype=torch.float64).index_add_(0, g, d)


def lengths(hist, lam):
  """(bias float64 [G, L], bits float64 [G]): bias = lam (log2 n - log2 hist), +inf on an empty bin, zeros at lam == 0; bits =
  sum_k hist (log2 n - log2 hist)."""
  h = hist.to(torch.float64)
  n = h.sum(dim=-1, keepdim=True)
  used = h > 0
  ln = torch.where(used, torch.log2(n) - torch.log2(torch.where(used, h, torch.ones_like(h))), torch.zeros_like(h))
  bits = (h * ln).sum(dim=-1)
  if lam == 0:
    return torch.zeros_like(h), bits
  return torch.where(used, lam * ln, torch.full_like(h, INF)), bits


def assign(x, c, bias, G):
  """(index, hist, sse) of one assignment."""
  L = c.shape[0]
  index = argmin_lowest(cost(x, c, bias, G))
  return index, hist_of(index, G, L), sse_of(x, c, index, G)


def encode_ec(x, c, lam, G, n_iter):
  """(index, report) of the iteration: round 0 without a bias, round t under the lengths of round t - 1."""
  index, hist, sse = assign(x, c, None, G)
  dist, bits = [float(sse.sum())], []
  for _ in range(n_iter):
    bias, b = lengths(hist, lam)
    bits.append(float(b.sum()))
    index, hist, sse = assign(x, c, bias, G)
    dist.append(float(sse.sum()))
  bits.append(float(lengths(hist, lam)[1].sum()))
  return index, dict(distortion=dist, bits=bits, cost=[d + lam * b for d, b in zip(dist, bits)])


def slack(D, J):
  """The fp32 rounding of a cost J = d + bias from the score loop of D terms plus one add: 2 (D + 2) 2^-24 J."""
  return 2.0 * (D + 2) * math.ldexp(1.0, -24) * J
