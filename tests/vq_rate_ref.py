"""Torch restatement of the rate term on per-group histograms (include/jpdse.h, "the rate term on per-group histograms";
DESIGN.md 4.16), written from its definitions on top of tests/vq_util.py.  Works in the dtype of its inputs and is
differentiable; the GPU tests run it in float64.  x_m is the [M, D] matrix of vectors, c the [L, D] code book; vector m belongs
to group m % G."""
import math

import torch

import vq_util


def assignment(x_m, c, sigma, hard=False):
  """p [M, L]: the soft assignment, or the one-hot of the nearest centre (lowest on a tie)."""
  if hard:
    return vq_util.onehot(vq_util.hard_index(x_m, c), c.shape[0], x_m.dtype)
  return vq_util.soft(x_m, c, sigma)


def hist_of(p, G):
  """hist[g][k] = sum over m with m % G == g of p[m][k]."""
  M, L = p.shape
  return p.view(M // G, G, L).sum(dim=0)


def rate_of_hist(hist, n, denom):
  """-sum hist log2(hist / n) / denom over the entries with hist > 0."""
  keep = hist > 0
  return -(hist[keep] * torch.log2(hist[keep] / n)).sum() / denom


def rate(x_m, c, sigma, G, denom, hard=False):
  """(rate, hist): differentiable in x_m and c (hard: a constant)."""
  hist = hist_of(assignment(x_m, c, sigma, hard), G)
  return rate_of_hist(hist, x_m.shape[0] // G, denom), hist


def dhist_of(hist, n, denom, scale=1.0):
  """scale * d rate / d hist by the stated formula (no autograd): -(log2 q + 1 / ln 2) / denom where hist > 0, else 0."""
  q = hist / n
  safe = torch.where(hist > 0, q, torch.ones_like(q))
  return torch.where(hist > 0, scale * (-(torch.log2(safe) + 1.0 / math.log(2.0))) / denom, torch.zeros_like(q))


def quantize_bwd_grouped(dy, x_m, c, sigma, G, dhist=None):
  """(dx, dC) of the soft form with dp[m][k] = <dy[m], c[k]> + dhist[m % G][k]; everything after dp is 4.15's."""
  M = x_m.shape[0]
  p = vq_util.soft(x_m, c, sigma)
  dp = dy @ c.t()
  if dhist is not None:
    dp = dp + dhist.repeat(M // G, 1)
  dx, dc_through_d = vq_util.soft_bwd(dp, p, x_m, c, sigma)
  return dx, p.t() @ dy + dc_through_d
