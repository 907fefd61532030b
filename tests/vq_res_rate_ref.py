"""Torch restatement of the rate term of the residual vector quantizer (include/jpdse.h, "residual vector quantizer: the rate
term"), written from its definitions on tests/vq_residual_ref.py (the hard chain, with `follow`), tests/vq_rate_ref.py
(the one-stage histogram, entropy, dhist and grouped backward) and tests/vq_util.py.  Works in the dtype of its inputs; the tests
run it in float64.  x_m is the [M, D] matrix of vectors, books the [S, L, D] code books; vector m belongs to group m % G."""
import torch

import vq_util
import vq_rate_ref
import vq_residual_ref as res


def chain(x_m, books, n_stages=None, follow=None):
  """(index int64 [n, M], decided [M]) of the hard forward: vq_residual_ref.forward's, `follow` included."""
  _, index, _, _, decided = res.forward(x_m.detach(), books.detach(), n_stages, follow)
  return index, decided


def residuals(x_m, books, index):
  """[r_1 .. r_n]: r_1 = x, r_{s+1} = r_s - C_s[index[s]] -- values only, no gradient path through the centres."""
  out, r = [], x_m
  for s in range(index.shape[0]):
    out.append(r)
    r = r - books[s][index[s]]
  return out


def rate(x_m, books, sigma, G, denom, n_stages=None, follow=None):
  """(rate, rates [n], hist [n, G, L], index): the stated formulas at the hard residuals.  Not differentiable through the chain:
  the gradient's oracle is loss() below."""
  index, _ = chain(x_m, books, n_stages, follow)
  M = x_m.shape[0]
  rates, hists = [], []
  for s, r in enumerate(residuals(x_m, books, index)):
    hist = vq_rate_ref.hist_of(vq_util.soft(r, books[s], sigma), G)
    hists.append(hist)
    rates.append(vq_rate_ref.rate_of_hist(hist, M // G, denom))
  total = rates[0]
  for v in rates[1:]:
    total = total + v                           # stage order
  return total, torch.stack(rates), torch.stack(hists), index


def dhist_of(hist, n, denom, scale=1.0):
  """[n_stages, G, L]: vq_rate_ref.dhist_of per stage."""
  return torch.stack([vq_rate_ref.dhist_of(h, n, denom, scale) for h in hist])


def loss(x_m, books, sigma, G, denom, dy, scale, n_stages=None, follow=None):
  """sum(y * dy) + scale * rate on the SURROGATE of vq_residual_ref.surrogate -- q_s carries the hard value (the centre of the
  hard chain, `follow` included) and the soft gradient -- with p_s evaluated at the surrogate's r_s: what autograd differentiates.
  Its value is the hard forward's."""
  index, _ = chain(x_m, books, n_stages, follow)
  M = x_m.shape[0]
  r, y, total = x_m, torch.zeros_like(x_m), 0.0
  for s in range(index.shape[0]):
    p = vq_util.soft(r, books[s], sigma)
    total = total + vq_rate_ref.rate_of_hist(vq_rate_ref.hist_of(p, G), M // G, denom)
    q_soft = p @ books[s]
    q = q_soft + (books[s][index[s]] - q_soft).detach()
    y = y + q
    r = r - q
  return (y * dy).sum() + scale * total


def grads(dy, x_m, books, sigma, G, denom, scale, n_stages=None, follow=None):
  """(dx, dbooks) of loss() by autograd; dbooks is zero beyond n_stages."""
  x = x_m.clone().requires_grad_(True)
  c = books.clone().requires_grad_(True)
  loss(x, c, sigma, G, denom, dy, scale, n_stages, follow).backward()
  return x.grad, c.grad if c.grad is not None else torch.zeros_like(books)


def bwd_grouped(dy, x_m, books, index, sigma, G, dhist=None):
  """(dx, dbooks [n, L, D]) by the stated recursion (no autograd): stages descending, a_s = dy - h_{s+1}, the one-stage grouped
  backward (vq_rate_ref.quantize_bwd_grouped) at r_s with dp = <a_s, C_s[k]> + dhist[s][m % G][k], h_s = h_{s+1} + u_s, dx = h_1."""
  rs = residuals(x_m, books, index)
  h = torch.zeros_like(x_m)
  dbooks = [None] * len(rs)
  for s in reversed(range(len(rs))):
    a = dy - h
    u, dbooks[s] = vq_rate_ref.quantize_bwd_grouped(a, rs[s], books[s], sigma, G, dhist[s] if dhist is not None else None)
    h = h + u
  return h, torch.stack(dbooks)
