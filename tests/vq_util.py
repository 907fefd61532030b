"""Torch-CPU restatement of the soft-to-hard vector quantizer, written from the arithmetic of DESIGN.md 4.13 (include/jpdse.h,
"soft-to-hard vector quantizer").  Works in the dtype of its inputs: float32 against tests/golden/s2hvq.npz, float64 as the
reference of the GPU tests.  x_m is the [M, D] matrix of vectors, c the [L, D] code book."""
import torch


def scores(x_m, c):
  """d[m][k] = sum_j (x[m][j] - c[k][j])^2: the direct form."""
  return ((x_m.unsqueeze(1) - c.unsqueeze(0)) ** 2).sum(dim=-1)


def soft(x_m, c, sigma):
  d = scores(x_m, c)
  return torch.softmax(-sigma * (d - d.min(dim=-1, keepdim=True).values), dim=-1)


def _lowest(hit):
  """Per row, the lowest column where `hit` is true."""
  L = hit.shape[-1]
  cols = torch.arange(L).expand_as(hit)
  return torch.where(hit, cols, torch.full_like(cols, L)).min(dim=-1).values


def hard_index(x_m, c):
  """The nearest centre, the lowest index on a tie."""
  d = scores(x_m, c)
  return _lowest(d == d.min(dim=-1, keepdim=True).values)


def argmax_lowest(s):
  return _lowest(s == s.max(dim=-1, keepdim=True).values)


def onehot(index, L, dtype=torch.float32):
  out = torch.zeros((index.numel(), L), dtype=dtype)
  out[torch.arange(index.numel()), index.view(-1)] = 1
  return out


def decode(index, c):
  return c[index]


def pmf(s):
  s = s.reshape(-1, s.shape[-1])
  return s.sum(dim=0) / s.shape[0]


def cross_entropy(pmf1, pmf2):
  keep = pmf2 > 0
  return (-pmf1[keep] * torch.log2(pmf2[keep])).sum()


def soft_bwd(dp, p, x_m, c, sigma):
  """(dx, dC) of soft() for the upstream gradient dp, by the stated formulas (no autograd)."""
  g = p * (dp - (p * dp).sum(dim=-1, keepdim=True))
  dd = -sigma * g
  diff = x_m.unsqueeze(1) - c.unsqueeze(0)                 # [M, L, D]
  dx = 2 * (dd.unsqueeze(-1) * diff).sum(dim=1)
  dc = -2 * (dd.unsqueeze(-1) * diff).sum(dim=0)
  return dx, dc


def decode_bwd(index, dy, L):
  return torch.zeros((L, dy.shape[1]), dtype=dy.dtype).index_add_(0, index.view(-1).long(), dy)


# ---- the module's surface on [n, d] inputs -----------------------------------------------------------------------------------
def encode(x, c, code_len, sigma, train=True, raw=True):
  n, L, D = x.shape[0], c.shape[0], c.shape[1]
  x_m = x.reshape(n * code_len, D)
  if train:
    p = soft(x_m, c, sigma)
    return p.view(n, code_len, L) if raw else argmax_lowest(p).view(n, code_len)
  index = hard_index(x_m, c)
  return onehot(index, L, x.dtype).view(n, code_len, L) if raw else index.view(n, code_len)


def decode_raw(code_raw, c):
  n, code_len, L = code_raw.shape
  return decode(argmax_lowest(code_raw.reshape(-1, L)), c).view(n, code_len * c.shape[1])


def golden_loss(x, c, code_len, sigma, r, q):
  """The loss of the fixture: sum(code_raw * r) + sum(decode(code_raw) * q) on the soft code."""
  code_raw = encode(x, c, code_len, sigma)
  return (code_raw * r).sum() + (decode_raw(code_raw, c) * q).sum()
