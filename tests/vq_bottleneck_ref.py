"""Torch restatement of the vector-quantizer bottleneck (include/jpdse.h, "vector-quantizer bottleneck"), written
from its definitions on top of tests/vq_util.py.  Works in the dtype of its inputs; the GPU tests run it in float64.  x_m is the
[M, D] matrix of vectors, c the [L, D] code book."""
import torch

import vq_util


def quantize_fwd(x_m, c, sigma, hard_forward=True):
  """(y, index, pmf): index the nearest centre (lowest on a tie), y = c[index] or sum_k p[m][k] c[k], pmf the column means
  of the soft assignment p."""
  index = vq_util.hard_index(x_m, c)
  p = vq_util.soft(x_m, c, sigma)
  y = vq_util.decode(index, c) if hard_forward else p @ c
  return y, index, vq_util.pmf(p)


def soft_value(x_m, c, sigma):
  """(y, pmf) of the soft form as differentiable torch expressions: what the backward is the gradient of."""
  p = vq_util.soft(x_m, c, sigma)
  return p @ c, vq_util.pmf(p)


def quantize_bwd(dy, x_m, c, sigma, dpmf=None):
  """(dx, dC) of the soft form by the stated formulas (no autograd):
    dp = <dy, c_k> + dpmf[k] / M,  g = p (dp - <p, dp>),  dd = -sigma g,
    dx = 2 sum_k dd (x - c_k),  dC[k] = sum_m (p dy - 2 dd (x - c_k))."""
  M = x_m.shape[0]
  p = vq_util.soft(x_m, c, sigma)
  dp = dy @ c.t()
  if dpmf is not None:
    dp = dp + dpmf.unsqueeze(0) / M
  dx, dc_through_d = vq_util.soft_bwd(dp, p, x_m, c, sigma)          # dc_through_d = -2 sum_m dd (x - c)
  return dx, p.t() @ dy + dc_through_d
