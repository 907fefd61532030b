"""float64 numpy restatement of the context-model rate term (TEST INFRASTRUCTURE), written from the definition
and not from the kernel: the yardstick of tests/test_code_rate_host.py and tests/test_hip_code_rate.py.

For a code b and the tanh output t, both [N, C, h, w] (logical NCHW here; the device tensors are NHWC):
  bit = b > 0;  ctx = left | up << 1 | upleft << 2 | upright << 3 over the bits of the same (n, c) stream, 0 outside the frame
  n1[n, c, k] / n0[n, c, k] = positions with ctx == k and bit 1 / 0
  p1 = (n1 + 1) / (n0 + n1 + 2),  cost1 = -log2(p1),  cost0 = -log2(1 - p1)
  e = (1 + t) / 2 * cost1[ctx] + (1 - t) / 2 * cost0[ctx]
  R = (1 / N) sum_n (1 / pixels) sum_{c, y, x} e
  dR/dt = scale * (cost1[ctx] - cost0[ctx]) / (2 N pixels)        (ctx and the costs are constants)
  hard mode (t None): t = +1 where b > 0, -1 elsewhere."""
import numpy as np


def contexts(b):
  """(bits, ctx): uint8 [N, C, h, w] each."""
  bits = (np.asarray(b) > 0).astype(np.uint8)
  N, C, h, w = bits.shape
  p = np.zeros((N, C, h + 1, w + 2), dtype=np.uint8)       # one row above, one column on either side: zeros
  p[:, :, 1:, 1:w + 1] = bits
  left = p[:, :, 1:, 0:w]
  up = p[:, :, 0:h, 1:w + 1]
  upleft = p[:, :, 0:h, 0:w]
  upright = p[:, :, 0:h, 2:w + 2]
  return bits, left | up << 1 | upleft << 2 | upright << 3


def counts(b):
  """int32 [N, C, 16, 2]: [..., k, 0] = n0, [..., k, 1] = n1."""
  bits, ctx = contexts(b)
  N, C, h, w = bits.shape
  out = np.zeros((N, C, 16, 2), dtype=np.int32)
  for n in range(N):
    for c in range(C):
      idx = ctx[n, c].astype(np.int64).reshape(-1) * 2 + bits[n, c].reshape(-1)
      out[n, c] = np.bincount(idx, minlength=32).reshape(16, 2)
  return out


def costs(cnt):
  """(cost0, cost1): float64 [N, C, 16] each, in bits."""
  n0, n1 = cnt[..., 0].astype(np.float64), cnt[..., 1].astype(np.float64)
  p1 = (n1 + 1.0) / (n0 + n1 + 2.0)
  return -np.log2(1.0 - p1), -np.log2(p1)


def rate(b, t, pixels, scale=1.0):
  """dict(R, per_image [N], grad [N, C, h, w] (already times scale), counts, cost0, cost1, bits_total [N, C]): float64.
  bits_total[n, c] is the stream's expected length in bits, sum of e over its positions."""
  b = np.asarray(b)
  bits, ctx = contexts(b)
  N = b.shape[0]
  cnt = counts(b)
  c0, c1 = costs(cnt)
  k = ctx.astype(np.int64)
  e0 = np.take_along_axis(c0, k.reshape(N, b.shape[1], -1), axis=2).reshape(b.shape)
  e1 = np.take_along_axis(c1, k.reshape(N, b.shape[1], -1), axis=2).reshape(b.shape)
  tt = np.where(bits > 0, 1.0, -1.0) if t is None else np.asarray(t, dtype=np.float64)
  e = (1.0 + tt) / 2.0 * e1 + (1.0 - tt) / 2.0 * e0
  per_image = e.sum(axis=(1, 2, 3)) / float(pixels)
  return dict(R=per_image.sum() / N, per_image=per_image, grad=scale * (e1 - e0) / (2.0 * N * float(pixels)), counts=cnt,
              cost0=c0, cost1=c1, bits_total=e.sum(axis=(2, 3)))
