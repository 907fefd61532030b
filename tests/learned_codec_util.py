"""numpy restatement of the learned codec's binarizer noise and codes (TEST INFRASTRUCTURE; include/jpdse.h "learned codec").

Philox4x32-10 after Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3" (SC'11); the known-answer
vectors of its Random123 distribution are checked in tests/test_learned_codec_host.py."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
  """ctr: uint32 array [..., 4], key: uint32 array [..., 2] (broadcast) -> uint32 [..., 4]."""
  c = [np.asarray(ctr[..., i], dtype=np.uint32) for i in range(4)]
  k0 = np.asarray(key[..., 0], dtype=np.uint32)
  k1 = np.asarray(key[..., 1], dtype=np.uint32)
  with np.errstate(over='ignore'):
    for _ in range(10):
      p0 = M0 * c[0].astype(np.uint64)
      p1 = M1 * c[2].astype(np.uint64)
      hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & MASK).astype(np.uint32)
      hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & MASK).astype(np.uint32)
      c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
      k0 = (k0 + W0).astype(np.uint32)
      k1 = (k1 + W1).astype(np.uint32)
  return np.stack(c, axis=-1)


def codec_noise(n_global, C, H, W, seed, draw):
  """u fp32 [C, H, W] of one image: word (e & 3) of Philox(counter=(e >> 2, n_global, draw lo, draw hi),
  key=(seed lo, seed hi)), u = (word >> 8) * 2^-24, e the logical NCHW index inside the image."""
  e = np.arange(C * H * W, dtype=np.uint64)
  ctr = np.zeros((e.size, 4), dtype=np.uint32)
  ctr[:, 0] = (e >> np.uint64(2)).astype(np.uint32)
  ctr[:, 1] = np.uint32(n_global)
  ctr[:, 2] = np.uint32(draw & 0xFFFFFFFF)
  ctr[:, 3] = np.uint32(draw >> 32)
  key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
  words = philox4x32_10(ctr, key)
  w = words[np.arange(e.size), (e & np.uint64(3)).astype(np.int64)]
  return ((w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).reshape(C, H, W)


def batch_noise(N, C, H, W, seed, draw, n_global0=0):
  return np.stack([codec_noise(n_global0 + i, C, H, W, seed, draw) for i in range(N)])


def soft_sign(t, u):
  """SoftSignFunction.forward (reference ctu/quantizers/binarize.py:17-24) in fp32: +1 where (1 - t) / 2 <= u, else -1."""
  t = np.asarray(t, dtype=np.float32)
  h = (np.float32(1.0) - t) / np.float32(2.0)
  return np.where(h <= u, np.float32(1.0), np.float32(-1.0))
