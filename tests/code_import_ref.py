"""numpy restatement of the learned codec's bitstream in both directions (jpdse_code_export / jpdse_code_import), built on
np.packbits / np.unpackbits: NCHW flatten order, MSB first, every image starting on a byte.  The yardstick shared by
tests/test_code_import_host.py, tests/test_hip_code_import.py and tests/test_hip_decode_golden.py."""
import numpy as np


def cpad(c):
  return (c + 7) & ~7


def export_packed(b):
  """b: [N, C, H, W] of +1 / -1 / 0 -> uint8 [N, ceil(C*H*W / 8)]: bit (b > 0), unused low bits of the last byte 0."""
  return np.packbits((b.reshape(b.shape[0], -1) > 0).astype(np.uint8), axis=1)


def export_float(b):
  """b: [N, C, H, W] -> float32 [N, C*H*W] = (b + 1) / 2."""
  return ((b.reshape(b.shape[0], -1).astype(np.float32) + np.float32(1)) * np.float32(0.5)).astype(np.float32)


def import_packed(code, N, C, H, W):
  """uint8 [N, ceil(C*H*W / 8)] -> float32 [N, C, H, W] of +1 / -1; bits beyond C*H*W of a row are ignored."""
  bits = C * H * W
  code = np.asarray(code, dtype=np.uint8)
  assert code.shape == (N, (bits + 7) // 8), code.shape
  on = np.unpackbits(code, axis=1)[:, :bits]
  return np.where(on > 0, np.float32(1), np.float32(-1)).reshape(N, C, H, W).astype(np.float32)


def import_float(code, N, C, H, W):
  """float32 [N, C*H*W] -> float32 [N, C, H, W]: +1 where code > 0.5f, -1 everywhere else (NaN included)."""
  code = np.asarray(code, dtype=np.float32)
  assert code.shape == (N, C * H * W), code.shape
  with np.errstate(invalid='ignore'):
    on = code > np.float32(0.5)
  return np.where(on, np.float32(1), np.float32(-1)).reshape(N, C, H, W).astype(np.float32)


def to_nhwc(b):
  """[N, C, H, W] -> the stored form [N, H, W, CPAD(C)], padding lanes 0."""
  n, c, h, w = b.shape
  out = np.zeros((n, h, w, cpad(c)), dtype=np.float32)
  out[..., :c] = np.transpose(b, (0, 2, 3, 1))
  return out
