"""Float64 yardstick of the MS-SSIM definition in DESIGN.md 4.5 (Wang, Simoncelli and Bovik 2003), for the tests of
jpdse_eval_metrics.  Deliberately NOT built like the kernel: the 11x11 window is applied as one direct 2-D correlation
(scipy.signal.correlate2d 'valid'; the same sum written as 121 shifted slices when scipy is absent), never as two 1-D passes,
the moments are the plain uncentred E_w[x^2] - mu^2, and nothing is shared with jpd-se_amd/.

Inputs: two images [3, H, W] (or [H, W, 3] uint8) holding the quantised values 0..255."""
import numpy as np

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
L = 255.0
C1 = (0.01 * L) ** 2
C2 = (0.03 * L) ** 2
MIN_SIDE = 176


def window():
  d = np.arange(11, dtype=np.float64) - 5.0
  g = np.exp(-d * d / (2.0 * 1.5 ** 2))
  w = np.outer(g, g)
  return w / w.sum()


def _correlate_valid(a, w):
  try:
    from scipy.signal import correlate2d
    return correlate2d(a, w, mode='valid')
  except ImportError:
    kh, kw = w.shape
    oh, ow = a.shape[0] - kh + 1, a.shape[1] - kw + 1
    out = np.zeros((oh, ow), dtype=np.float64)
    for i in range(kh):
      for j in range(kw):
        out += w[i, j] * a[i:i + oh, j:j + ow]
    return out


def _planes(img):
  a = np.asarray(img)
  if a.ndim != 3:
    raise ValueError('expected a 3-channel image, got shape %r' % (a.shape,))
  if a.shape[0] != 3 and a.shape[-1] == 3:
    a = np.transpose(a, (2, 0, 1))
  if a.shape[0] != 3:
    raise ValueError('expected 3 channels, got shape %r' % (a.shape,))
  return a.astype(np.float64)


def scale_maps(x, y):
  """(cs map, ssim map), each [3, H-10, W-10], of one scale."""
  w = window()
  cs, ss = [], []
  for c in range(3):
    a, b = x[c], y[c]
    mu_a, mu_b = _correlate_valid(a, w), _correlate_valid(b, w)
    s_aa = _correlate_valid(a * a, w) - mu_a * mu_a
    s_bb = _correlate_valid(b * b, w) - mu_b * mu_b
    s_ab = _correlate_valid(a * b, w) - mu_a * mu_b
    m_cs = (2.0 * s_ab + C2) / (s_aa + s_bb + C2)
    m_l = (2.0 * mu_a * mu_b + C1) / (mu_a * mu_a + mu_b * mu_b + C1)
    cs.append(m_cs)
    ss.append(m_cs * m_l)
  return np.stack(cs), np.stack(ss)


def downsample(a):
  """2x2 mean, stride 2; an odd last row / column is dropped."""
  h, w = a.shape[1] // 2 * 2, a.shape[2] // 2 * 2
  a = a[:, :h, :w]
  return 0.25 * (a[:, 0::2, 0::2] + a[:, 0::2, 1::2] + a[:, 1::2, 0::2] + a[:, 1::2, 1::2])


def combine(cs, ssim):
  """ms_ssim of the per-scale means; a mean <= 0 among the five that enter the product gives 0 (never nan)."""
  terms = [float(v) for v in cs[:4]] + [float(ssim[4])]
  if min(terms) <= 0.0:
    return 0.0
  out = 1.0
  for t, w in zip(terms, WEIGHTS):
    out *= t ** w
  return out


def ms_ssim(x, y):
  """dict(cs = [5] per-scale means of the cs maps, ssim = [5] of the ssim maps, ms_ssim = the combined value)."""
  x, y = _planes(x), _planes(y)
  if x.shape != y.shape:
    raise ValueError('shape mismatch %r vs %r' % (x.shape, y.shape))
  if min(x.shape[1:]) < MIN_SIDE:
    raise ValueError('the shorter side must be at least %d for five scales, got %r' % (MIN_SIDE, x.shape[1:]))
  cs, ss = [], []
  for j in range(5):
    if j:
      x, y = downsample(x), downsample(y)
    m_cs, m_ss = scale_maps(x, y)
    cs.append(float(m_cs.mean()))
    ss.append(float(m_ss.mean()))
  return dict(cs=np.array(cs), ssim=np.array(ss), ms_ssim=combine(cs, ss))


def quantise(x, mean, std):
  """tensor2im's quantiser on a normalised float array [..., 3 channels first]: uint8(clip((x * std + mean) * 255, 0, 255)),
  float64 arithmetic, truncation.  x: [3, H, W] or [N, 3, H, W]."""
  x = np.asarray(x, dtype=np.float64)
  shape = [1] * x.ndim
  shape[-3] = 3
  m = np.asarray(mean, dtype=np.float64).reshape(shape)
  s = np.asarray(std, dtype=np.float64).reshape(shape)
  return np.clip((x * s + m) * 255.0, 0, 255).astype(np.uint8)
