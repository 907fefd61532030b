"""Float64 yardstick of the MS-SSIM training loss (--distortion_loss_fn ms_ssim), for the tests of
jpdse_msssim_loss.  torch on the CPU; the gradient is autograd's.  Deliberately NOT built like the kernel: the 11x11 window
is one 2-D F.conv2d, never two 1-D passes, the moments are the plain uncentred E_w[x^2] - mu^2, the scales come from
F.avg_pool2d, and nothing is shared with jpd-se_amd/.

Inputs: normalised images [N, 3, H, W] (the values the network produces), mean / std: the per-channel de-normalisation
u = v * std_c + mean_c.  No clipping, no quantisation; L = 1."""
import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
C1 = 0.01 ** 2
C2 = 0.03 ** 2
MIN_SIDE = 176


def window(dtype=torch.float64):
  d = torch.arange(11, dtype=torch.float64) - 5.0
  g = torch.exp(-d * d / (2.0 * 1.5 ** 2))
  w = torch.outer(g, g)
  return (w / w.sum()).to(dtype)


def scale_means(fake, real, mean, std, dtype=torch.float64):
  """(cs [N, 5], ssim [N, 5]): the per-scale means over channels and positions, differentiable w.r.t. `fake`."""
  if fake.shape != real.shape or fake.dim() != 4 or fake.shape[1] != 3:
    raise ValueError('expected two [N, 3, H, W] images, got %r and %r' % (tuple(fake.shape), tuple(real.shape)))
  if min(fake.shape[2:]) < MIN_SIDE:
    raise ValueError('the shorter side must be at least %d for five scales, got %r' % (MIN_SIDE, tuple(fake.shape[2:])))
  m = torch.tensor([float(v) for v in mean], dtype=dtype).view(1, 3, 1, 1)
  s = torch.tensor([float(v) for v in std], dtype=dtype).view(1, 3, 1, 1)
  x = fake.to(dtype) * s + m
  y = real.to(dtype) * s + m
  w = window(dtype)[None, None].repeat(3, 1, 1, 1)
  cs, ss = [], []
  for j in range(5):
    if j:
      x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)      # floor mode: an odd last row / column is dropped
    mx, my = F.conv2d(x, w, groups=3), F.conv2d(y, w, groups=3)
    sxx = F.conv2d(x * x, w, groups=3) - mx * mx
    syy = F.conv2d(y * y, w, groups=3) - my * my
    sxy = F.conv2d(x * y, w, groups=3) - mx * my
    m_cs = (2.0 * sxy + C2) / (sxx + syy + C2)
    m_l = (2.0 * mx * my + C1) / (mx * mx + my * my + C1)
    cs.append(m_cs.mean(dim=(1, 2, 3)))
    ss.append((m_cs * m_l).mean(dim=(1, 2, 3)))
  return torch.stack(cs, dim=1), torch.stack(ss, dim=1)


def ms_ssim_per_image(cs, ss):
  """[N]: prod_{j<5} cs_j^w_j * ssim_5^w_5; an image with one of those five means <= 0 gets the constant 0 (gradient 0)."""
  terms = torch.cat([cs[:, :4], ss[:, 4:5]], dim=1)
  w = torch.tensor(WEIGHTS, dtype=terms.dtype)
  ok = (terms > 0).all(dim=1)
  safe = torch.where(ok[:, None], terms, torch.ones_like(terms))
  return torch.where(ok, torch.prod(safe ** w, dim=1), torch.zeros_like(ok, dtype=terms.dtype))


def loss(fake, real, mean, std, dtype=torch.float64):
  """dict(loss: 0-dim tensor mean_n (1 - ms_ssim_n), ms_ssim [N], cs [N, 5], ssim [N, 5]); no gradient."""
  with torch.no_grad():
    cs, ss = scale_means(fake, real, mean, std, dtype)
    ms = ms_ssim_per_image(cs, ss)
    return dict(loss=(1.0 - ms).mean(), ms_ssim=ms, cs=cs, ssim=ss)


def loss_and_grad(fake, real, mean, std):
  """The float64 loss and d loss / d fake [N, 3, H, W] (float64), from autograd."""
  f = fake.detach().to(torch.float64).clone().requires_grad_(True)
  cs, ss = scale_means(f, real.detach(), mean, std)
  ms = ms_ssim_per_image(cs, ss)
  value = (1.0 - ms).mean()
  g, = torch.autograd.grad(value, f, allow_unused=True)
  if g is None:                        # every image under the zero rule
    g = torch.zeros_like(f)
  return dict(loss=value.detach(), ms_ssim=ms.detach(), cs=cs.detach(), ssim=ss.detach(), grad=g)
