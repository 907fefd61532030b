"""Integer yardstick of the per-class distortion table jpdse_eval_metrics_sem writes, for its tests.  Plain numpy on integer
arrays: np.bincount of the class index, weighted by each pixel's |d| and d^2 summed over the three channels.  The images are
quantised by tests/msssim_ref.py's `quantise` (tensor2im's arithmetic); nothing is shared with jpd-se_amd/.

Definition (the intent of the reference's get_sem_wise_distortion, pix2pixHD_model.py:646-706): row k of image n holds
(sum |q(fake) - q(real)|, sum (q(fake) - q(real))^2, pixels) over the 3 channels of the pixels labelled k; a label outside
[0, n_classes) or not an integer goes to row n_classes.  l1 / mse of a class = sum / (3 * pixels), 0 for an absent class."""
import numpy as np


def class_index(label, n_classes):
  """label: float array of any shape -> int64 class index of the same shape, n_classes for a stray label."""
  lab = np.asarray(label, dtype=np.float64)
  with np.errstate(invalid='ignore'):
    ok = (lab >= 0) & (lab < n_classes) & (lab == np.floor(lab))
  return np.where(ok, np.where(ok, lab, 0).astype(np.int64), n_classes)


def table(qf, qr, label, n_classes):
  """qf, qr: uint8 [N, 3, H, W] quantised images; label: [N, 1, H, W] or [N, H, W] floats.  int64 [N, n_classes + 1, 3]."""
  qf, qr = np.asarray(qf), np.asarray(qr)
  assert qf.dtype == np.uint8 and qr.dtype == np.uint8 and qf.shape == qr.shape and qf.shape[1] == 3
  n = qf.shape[0]
  idx = class_index(label, n_classes).reshape(n, -1)
  d = qf.astype(np.int64) - qr.astype(np.int64)
  a = np.abs(d).sum(axis=1).reshape(n, -1)
  s = (d * d).sum(axis=1).reshape(n, -1)
  out = np.zeros((n, n_classes + 1, 3), dtype=np.int64)
  for i in range(n):
    # bincount's weights are float64: every weight and every class total here is an integer far below 2^53, so exact
    out[i, :, 0] = np.rint(np.bincount(idx[i], weights=a[i], minlength=n_classes + 1)).astype(np.int64)
    out[i, :, 1] = np.rint(np.bincount(idx[i], weights=s[i], minlength=n_classes + 1)).astype(np.int64)
    out[i, :, 2] = np.bincount(idx[i], minlength=n_classes + 1)
  return out


def figures(tab):
  """tab: int64 [..., n_classes, 3] (the extra row already cut off) -> dict(pixels, l1, mse, psnr) of shape [..., n_classes]."""
  tab = np.asarray(tab, dtype=np.int64)
  pix = tab[..., 2]
  seen = pix > 0
  den = np.where(seen, 3 * pix, 1).astype(np.float64)
  l1 = np.where(seen, tab[..., 0] / den, 0.0)
  mse = np.where(seen, tab[..., 1] / den, 0.0)
  exact = 10.0 * np.log10(255.0 ** 2 / np.where(mse > 0, mse, 1.0))
  psnr = np.where(seen, np.where(mse > 0, exact, np.inf), np.nan)
  return dict(pixels=pix, l1=l1, mse=mse, psnr=psnr)


def per_class(tab):
  """The dict ops.eval_metrics returns under `per_class`, from the full table [N, n_classes + 1, 3]: batch figures are
  pixel-weighted (sums over the batch first), then the same per image."""
  tab = np.asarray(tab, dtype=np.int64)
  r = figures(tab[:, :-1].sum(axis=0))
  r['unlabelled'] = int(tab[:, -1, 2].sum())
  r['per_image'] = figures(tab[:, :-1])
  return r
