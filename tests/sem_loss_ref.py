"""float64 torch-CPU restatement of the semantics-weighted distortion: the yardstick of
tests/test_hip_sem_loss.py, pinned to hand-written examples in tests/test_sem_loss_host.py.

  w(p)   = cw[label(p)] * (ew if edge(p) else 1);  a label outside [0, len(cw)) has weight 1, a fractional one is truncated
  edge(p): the instance id of p differs from its left, right, upper or lower neighbour's inside the same image
  value  = sum_p sum_c w(p) f(d) / (N H W C),  d = fake - real,  f = |d| (l1) or d^2 (mse)
  grad   = scale * w(p) * sign(d) / (N H W C)  or  scale * w(p) * 2 d / (N H W C)
"""
import torch


def edges(inst):
  """inst: integer tensor [N, H, W] -> bool [N, H, W].  Ids are compared as int64."""
  inst = inst.to(torch.int64)
  assert inst.dim() == 3
  e = torch.zeros(inst.shape, dtype=torch.bool)
  dx = inst[:, :, 1:] != inst[:, :, :-1]       # between horizontal neighbours of one row
  e[:, :, 1:] |= dx
  e[:, :, :-1] |= dx
  dy = inst[:, 1:, :] != inst[:, :-1, :]       # between vertical neighbours of one image
  e[:, 1:, :] |= dy
  e[:, :-1, :] |= dy
  return e


def weight_map(label, inst, table, edge_w):
  """label: float [N, H, W]; inst: integer [N, H, W] or None; table: sequence of class weights -> float64 [N, H, W]."""
  cw = torch.as_tensor([float(v) for v in table], dtype=torch.float64)
  lab = torch.trunc(label.to(torch.float64))
  inside = (lab >= 0) & (lab < cw.numel())     # NaN compares false
  idx = torch.where(inside, lab, torch.zeros_like(lab)).to(torch.int64)
  w = torch.where(inside, cw[idx], torch.ones_like(lab))
  if inst is not None:
    w = torch.where(edges(inst), w * float(edge_w), w)
  return w


def loss(fake, real, label, inst, table, edge_w, kind):
  """fake, real: [N, C, H, W]; the weighted value as a Python float (float64 arithmetic)."""
  d = fake.to(torch.float64) - real.to(torch.float64)
  f = d.abs() if kind == 'l1' else d * d
  assert kind in ('l1', 'mse')
  w = weight_map(label, inst, table, edge_w)[:, None]
  return float((w * f).sum() / d.numel())


def grad(fake, real, label, inst, table, edge_w, kind, scale=1.0):
  """d (scale * loss) / d fake, float64 [N, C, H, W]."""
  d = fake.to(torch.float64) - real.to(torch.float64)
  assert kind in ('l1', 'mse')
  g = torch.sign(d) if kind == 'l1' else 2.0 * d
  return float(scale) * weight_map(label, inst, table, edge_w)[:, None] * g / d.numel()
