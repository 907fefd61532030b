"""The GEMM panels of one conv filter: when they are rebuilt from the fp32 KRSC master, and by which launch.

A layer keeps two panels per master, forward and data gradient.  WeightPanels owns them; decide() is the whole rule (state
table: DESIGN.md 5.1); stamp() is what "the master moved" means.

Optimizer protocol -- three attributes on the parameter tensor, touched only by the five functions below this docstring:
    _jpdse_wver       int, +1 per fused optimizer step that updated the tensor (the kernel writes the master outside torch's
                      version counter).  Written by optimizer_stepped(), read by stamp().
    _jpdse_cast_out   a bf16 tensor the optimizer kernel fills with a plain cast of the updated master, or None / absent.
                      Written by publish_cast() -- a CAST layer publishes its forward panel --, read by cast_target().
    _jpdse_cast_wver  the _jpdse_wver at which _jpdse_cast_out was last written.  Written by optimizer_stepped(), read by
                      cast_is_fresh().
"""
import torch

from . import JpdseError
from . import ops

_weights_epoch = [0]


def bump_weights_epoch():
  """Call after any in-place update of master weights done outside torch's version counter and outside the optimizer protocol:
  every panel is rebuilt lazily on next use."""
  _weights_epoch[0] += 1


def stamp(w):
  """What a master's panels were built from: (torch version, weights epoch, data_ptr, optimizer counter)."""
  return (w._version, _weights_epoch[0], w.data_ptr(), getattr(w, '_jpdse_wver', 0))


def cast_target(p):
  return getattr(p, '_jpdse_cast_out', None)


def publish_cast(w, fwd):
  w._jpdse_cast_out = fwd


def cast_is_fresh(w, fwd, now):
  """Did the optimizer step that produced stamp `now` write the forward panel `fwd`?"""
  _, _, _, counter = now
  return cast_target(w) is fwd and getattr(w, '_jpdse_cast_wver', None) == counter


def optimizer_stepped(p):
  """The optimizer's side: its kernel has updated p, and p's cast target if it has one."""
  p._jpdse_wver = getattr(p, '_jpdse_wver', 0) + 1
  if cast_target(p) is not None:
    p._jpdse_cast_wver = p._jpdse_wver


# Kind of a (master, layout) pair, fixed at construction.
#   ALIAS    fp32, the forward panel is the master itself: there is only a data-gradient panel to build
#   CAST     bf16, the forward panel is a plain cast of the master: the optimizer kernel writes it
#   PACKED   everything else: both panels come from the pack kernel
ALIAS, CAST, PACKED = 'alias', 'cast', 'packed'
ALLOC_AND_PACK, PACK_BOTH, PACK_DGRAD_ONLY, NONE = 'alloc_and_pack', 'pack_both', 'pack_dgrad_only', 'none'


def decide(kind, present, old, new, cast_fresh):
  """(action, batchable): what the lazy path does for panels built at stamp `old` (`present`: there are any) when the master
  is at `new`, and whether one batched launch over many layers (layers.PackBatcher) may do that work instead.  Pure."""
  if not present:
    return ALLOC_AND_PACK, False
  if old == new:
    return NONE, True
  (over, oepoch, optr, _), (nver, nepoch, nptr, _) = old, new
  only_optimizer = (over, oepoch, optr) == (nver, nepoch, nptr)
  if kind == ALIAS:
    if optr != nptr:
      return ALLOC_AND_PACK, False        # the forward panel IS the old storage
    return PACK_DGRAD_ONLY, only_optimizer
  if kind == CAST and only_optimizer and cast_fresh:
    return PACK_DGRAD_ONLY, True
  return PACK_BOTH, False


class WeightPanels(object):
  """The (forward, data gradient) panels of one master in the layout of conv descriptor `d` (N, H, W do not matter)."""

  def __init__(self, kind, d):
    self.kind, self.d, self.dtype = kind, d, d.dtype
    self._bufs = self._stamp = None
    self._entries = (None, None)        # (master ptr, panel ptr) -> ops.conv_pack_entries of them

  def _decide(self, w, now):
    present = self._bufs is not None
    return decide(self.kind, present, self._stamp, now, present and self.kind == CAST and cast_is_fresh(w, self._bufs[0], now))

  def get(self, w, source=None):
    """Panels of master `w`, rebuilt first if w moved.  source() -> the tensor to pack when that is not w itself (a slice)."""
    now = stamp(w)
    if now == self._stamp:
      return self._bufs
    action, _ = self._decide(w, now)
    src = w if source is None else source()
    if action == ALLOC_AND_PACK and self.kind != ALIAS:
      self._bufs = ops.conv_pack(self.d, src, w.device)
      if self.kind == CAST:
        publish_cast(w, self._bufs[0])
    else:
      if action == ALLOC_AND_PACK:
        self._bufs = (w.detach(), torch.empty(ops.conv_dgrad_pack_size(self.d), dtype=torch.uint8, device=w.device))
      fwd, dgrad = self._bufs
      if dgrad.device != w.device:
        raise JpdseError('weight panels live on %s but their master moved to %s' % (dgrad.device, w.device))
      ops.conv_pack_into(self.d, src, fwd if action == PACK_BOTH else None, dgrad)
    self._stamp = now
    return self._bufs

  def batch_entries(self, w):
    """Table entries for layers.PackBatcher; [] when nothing moved; None when the lazy path has to do the work (first use, both
    panels to build, weights replaced)."""
    action, batchable = self._decide(w, stamp(w))
    if not batchable:
      return None
    if action == NONE:
      return []
    key = (w.data_ptr(), self._bufs[1].data_ptr())
    if self._entries[0] != key:
      self._entries = (key, ops.conv_pack_entries(self.d, w, self._bufs[1]))
    return self._entries[1]

  def mark_fresh(self, w):
    """The batched launch has done what get(w) would have done."""
    self._stamp = stamp(w)
