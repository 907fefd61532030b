"""Layer objects with explicit forward/backward over the C ABI (no autograd on the hot path).

Each layer exposes
    fwd(x: Act) -> (y: Act, ctx)          ctx = what backward needs (batch-sliceable)
    bwd(ctx, dy: Act, need_dx, need_dw) -> dx | None
Parameters are torch Parameters whose logical shapes/keys equal the reference checkpoint
layout while their memory is channels_last (= KRSC, the ABI's master
layout), so `state_dict()` round-trips with reference `net_G.pth` / `net_D.pth` files.
Weight gradients are written by the kernels straight into persistent `.grad` buffers.
"""
import math

import torch
import torch.nn as nn

from . import ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, PAD_ZERO, PAD_REFLECT, F32, BF16, binding_epoch
from . import ops
from .ops import Act
from .panels import WeightPanels, ALIAS, CAST, PACKED, bump_weights_epoch   # noqa: F401  (bump_weights_epoch: the trainer's import)


class Ctx(object):
  """Saved tensors of one layer call; every entry is batch-first so a sub-batch can be
  back-propagated on its own (used for the fake half of the batched discriminator pass)."""
  __slots__ = ('items',)

  def __init__(self, *items):
    self.items = items

  def slice(self, b0, b1):
    out = []
    for it in self.items:
      if isinstance(it, Act):
        out.append(it.batch_slice(b0, b1))
      elif torch.is_tensor(it):
        out.append(it[b0:b1])
      elif isinstance(it, Ctx):
        out.append(it.slice(b0, b1))
      elif isinstance(it, (list, tuple)):
        out.append(type(it)(c.slice(b0, b1) if isinstance(c, Ctx) else c for c in it))
      else:
        out.append(it)
    return Ctx(*out)


class HipConv2d(nn.Module):
  """nn.Conv2d / nn.ConvTranspose2d with the padding layer and the activation folded in."""

  def __init__(self, cin, cout, k, stride=1, pad=0, pad_mode=PAD_ZERO, act=ACT_NONE, slope=0.2,
               apply_bias=True, transposed=False, dtype=F32, device=None, bias=True):
    super(HipConv2d, self).__init__()
    self.cin, self.cout, self.k = cin, cout, k
    self.stride, self.pad, self.pad_mode = stride, pad, pad_mode
    self.act, self.slope = act, slope
    self.apply_bias = apply_bias      # False: conv feeds an affine-less InstanceNorm (bias is dead)
    assert bias or not apply_bias     # bias=False: no bias parameter at all (nn.Conv2d(..., bias=False))
    self.transposed = transposed
    self.cdtype = dtype
    if transposed:
      assert stride == 2 and pad == 1 and k == 3 and act == ACT_NONE and not apply_bias
      shape = (cin, cout, k, k)       # torch IOHW
    else:
      shape = (cout, cin, k, k)
    w = torch.empty(shape, device=device).contiguous(memory_format=torch.channels_last)
    w.normal_(0.0, 0.02)              # weights_init (networks.py:19-25)
    fan_in = shape[1] * k * k
    bound = 1.0 / math.sqrt(fan_in)
    b = torch.empty(cout, device=device).uniform_(-bound, bound)
    self.weight = nn.Parameter(w)
    if bias:
      self.bias = nn.Parameter(b)
    else:
      self.register_parameter('bias', None)
    self._panels = WeightPanels(self._panel_kind(), self._desc(1, 64, 64))
    self._slice = (None, None)        # bwd_input_slice: (channel range, its WeightPanels)
    self._route_answers = {}          # _route_answer
    self._bias_grad_store = None
    self.grad_ready_hook = None       # callable(param) fired right after a gradient is written

  # -- descriptors ---------------------------------------------------------------------------
  def _desc(self, N, H, W):
    """H, W: spatial size of the underlying Conv2d's INPUT."""
    if self.transposed:
      return ops.conv_desc(self.cdtype, N, H, W, self.cout, self.cin, self.k, self.k, 2, 1, PAD_ZERO)
    return ops.conv_desc(self.cdtype, N, H, W, self.cin, self.cout, self.k, self.k, self.stride, self.pad,
                         self.pad_mode, self.act, self.slope)

  def _master(self):
    w = self.weight
    assert w.dtype == torch.float32 and w.permute(0, 2, 3, 1).is_contiguous(), \
        'master weights must be fp32 channels_last (KRSC)'
    return w

  def _panel_kind(self):
    """ALIAS: fp32 layers whose forward panel [Ks][R][S*Cs] would be an element-for-element copy of the KRSC master (no channel
    or chunk padding): the kernels read the master itself -- no copy after each optimizer step (round 4: 32 such copies per
    step cost BASELINE config 2 0.4 ms of 24).  CAST: bf16 layers whose forward panel is an element-for-element cast of the
    master (no padding, no Toeplitz extra; thin inputs / heads carry extra panels) -- the fused Adam kernel can write it."""
    C, K = (self.cout, self.cin) if self.transposed else (self.cin, self.cout)
    if self.cdtype == F32:
      return ALIAS if C % 8 == 0 and K % 8 == 0 and (self.k * C) % 16 == 0 else PACKED
    return CAST if C % 64 == 0 and K % 8 == 0 and K > 8 else PACKED

  def packs(self):
    assert self.cdtype == self._panels.dtype, 'the compute dtype is fixed at construction'
    return self._panels.get(self._master())

  def batched_pack_entries(self):
    """Table entries for PackBatcher, [] when there is nothing to do, or None when this layer needs its own pack call right
    now (panels.decide)."""
    return self._panels.batch_entries(self._master())

  def _wgrad_buffer(self):
    w = self.weight
    if w.grad is None or w.grad.data_ptr() == 0 or not w.grad.permute(0, 2, 3, 1).is_contiguous():
      w.grad = torch.zeros_like(w, memory_format=torch.preserve_format)
    return w.grad

  def _bgrad_buffer(self):
    if self.bias is None:
      return None
    if self._bias_grad_store is None or self._bias_grad_store.device != self.bias.device:
      self._bias_grad_store = torch.zeros(ops.cpad(self.cout), dtype=torch.float32, device=self.bias.device)
      self.bias.grad = self._bias_grad_store[:self.cout]
    elif self.bias.grad is None:
      self.bias.grad = self._bias_grad_store[:self.cout]
    return self._bias_grad_store

  def ensure_grads(self):
    if self.weight.requires_grad:
      self._wgrad_buffer()
      self._bgrad_buffer()

  # -- forward / backward ---------------------------------------------------------------------
  def fwd(self, x):
    fwd_pack, dgrad_pack = self.packs()
    if self.transposed:
      d = self._desc(x.N, 2 * x.H, 2 * x.W)
      y = ops.conv_dgrad(d, x, dgrad_pack)
      return y, Ctx(x)
    d = self._desc(x.N, x.H, x.W)
    y = ops.conv_fwd(d, x, fwd_pack, self.bias if self.apply_bias else None)
    return y, Ctx(x, y if self.act != ACT_NONE else None)

  def fwd_pool(self, x):
    """(y, MaxPool2d(2, 2)(y), ctx): the conv -> ReLU -> pool chain of VGG19 in one call."""
    assert not self.transposed
    fwd_pack, _ = self.packs()
    d = self._desc(x.N, x.H, x.W)
    y, yp = ops.conv_fwd_pool(d, x, fwd_pack, self.bias if self.apply_bias else None)
    return y, yp, Ctx(x, y if self.act != ACT_NONE else None)

  def fwd_moments(self, x):
    """Forward for a conv whose output goes straight into an affine-less InstanceNorm: (y, ctx, moments, slots) with the
    norm's moment pass fused into the conv epilogue (jpdse_conv_fwd_moments), or None when this layer's kernel has no such
    epilogue (or the layer applies a bias / activation)."""
    if self.apply_bias or self.act != ACT_NONE or self.cdtype != BF16:
      return None
    dims = (x.N, 2 * x.H, 2 * x.W) if self.transposed else (x.N, x.H, x.W)
    slots = self._route_answer(ops.conv_moment_slots, dims, self.transposed)
    if slots <= 0:
      return None
    fwd_pack, dgrad_pack = self.packs()
    y, mom = ops.conv_fwd_moments(self._desc(*dims), x, dgrad_pack if self.transposed else fwd_pack, slots, self.transposed)
    return y, (Ctx(x) if self.transposed else Ctx(x, None)), mom, slots

  def nsum_slots(self, N, H, W):
    """Slots per image of the norm-backward sums this layer's data-gradient epilogue can write (0: none), cached per shape."""
    if self.transposed or self.cdtype != BF16:
      return 0
    return self._route_answer(ops.conv_dgrad_nsum_slots, (N, H, W))

  def _route_answer(self, query, dims, *args):
    """query(self._desc(*dims), *args), asked once per shape and per binding: the answer depends on which library /
    kernel-selection mode is bound."""
    key = (query, binding_epoch(), dims)
    if key not in self._route_answers:
      self._route_answers[key] = query(self._desc(*dims), *args)
    return self._route_answers[key]

  def bwd(self, ctx, dy, need_dx=True, need_dw=True, dy_is_dz=False, relu_input=False, addend=None, input_slope=0.0, sink=None):
    """dy_is_dz: dy is already the gradient w.r.t. the PRE-activation (the caller fused this layer's
    activation backward upstream); relu_input: the layer's input is a ReLU output (LeakyReLU(input_slope) when
    input_slope != 0) and the returned dx is wanted w.r.t. that activation's pre-activation (mask fused into the
    data-gradient epilogue); addend: another gradient w.r.t. the layer's input, summed into dx in the same epilogue;
    sink = (norm input Act, stats, act, slope): dx is the gradient w.r.t. the OUTPUT of that InstanceNorm (+ activation) -- when
    this layer's data-gradient kernel can, its epilogue also writes the sums of that norm's backward (dx.nsums)."""
    fwd_pack, dgrad_pack = self.packs()
    need_dw = need_dw and self.weight.requires_grad
    if self.transposed:
      (x,) = ctx.items
      d = self._desc(x.N, 2 * x.H, 2 * x.W)
      if need_dw:
        ops.conv_wgrad(d, dy, x, self._wgrad_buffer())
        self._bgrad_buffer()
        self._fire()
      return ops.conv_fwd(d, dy, fwd_pack, None) if need_dx else None
    x, y = ctx.items
    d = self._desc(x.N, x.H, x.W)
    dz = dy if (self.act == ACT_NONE or dy_is_dz) else ops.act_bwd(y, dy, self.act, self.slope)
    if need_dw:
      ops.conv_wgrad(d, x, dz, self._wgrad_buffer())
      store = self._bgrad_buffer()
      if self.apply_bias:
        ops.channel_sum(dz, store)          # writes CPAD(K) sums into the layer's private store
        if self.bias.grad.data_ptr() != store.data_ptr():
          self.bias.grad.copy_(store[:self.cout])   # .grad re-homed into a DDP bucket view
      self._fire()
    if not need_dx:
      return None
    if sink is not None and input_slope == 0.0:
      slots = self.nsum_slots(x.N, x.H, x.W)
      if slots > 0:
        sx, sstats, sact, sslope = sink
        return ops.conv_dgrad_nsums(d, dz, dgrad_pack, slots, sx, sstats, sact, sslope,
                                    relu_input=x if relu_input else None, addend=addend)
    return ops.conv_dgrad(d, dz, dgrad_pack, relu_input=x if relu_input else None, addend=addend, mask_slope=input_slope)

  def bwd_batched(self, ctx, dy, B, later, relu_input=False, addend=None, input_slope=0.0):
    """One backward call for two losses (the PatchGAN under loss_G and loss_D): `ctx` is the saved forward of 2B images and
    dy holds 3B gradient images [loss_G on images 0..B ; loss_D on images 0..2B].  The data gradient runs over all 3B in one
    launch, gradient image n >= B reading the saved operands of image n - B (jpdse_conv_dgrad_batched); addend (B images)
    joins the loss_G part only.  The weight gradient is loss_D's: images B..3B of dy against the saved 2B inputs, appended
    to `later` as a call for the owner to make.  For layers without an activation of their own."""
    assert not self.transposed and self.act == ACT_NONE
    _, dgrad_pack = self.packs()
    x, _ = ctx.items
    assert dy.N == x.N + B
    if self.weight.requires_grad:
      later.append(lambda: self.bwd(ctx, dy.batch_slice(B, dy.N), need_dx=False, need_dw=True))
    return ops.conv_dgrad_batched(self._desc(dy.N, x.H, x.W), dy, dgrad_pack, B, relu_input=x if relu_input else None,
                                  addend=addend, mask_slope=input_slope)

  def bwd_input_slice(self, ctx, dy, c0, c1, dy_is_dz=False):
    """Data gradient w.r.t. input channels [c0, c1) only (no weight gradient): the conv restricted to those input
    channels has the filter w[:, c0:c1], and its data gradient is that slice of the full one.  Used where only part
    of a concatenated input needs a gradient (PatchGAN layer 0: 3 image channels of the 39-channel input -- the
    full data gradient is 13x the work and 5x the bytes)."""
    assert not self.transposed
    x, y = ctx.items
    dz = dy if (self.act == ACT_NONE or dy_is_dz) else ops.act_bwd(y, dy, self.act, self.slope)
    w = self._master()
    d = ops.conv_desc(self.cdtype, x.N, x.H, x.W, c1 - c0, self.cout, self.k, self.k, self.stride, self.pad,
                      self.pad_mode, ACT_NONE, self.slope)
    # panels of their own per channel range: while the range stays, a moved master is re-packed into the existing buffers
    # (the weight version alone changes every step)
    if self._slice[0] != (c0, c1):
      self._slice = ((c0, c1), WeightPanels(PACKED, d))
    _, dgrad_pack = self._slice[1].get(w, lambda: w.detach()[:, c0:c1].contiguous(memory_format=torch.channels_last))
    return ops.conv_dgrad(d, dz, dgrad_pack)

  def _fire(self):
    if self.grad_ready_hook is not None:
      self.grad_ready_hook(self)


class HipBinarizer(nn.Module):
  """Binarizer (ctu/quantizers/binarize.py:47-65): 1x1 conv without bias -> tanh (the conv's epilogue) -> sign, stochastic
  in training (SoftSignFunction) and deterministic in eval, following the module's `training` flag.  The conv is
  registered as `conv`: state-dict key `<prefix>.conv.weight` [cout, cin, 1, 1] as in the reference.

  Noise (train mode): the Philox stream of jpdse_binarize_fwd, addressed by `seed`, `draw` (the caller's count of training
  forwards) and `n_global0` (index of the call's first image in the global batch), all set by the owner before fwd.
  `noise_override`: fp32 [N, C, H, W] cuda tensor used by the NEXT fwd only, instead of the stream (test hook)."""

  def __init__(self, cin, cout, dtype=F32, device=None):
    super(HipBinarizer, self).__init__()
    self.conv = HipConv2d(cin, cout, 1, act=ACT_TANH, apply_bias=False, bias=False, dtype=dtype, device=device)
    self.seed, self.draw, self.n_global0 = 0, 0, 0
    self.noise_override = None
    self.rate_scale, self.rate_denom, self.rate_value = None, 0, None      # rate_denom: pixels per image

  def fwd(self, x):
    t, ctx = self.conv.fwd(x)                     # ctx = (x, t): the tanh backward reads the stored t
    u, self.noise_override = self.noise_override, None
    b = ops.binarize_fwd(t, self.training, self.seed, self.draw, self.n_global0, u)
    if self.rate_scale is not None:
      # --lambda_rate: the owner set rate_scale / rate_denom for this call; the value slot stays in
      # rate_value and the gradient w.r.t. t travels with the context
      self.rate_value, _, d_rate, _ = ops.code_rate_loss(b, t, self.rate_denom, self.rate_scale)
      ctx = Ctx(ctx, d_rate)
    return b, ctx

  def bwd(self, ctx, db, need_dx=True, need_dw=True):
    """Straight-through estimator (binarize.py:26-28): db is the gradient w.r.t. tanh's output; conv.bwd applies
    tanh' = 1 - t^2 and runs the 1x1 conv's data / weight gradients.  A context of a forward with a rate scale also holds
    the rate term's gradient w.r.t. t, which is added to db first."""
    if len(ctx.items) == 2 and isinstance(ctx.items[0], Ctx):
      ctx, d_rate = ctx.items
      db = ops.add(db, d_rate)
    return self.conv.bwd(ctx, db, need_dx, need_dw)


def vq_bottleneck_check(cout, n_center, center_size, sigma, who='HipVQBottleneck'):
  """ValueError unless a bottleneck of `cout` channels can be quantized in groups of center_size (host only)."""
  if center_size < 1 or cout % center_size != 0:
    raise ValueError('%s: center_size %d does not divide the bottleneck\'s %d channels' % (who, center_size, cout))
  if ops.cpad(cout) != cout:
    raise ValueError('%s: %d channels are no multiple of 8: the NHWC tensor would carry padding lanes between the vectors'
                     % (who, cout))
  if not 1 <= center_size <= ops.VQ_MAX_D or not 2 <= n_center <= ops.VQ_MAX_L:
    raise ValueError('%s: center_size %d / n_center %d, the kernels take 1 .. %d and 2 .. %d'
                     % (who, center_size, n_center, ops.VQ_MAX_D, ops.VQ_MAX_L))
  if not (float(sigma) > 0.0 and float(sigma) != float('inf')):
    raise ValueError('%s: sigma must be a finite number > 0, got %r' % (who, sigma))


class HipVQBottleneck(nn.Module):
  """The soft-to-hard vector quantizer as the encoder's bottleneck, in the binarizer's Sequential slot: a 1x1
  conv without bias or activation (`conv`: state-dict key `<prefix>.conv.weight` [cout, cin, 1, 1]) and an S2HVQ (`vq`: key
  `<prefix>.vq._code_book` [n_center, center_size]).  The conv's NHWC output [N, h, w, cout] IS the quantizer's [M][D] matrix:
  M = N h w cout / D, vector m = pixel * (cout / D) + group, every vector D consecutive channels of one pixel -- no re-layout
  pass.  That needs center_size | cout and cpad(cout) == cout (no padding lanes); anything else is a ValueError here.

  Forward: the hard form (y = the nearest centre) in eval mode and, unless `hard_forward` is False, in training; backward: the
  gradient of the soft form either way (ops.vq_quantize_bwd), the code book's written into its persistent `.grad` buffer.
  Code book: uniform in [-1, 1], drawn as 2 * torch.rand(n_center, center_size) - 1 in float32 from a CPU torch.Generator
  seeded with `seed` (default 0) -- the same book on every device and rank; load_state_dict replaces it."""

  def __init__(self, cin, cout, n_center=64, center_size=8, sigma=10.0, hard_forward=True, dtype=F32, device=None, seed=0):
    super(HipVQBottleneck, self).__init__()
    n_center, center_size = int(n_center), int(center_size)
    vq_bottleneck_check(cout, n_center, center_size, sigma)
    from ctu.quantizers.s2h_vq import S2HVQ      # the module the layer wraps; it refuses n_center / center_size beyond the kernels'
    book = torch.rand(n_center, center_size, generator=torch.Generator().manual_seed(int(seed))) * 2 - 1
    self.conv = HipConv2d(cin, cout, 1, act=ACT_NONE, apply_bias=False, bias=False, dtype=dtype, device=device)
    self.vq = S2HVQ(book.to(device) if device is not None else book, sigma=float(sigma))
    self.cout, self.center_size, self.n_center = cout, center_size, n_center
    self.hard_forward = bool(hard_forward)
    self.grad_ready_hook = None
    self.rate_scale, self.rate_denom, self.rate_value = None, 0, None

  @property
  def groups(self):
    """Channel groups of a pixel: vector m of the [M][D] matrix belongs to group m % groups."""
    return self.cout // self.center_size

  def _book(self):
    c = self.vq._code_book
    assert c.dtype == torch.float32 and c.is_contiguous(), 'the code book must be contiguous fp32'
    return c

  def _cgrad_buffer(self):
    c = self._book()
    if c.grad is None or not c.grad.is_contiguous():
      c.grad = torch.zeros_like(c)
    return c.grad

  def ensure_grads(self):
    if self.vq._code_book.requires_grad:
      self._cgrad_buffer()

  def _quantize(self, h, hard):
    D = self.center_size
    y, index, _ = ops.vq_quantize_fwd(h.t.view(-1, D), self._book().detach(), self.vq.sigma, hard)
    return Act(y.view(h.t.shape), h.C), index

  def fwd(self, x):
    h, c_conv = self.conv.fwd(x)
    y, _ = self._quantize(h, self.hard_forward or not self.training)
    if self.rate_scale is not None:
      # --lambda_vq_rate: the owner set rate_scale / rate_denom for this call; the value stays in rate_value
      # and the gradient w.r.t. the per-group sums of the soft assignment travels with the context
      self.rate_value, _, dhist = ops.vq_rate_fwd(h.t.view(-1, self.center_size), self._book().detach(), self.vq.sigma,
                                                  self.groups, self.rate_denom, self.rate_scale)
      return y, Ctx(c_conv, h, dhist)
    return y, Ctx(c_conv, h)

  def rate(self, x, denom):
    """fp32 [1]: the hard-mode rate of x's features (ops.vq_rate_fwd, hard): the zero-order entropy of code(x) per channel
    group, in bits / denom."""
    h, _ = self.conv.fwd(x)
    value, _, _ = ops.vq_rate_fwd(h.t.view(-1, self.center_size), self._book().detach(), self.vq.sigma, self.groups, denom,
                                  hard=True, want_grad=False)
    return value

  def features(self, x):
    """The 1x1 conv's output as the [M, D] matrix the quantizer sees (the layout above; a view, in the layer's dtype)."""
    h, _ = self.conv.fwd(x)
    return h.t.view(-1, self.center_size)

  def usage(self, x):
    """fp32 [groups, n_center]: how many vectors of x's features have each centre as their nearest, per channel group
    (ops.vq_rate_fwd, hard: the histogram of code(x))."""
    _, hist, _ = ops.vq_rate_fwd(self.features(x), self._book().detach(), self.vq.sigma, self.groups, 1.0, hard=True,
                                 want_hist=True, want_grad=False)
    return hist

  def fit(self, feature_matrices, n_iter=10, init='sample', seed=0, reseed=True):
    """Fit the code book to feature matrices as features() returns them (a list of [M, D] tensors): S2HVQ.fit with code_len 1
    (DESIGN.md 4.21).  In place: the book's storage, requires_grad and .grad stay."""
    return self.vq.fit(feature_matrices, 1, n_iter=n_iter, init=init, seed=seed, reseed=reseed)

  def code(self, x):
    """int32 [N, h * w * cout / D]: the index of the nearest centre of every vector of x's features, in the layout above."""
    h, _ = self.conv.fwd(x)
    _, index = self._quantize(h, True)
    return index.view(h.N, -1)

  def code_ec(self, x, lam, n_iter=2):
    """(index, reports): code() under the entropy constraint -- S2HVQ.encode_ec PER IMAGE on that image's rows
    of features(x), groups = the channel groups: the coders adapt per image, so the histograms are per image.  index int32
    [N, h * w * cout / D]; reports: the N report dicts of encode_ec."""
    f = self.features(x)
    N = x.N
    rows = f.shape[0] // N
    codes, reports = [], []
    for i in range(N):
      code, report = self.vq.encode_ec(f[i * rows:(i + 1) * rows], 1, lam, groups=self.groups, n_iter=n_iter)
      codes.append(code.view(1, rows))
      reports.append(report)
    return torch.cat(codes, dim=0).to(torch.int32), reports

  def decode(self, index, N, h, w, dtype_code):
    """The features Act [N, h, w, cout] of an index tensor as code() returns it (ops.vq_decode: bit for bit what the hard
    forward emitted) and the status word of ops.vq_decode."""
    from .ops import tdtype_of
    y, status = ops.vq_decode(index.contiguous().view(-1), self._book().detach(), tdtype_of(dtype_code))
    return Act(y.view(N, h, w, self.cout), self.cout), status

  def bwd(self, ctx, dy, need_dx=True, need_dw=True):
    """dy: the gradient w.r.t. the quantized features.  Straight-through: the soft form's gradient, then the
    1x1 conv's data / weight gradients."""
    c_conv, h = ctx.items[:2]
    D = self.center_size
    book = self._book()
    want_dc = need_dw and book.requires_grad
    if len(ctx.items) == 3:      # a forward with a rate scale: its dhist joins dp in the grouped backward
      dh, _ = ops.vq_quantize_bwd(dy.t.view(-1, D), h.t.view(-1, D), book.detach(), self.vq.sigma, None, want_dx=True,
                                  want_dc=want_dc, dc_out=self._cgrad_buffer() if want_dc else None, groups=self.groups,
                                  dhist=ctx.items[2])
    else:
      dh, _ = ops.vq_quantize_bwd(dy.t.view(-1, D), h.t.view(-1, D), book.detach(), self.vq.sigma, None, want_dx=True,
                                  want_dc=want_dc, dc_out=self._cgrad_buffer() if want_dc else None)
    if want_dc and self.grad_ready_hook is not None:
      self.grad_ready_hook(self)
    return self.conv.bwd(c_conv, Act(dh.view(h.t.shape), h.C), need_dx, need_dw)


class StageDepth(object):
  """The fourth item of a HipResidualVQBottleneck context that was made with a depth map: told from a dhist
  tensor by its type, not by the context's length."""
  __slots__ = ('depth',)

  def __init__(self, depth):
    self.depth = depth


class HipResidualVQBottleneck(nn.Module):
  """The residual (multi-stage) quantizer as the encoder's bottleneck: HipVQBottleneck's sibling with S code
  books.  A 1x1 conv (`conv`: `<prefix>.conv.weight`) and a ResidualS2HVQ (`vq`: `<prefix>.vq._code_books` [S, n_center,
  center_size]) on the same [M][D] view of the conv's NHWC output, under the same geometry check.

  Forward: always the hard form, over the first `stages` books (ops.vq_res_rows_fwd); backward: the soft form's gradient at
  every stage (ops.vq_res_bwd), books beyond `stages` getting zeros.  The soft forward and the cost walks are built for one
  stage only and are not methods of this layer; the entropy-constrained code and the usage counts are the multi-stage ones of
  DESIGN.md 4.25 (code_ec, usage).
  Rate term: with `rate_scale` set by the owner (rate_denom with it) a training forward is ONE
  ops.vq_res_rate_fwd(want_code=True) call on the conv's output -- y and index are ops.vq_res_rows_fwd's bit for bit, the unscaled
  total stays in `rate_value` (fp32 [1]), the per-stage values in `rate_stage_values` (fp32 [stages]), and dhist, scaled by
  rate_scale, travels with the context into the grouped backward.  With rate_scale None every call is the one above.
  Stage depth: with `depth` set by the owner for a call -- int32 [N * h * w] on the device, one value per pixel of
  the feature map, whose `groups` consecutive vectors form a cell -- fwd, code, decode and bwd run the depth forms of the same
  kernels: a vector takes its first min(stages, depth) stages, its code is -1 beyond.  Not together with rate_scale.  With depth
  None every call is the one above.
  Books: stage s is (2 * torch.rand(n_center, center_size) - 1) * 0.5 ** s from a CPU torch.Generator seeded with seed + s --
  the same books on every device and rank; load_state_dict replaces them."""

  def __init__(self, cin, cout, n_center=64, center_size=8, n_stages=2, sigma=10.0, dtype=F32, device=None, seed=0):
    super(HipResidualVQBottleneck, self).__init__()
    n_center, center_size, n_stages = int(n_center), int(center_size), int(n_stages)
    vq_bottleneck_check(cout, n_center, center_size, sigma, who='HipResidualVQBottleneck')
    if not 1 <= n_stages <= ops.VQ_RES_MAX_STAGES:
      raise ValueError('HipResidualVQBottleneck: %d stages, the kernels take 1 .. %d' % (n_stages, ops.VQ_RES_MAX_STAGES))
    from ctu.quantizers.residual_s2h_vq import ResidualS2HVQ
    books = torch.stack([(2 * torch.rand(n_center, center_size, generator=torch.Generator().manual_seed(int(seed) + s)) - 1) * 0.5 ** s
                         for s in range(n_stages)])
    self.conv = HipConv2d(cin, cout, 1, act=ACT_NONE, apply_bias=False, bias=False, dtype=dtype, device=device)
    self.vq = ResidualS2HVQ(books.to(device) if device is not None else books, sigma=float(sigma))
    self.cout, self.center_size, self.n_center, self.n_stages = cout, center_size, n_center, n_stages
    self.hard_forward = True
    self.grad_ready_hook = None
    self.train_stages = None      # the owner's stage count for the next training forward (None: all); eval ignores it
    self.rate_scale, self.rate_denom, self.rate_value, self.rate_stage_values = None, 0, None, None
    self.depth = None             # the owner's per-pixel stage depth for the next calls (None: every stage everywhere)

  @property
  def groups(self):
    return self.cout // self.center_size

  def _books(self):
    c = self.vq._code_books
    assert c.dtype == torch.float32 and c.is_contiguous(), 'the code books must be contiguous fp32'
    return c

  def _cgrad_buffer(self):
    c = self._books()
    if c.grad is None or not c.grad.is_contiguous():
      c.grad = torch.zeros_like(c)
    return c.grad

  def ensure_grads(self):
    if self.vq._code_books.requires_grad:
      self._cgrad_buffer()

  def _stages(self, stages):
    n = self.n_stages if stages is None else stages
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= self.n_stages:
      raise ValueError('stages must be an int in 1 .. %d, got %r' % (self.n_stages, stages))
    return n

  def _quantize(self, h, n):
    if self.depth is not None:
      y, index = ops.vq_res_rows_fwd(h.t.view(-1, self.center_size), self._books().detach(), n, depth=self.depth, groups=self.groups)
    else:
      y, index = ops.vq_res_rows_fwd(h.t.view(-1, self.center_size), self._books().detach(), n)
    return Act(y.view(h.t.shape), h.C), index

  def fwd(self, x, stages=None):
    if stages is None and self.training:
      stages = self.train_stages
    n = self._stages(stages)
    h, c_conv = self.conv.fwd(x)
    if self.depth is not None:
      if self.rate_scale is not None:
        raise ValueError('HipResidualVQBottleneck: depth and rate_scale cannot be combined (the rate term has no depth form)')
      y, index = self._quantize(h, n)
      return y, Ctx(c_conv, h, index, StageDepth(self.depth))
    if self.rate_scale is not None:
      # opt.lambda_vq_stage_rate: the owner set rate_scale / rate_denom for this call; one kernel gives the code
      # and the histograms of the stages in use, and the gradient w.r.t. those sums travels with the context
      self.rate_value, self.rate_stage_values, _, dhist, y, index = ops.vq_res_rate_fwd(
          h.t.view(-1, self.center_size), self._books().detach(), self.vq.sigma, self.groups, self.rate_denom, self.rate_scale,
          n_stages=n, want_code=True)
      return Act(y.view(h.t.shape), h.C), Ctx(c_conv, h, index, dhist)
    y, index = self._quantize(h, n)
    return y, Ctx(c_conv, h, index)

  def features(self, x):
    """The 1x1 conv's output as the [M, D] matrix the quantizer sees (a view, in the layer's dtype)."""
    h, _ = self.conv.fwd(x)
    return h.t.view(-1, self.center_size)

  def fit(self, feature_matrices, n_iter=10, init='sample', seed=0, reseed=True):
    """Fit the books stage by stage to feature matrices as features() returns them (a list of [M, D] tensors, concatenated):
    ResidualS2HVQ.fit with code_len 1, in place.  Returns the list of per-stage reports."""
    x = feature_matrices if torch.is_tensor(feature_matrices) else torch.cat(list(feature_matrices), dim=0)
    return self.vq.fit(x, 1, n_iter=n_iter, init=init, seed=seed, reseed=reseed)

  def code(self, x, stages=None):
    """int32 [N, stages, h * w * cout / D]: per image, the stage-major indices of every vector of x's features."""
    n = self._stages(stages)
    h, _ = self.conv.fwd(x)
    _, index = self._quantize(h, n)
    return index.view(n, h.N, -1).transpose(0, 1).contiguous()

  def code_ec(self, x, lam, n_iter=2, stages=None):
    """(index, reports): code() under the entropy constraint -- ResidualS2HVQ.encode_ec PER IMAGE on that
    image's rows of features(x), groups = the channel groups, as HipVQBottleneck.code_ec: the coders adapt per image, so the
    histograms are per image.  index int32 [N, stages, h * w * cout / D]; reports: the N report dicts of encode_ec."""
    n = self._stages(stages)
    f = self.features(x)
    N = x.N
    rows = f.shape[0] // N
    codes, reports = [], []
    for i in range(N):
      code, report = self.vq.encode_ec(f[i * rows:(i + 1) * rows], 1, lam, groups=self.groups, n_iter=n_iter, stages=n)
      codes.append(code.view(n, rows))
      reports.append(report)
    return torch.stack(codes, dim=0).to(torch.int32), reports

  def usage(self, x):
    """int64 [S, groups, n_center]: how many vectors of x's features take each centre at each stage of code(x), per channel
    group, over the batch (ResidualS2HVQ.usage)."""
    return self.vq.usage(self.features(x), 1, groups=self.groups)

  def decode(self, index, N, h, w, dtype_code):
    """The features Act [N, h, w, cout] of an index tensor int32 [N, S', per-image indices], 1 <= S' <= S, as code() returns it
    or a stage prefix of it (ops.vq_res_decode: bit for bit the forward over S' stages) and the decoder's status word."""
    from .ops import tdtype_of
    assert index.dim() == 3 and int(index.shape[0]) == N and 1 <= int(index.shape[1]) <= self.n_stages, tuple(index.shape)
    planes = index.transpose(0, 1).contiguous().view(int(index.shape[1]), -1)
    if self.depth is not None:
      y, status = ops.vq_res_decode(planes, self._books().detach(), dtype=tdtype_of(dtype_code), depth=self.depth, groups=self.groups)
    else:
      y, status = ops.vq_res_decode(planes, self._books().detach(), dtype=tdtype_of(dtype_code))
    return Act(y.view(N, h, w, self.cout), self.cout), status

  def bwd(self, ctx, dy, need_dx=True, need_dw=True):
    """dy: the gradient w.r.t. the quantized features.  Straight-through: the soft form's gradient at every stage of the forward
    (DESIGN.md 4.23), zeros for the books it did not use, then the 1x1 conv's data / weight gradients."""
    c_conv, h, index = ctx.items[:3]
    D = self.center_size
    books = self._books()
    want_dc = need_dw and books.requires_grad
    extra = ctx.items[3] if len(ctx.items) > 3 else None
    if isinstance(extra, StageDepth):
      # a forward with a depth map: the per-row recursion under the map the FORWARD used, which travels with the
      # context -- code and decode read self.depth at the time of their call, the owner may have unset it since
      dh, _ = ops.vq_res_bwd(dy.t.view(-1, D), h.t.view(-1, D), books.detach(), index, self.vq.sigma, want_dx=True,
                             want_dc=want_dc, dc_out=self._cgrad_buffer() if want_dc else None, groups=self.groups,
                             depth=extra.depth)
    elif extra is not None:    # a forward with a rate scale: its dhist joins dp of every stage in the grouped backward
      dh, _ = ops.vq_res_bwd(dy.t.view(-1, D), h.t.view(-1, D), books.detach(), index, self.vq.sigma, want_dx=True,
                             want_dc=want_dc, dc_out=self._cgrad_buffer() if want_dc else None, groups=self.groups,
                             dhist=ctx.items[3])
    else:
      dh, _ = ops.vq_res_bwd(dy.t.view(-1, D), h.t.view(-1, D), books.detach(), index, self.vq.sigma, want_dx=True,
                             want_dc=want_dc, dc_out=self._cgrad_buffer() if want_dc else None)
    if want_dc and self.grad_ready_hook is not None:
      self.grad_ready_hook(self)
    return self.conv.bwd(c_conv, Act(dh.view(h.t.shape), h.C), need_dx, need_dw)


class PackBatcher(object):
  """Re-packs the data-gradient panels of all conv layers of one network in ONE launch right after its
  optimizer step (jpdse_conv_pack_run); layers it cannot cover keep their lazy per-layer pack."""

  def __init__(self, net):
    self.net = net
    self._table = {}

  def run(self):
    layers, entries = [], []
    for m in self.net.modules():
      if isinstance(m, HipConv2d):
        e = m.batched_pack_entries()
        if e:
          layers.append(m)
          entries.extend(e)
    if not entries:
      return 0
    sig = tuple((e.w, e.out) for e in entries)
    ops.conv_pack_run(*ops.device_table(self._table, 0, sig, lambda: ops.conv_pack_table(entries), layers[0].weight.device))
    for m in layers:
      m._panels.mark_fresh(m.weight)
    return len(layers)


class InstNormAct(object):
  """InstanceNorm2d(affine=False, eps=1e-5) + {none, ReLU, LeakyReLU(0.2)} (+ residual)."""

  def __init__(self, act=ACT_NONE, slope=0.2, eps=1e-5):
    self.act, self.slope, self.eps = act, slope, eps

  def fwd(self, x, residual=None):
    y, stats = ops.inorm_fwd(x, self.act, self.slope, self.eps, residual)
    return y, Ctx(x, stats)

  def fwd_from_moments(self, x, mom, slots, residual=None):
    y, stats = ops.inorm_fwd_from_moments(x, mom, slots, self.act, self.slope, self.eps, residual)
    return y, Ctx(x, stats)

  def bwd(self, ctx, dy, need_dx=True, need_dw=True):
    x, stats = ctx.items
    return ops.inorm_bwd(x, stats, dy, self.act, self.slope, self.eps)     # takes dy.nsums when the producer of dy wrote them

  def sink(self, ctx):
    """What the producer of this norm's dy needs to write the backward sums in its epilogue (HipConv2d.bwd sink=)."""
    x, stats = ctx.items
    return (x, stats, self.act, self.slope)


def conv_norm_fwd(conv, norm, x, residual=None):
  """conv -> InstanceNorm (+ activation / residual): (y, conv ctx, norm ctx).  The norm's moment pass runs in the conv's epilogue
  when its kernel has one (jpdse_conv_fwd_moments: the halo kernel of the full-width blocks), leaving ONE kernel per norm."""
  fused = conv.fwd_moments(x)
  if fused is not None:
    h, c, mom, slots = fused
    y, n = norm.fwd_from_moments(h, mom, slots, residual=residual)
    return y, c, n
  h, c = conv.fwd(x)
  y, n = norm.fwd(h, residual=residual)
  return y, c, n


class ConvNormAct(object):
  """[pad] conv -> InstanceNorm -> activation: one stage of the generator trunk / PatchGAN.
  A plain object (not an nn.Module) so the conv is registered once, under its reference key."""

  def __init__(self, conv, norm):
    self.conv, self.norm = conv, norm

  def fwd(self, x):
    y, c1, c2 = conv_norm_fwd(self.conv, self.norm, x)
    return y, Ctx(c1, c2)

  def bwd(self, ctx, dy, need_dx=True, need_dw=True, addend=None, **conv_kw):
    c1, c2 = ctx.items
    dh = self.norm.bwd(c2, dy)
    return self.conv.bwd(c1, dh, need_dx, need_dw, addend=addend, **conv_kw)

  def bwd_batched(self, ctx, dy, B, later, addend=None, **conv_kw):
    """HipConv2d.bwd_batched behind the norm's backward over the same 3B gradient images (jpdse_inorm_bwd with the descriptor's alias)."""
    c1, c2 = ctx.items
    x, stats = c2.items
    dh = ops.inorm_bwd_aliased(x, stats, dy, B, self.norm.act, self.norm.slope, self.norm.eps)
    return self.conv.bwd_batched(c1, dh, B, later, addend=addend, **conv_kw)

  def dy_sink(self, ctx):
    """The norm that consumes the gradient handed to bwd(): run_chain_bwd passes it to the stage that produces that gradient."""
    return self.norm.sink(ctx.items[1])


class _Slot(nn.Module):
  """Parameter-free placeholder keeping nn.Sequential indices equal to the reference's."""

  def forward(self, x):
    return x


class HipResnetBlock(nn.Module):
  """x + IN(conv3(reflpad(ReLU(IN(conv3(reflpad(x)))))))   (networks.py:266-305)."""

  def __init__(self, dim, dtype=F32, device=None):
    super(HipResnetBlock, self).__init__()
    mk = lambda: HipConv2d(dim, dim, 3, 1, 1, PAD_REFLECT, apply_bias=False, dtype=dtype, device=device)
    self.conv_block = nn.Sequential(_Slot(), mk(), _Slot(), _Slot(), _Slot(), mk(), _Slot())
    self.norm1 = InstNormAct(ACT_RELU)
    self.norm2 = InstNormAct(ACT_NONE)

  # Activation checkpointing (BASELINE config 5): keep only the block's input and run the forward again
  # inside backward.  Off by default -- 288 GB of HBM hold every activation of the 2048x1024 step -- and, the
  # kernels being deterministic, bit-identical to the stored-activation path when on (tests/test_hip_configs.py).
  recompute = False

  def _fwd(self, x):
    h, c1, n1 = conv_norm_fwd(self.conv_block[1], self.norm1, x)
    y, c2, n2 = conv_norm_fwd(self.conv_block[5], self.norm2, h, residual=x)
    return y, Ctx(c1, n1, c2, n2)

  def fwd(self, x):
    y, ctx = self._fwd(x)
    return (y, Ctx(x)) if self.recompute else (y, ctx)

  accepts_dx_sink = True

  def bwd(self, ctx, dy, need_dx=True, need_dw=True, dx_sink=None):
    """dx_sink: the InstanceNorm that consumes the returned gradient (the previous stage's, see dy_sink): the sums of its
    backward are then written by the epilogue of this block's first conv's data gradient; likewise norm1's by the second conv's
    -- no separate pass over (x, dy) for either (jpdse_conv_dgrad_fused_nsums)."""
    ctx = self.materialize(ctx)
    c1, n1, c2, n2 = ctx.items
    d = self.norm2.bwd(n2, dy)
    d = self.conv_block[5].bwd(c2, d, True, need_dw, sink=self.norm1.sink(n1) if self.fuse_norm_sums else None)
    d = self.norm1.bwd(n1, d)
    # the skip connection's gradient is summed in the data-gradient epilogue of the first conv
    return self.conv_block[1].bwd(c1, d, need_dx, need_dw, addend=dy if need_dx else None,
                                  sink=dx_sink if self.fuse_norm_sums else None)

  fuse_norm_sums = True       # False (A/B, tests): every norm backward computes its sums in its own pass

  def materialize(self, ctx):
    """The block's saved tensors: `ctx` itself, or -- checkpointed block (ctx holds only the block input) -- rebuilt by running
    the block's forward again.  run_chain_bwd calls this one stage early so that the stage above can be told about this block's
    second norm (dy_sink) in the checkpointed run exactly as in the stored-activation run: same kernels, bit-identical step."""
    if len(ctx.items) == 1:
      _, ctx = self._fwd(ctx.items[0])
    return ctx

  def dy_sink(self, ctx):
    if len(ctx.items) == 1:                     # checkpointed and not materialized
      return None
    return self.norm2.sink(ctx.items[3])


def run_chain_fwd(stages, x):
  ctxs = []
  for st in stages:
    x, c = st.fwd(x)
    ctxs.append(c)
  return x, ctxs


def run_chain_bwd(stages, ctxs, dy, need_dx=True, need_dw=True):
  """Back-propagate through `stages`; the first stage computes dx only when need_dx."""
  pending = None          # stage i - 1's saved tensors, materialized while stage i runs (the caller's list is left alone)
  for i in range(len(stages) - 1, -1, -1):
    ctx_i, pending = (pending if pending is not None else ctxs[i]), None
    below = None
    if i > 0 and hasattr(stages[i - 1], 'materialize'):
      below = pending = stages[i - 1].materialize(ctxs[i - 1])   # a checkpointed block's tensors, one stage early (see there)
    elif i > 0:
      below = ctxs[i - 1]
    if i > 0 and getattr(stages[i], 'accepts_dx_sink', False) and hasattr(stages[i - 1], 'dy_sink'):
      # stage i's dx goes straight into the InstanceNorm backward of stage i - 1: let its data-gradient epilogue write that
      # norm's sums (HipResnetBlock.bwd)
      dy = stages[i].bwd(ctx_i, dy, True, need_dw, dx_sink=stages[i - 1].dy_sink(below))
    else:
      dy = stages[i].bwd(ctx_i, dy, need_dx or i > 0, need_dw)
  return dy
