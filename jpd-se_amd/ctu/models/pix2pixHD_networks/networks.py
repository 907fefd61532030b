"""MI355X-native pix2pixHD networks behind the reference's `networks` interface.

Drop-in for /root/reference/ctu/models/pix2pixHD_networks/networks.py: same factory
signatures (`define_G` :38-56, `define_D` :58-66), same class names, same `state_dict`
keys/shapes.  Every layer runs as a hand-written gfx950 kernel through
libjpdse_hip.so; there is no torch.nn compute and no CPU fallback.

Two entry styles per network:
  * `net(x)` -- reference style: fp32 NCHW cuda tensor in, fp32 NCHW tensor(s) out (inference);
  * `net.fwd(act)` / `net.bwd(...)` -- NHWC `Act` in/out with an explicit backward, used by
    `Pix2PixHDModel`'s train-step schedule.
"""
import torch
import torch.nn as nn

from jpdse_hip import (ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, PAD_ZERO, PAD_REFLECT, F32, BF16, JpdseError,
                       require_gpu)
from jpdse_hip import ops
from jpdse_hip.ops import Act
from jpdse_hip.layers import (HipConv2d, HipResnetBlock, HipBinarizer, HipVQBottleneck, HipResidualVQBottleneck, vq_bottleneck_check, InstNormAct,
                              ConvNormAct, Ctx, _Slot,
                              run_chain_fwd, run_chain_bwd)

ResnetBlock = HipResnetBlock

VGG_CFG = (64, 64, 'M', 128, 128, 'M', 256, 256, 256, 256, 'M', 512, 512, 512, 512, 'M', 512)
VGG_TAPS = (0, 2, 4, 8, 12)


def dtype_code(name):
  if name in (F32, BF16):
    return name
  table = {'fp32': F32, 'float32': F32, 'f32': F32, 'bf16': BF16, 'bfloat16': BF16}
  if name not in table:
    raise ValueError('compute dtype must be fp32 or bf16, got %r' % (name,))
  return table[name]


def get_norm_layer(norm_type='instance'):
  """Only the reference default is on the accelerated path (networks.py:27-36)."""
  if norm_type != 'instance':
    raise NotImplementedError('normalization layer [%s] is not implemented on the HIP path '
                              '(per-image data parallelism relies on InstanceNorm: SURVEY.md §8e)' % norm_type)
  return InstNormAct


def weights_init(m):
  """N(0, 0.02) on every conv weight (networks.py:19-25)."""
  if isinstance(m, HipConv2d):
    m.weight.data.normal_(0.0, 0.02)


def _to_act(x, dtype):
  if isinstance(x, Act):
    return x
  if not (torch.is_tensor(x) and x.is_cuda):
    raise JpdseError('HIP networks take cuda tensors (no CPU fallback); got %r' % (type(x),))
  return ops.nchw_to_nhwc(x.float().contiguous(), dtype)


# =============================================================================================
# generators
# =============================================================================================
def _global_indices(n_down, n_blocks):
  first = 1
  down = [4 + 3 * i for i in range(n_down)]
  res = [4 + 3 * n_down + b for b in range(n_blocks)]
  up = [4 + 3 * n_down + n_blocks + 3 * i for i in range(n_down)]
  last = 4 + 3 * n_down + n_blocks + 3 * n_down + 1
  return first, down, res, up, last


def _build_global(input_nc, output_nc, ngf, n_down, n_blocks, dtype, device, with_head=True):
  """Returns (nn.Sequential with reference indices, trunk stage list, head stage or None)."""
  first, down, res, up, last = _global_indices(n_down, n_blocks)
  total = last + 2 if with_head else last - 1     # drop [ReflPad, Conv7, Tanh] for the enhancer's core
  slots = [_Slot() for _ in range(total)]
  kw = dict(dtype=dtype, device=device)
  stages = []
  slots[first] = HipConv2d(input_nc, ngf, 7, 1, 3, PAD_REFLECT, apply_bias=False, **kw)
  stages.append(ConvNormAct(slots[first], InstNormAct(ACT_RELU)))
  for i, idx in enumerate(down):
    c = ngf * 2 ** i
    slots[idx] = HipConv2d(c, 2 * c, 3, 2, 1, PAD_ZERO, apply_bias=False, **kw)
    stages.append(ConvNormAct(slots[idx], InstNormAct(ACT_RELU)))
  dim = ngf * 2 ** n_down
  for idx in res:
    slots[idx] = HipResnetBlock(dim, **kw)
    stages.append(slots[idx])
  for i, idx in enumerate(up):
    c = ngf * 2 ** (n_down - i)
    slots[idx] = HipConv2d(c, c // 2, 3, 2, 1, transposed=True, apply_bias=False, **kw)
    stages.append(ConvNormAct(slots[idx], InstNormAct(ACT_RELU)))
  head = None
  if with_head:
    slots[last] = HipConv2d(ngf, output_nc, 7, 1, 3, PAD_REFLECT, act=ACT_TANH, apply_bias=True, **kw)
    head = slots[last]
  return nn.Sequential(*slots), stages, head


class GlobalGenerator(nn.Module):
  """networks.py:198-251 (binarizer branches are outside the JPD-SE flag subset)."""

  def __init__(self, input_nc, output_nc, ngf=64, n_downsampling=3, n_blocks=9, norm_layer=None,
               padding_type='reflect', binarize=False, binarizer_out_channels=128, bin_before_res=True,
               compute_dtype='fp32', device=None):
    super(GlobalGenerator, self).__init__()
    assert n_blocks >= 0
    if binarize:
      raise NotImplementedError('generator binarization is outside the JPD-SE hot path (SURVEY.md §2 row 3)')
    if padding_type != 'reflect':
      raise NotImplementedError('padding [%s] is not implemented' % padding_type)
    self.binarize = False
    self.n_downsampling, self.n_blocks = n_downsampling, n_blocks
    self.input_nc, self.output_nc = input_nc, output_nc
    self.cdtype = dtype_code(compute_dtype)
    self.model, stages, head = _build_global(input_nc, output_nc, ngf, n_downsampling, n_blocks, self.cdtype,
                                             device)
    self._stages = stages + [head]

  def fwd(self, x):
    return run_chain_fwd(self._stages, x)

  def bwd(self, ctxs, dy, need_dx=False, need_dw=True, dx_channels=None):
    """dx_channels=(c0, c1): also return the gradient w.r.t. input channels [c0, c1) only -- the encoded features of the
    learned codec (pix2pixHD_model.py:595: torch.cat((input_label, feat_map))); the first conv's data gradient is then
    restricted to those channels (HipConv2d.bwd_input_slice), the label channels need none."""
    if dx_channels is None:
      return run_chain_bwd(self._stages, ctxs, dy, need_dx, need_dw)
    d = run_chain_bwd(self._stages[1:], ctxs[1:], dy, True, need_dw)
    first = self._stages[0]
    c_conv, c_norm = ctxs[0].items
    dh = first.norm.bwd(c_norm, d)
    first.conv.bwd(c_conv, dh, False, need_dw)
    return first.conv.bwd_input_slice(c_conv, dh, dx_channels[0], dx_channels[1])

  def forward(self, input, mode='get_continuous_img'):
    if mode == 'get_binary_code':
      raise AttributeError('Generator: no binarizer found')
    if mode != 'get_continuous_img':
      raise ValueError('Invalid generator mode: {}'.format(mode))
    y, _ = self.fwd(_to_act(input, self.cdtype))
    return ops.nhwc_to_nchw(y)


class LocalEnhancer(nn.Module):
  """networks.py:144-196: coarse GlobalGenerator(ngf*2^n) core on the pooled input, then per
  enhancer [ReflPad3,Conv7,IN,ReLU,Conv3s2,IN,ReLU](full-res) + coarse -> ResBlocks -> ConvT."""

  def __init__(self, input_nc, output_nc, ngf=32, n_downsample_global=3, n_blocks_global=9, n_local_enhancers=1,
               n_blocks_local=3, norm_layer=None, padding_type='reflect', compute_dtype='fp32', device=None):
    super(LocalEnhancer, self).__init__()
    if padding_type != 'reflect':
      raise NotImplementedError('padding [%s] is not implemented' % padding_type)
    self.n_local_enhancers = n_local_enhancers
    self.input_nc, self.output_nc = input_nc, output_nc
    self.cdtype = dtype_code(compute_dtype)
    kw = dict(dtype=self.cdtype, device=device)
    self.model, self._core, _ = _build_global(input_nc, output_nc, ngf * 2 ** n_local_enhancers,
                                              n_downsample_global, n_blocks_global, self.cdtype, device,
                                              with_head=False)
    self._down, self._up = {}, {}
    for n in range(1, n_local_enhancers + 1):
      g = ngf * 2 ** (n_local_enhancers - n)
      c7 = HipConv2d(input_nc, g, 7, 1, 3, PAD_REFLECT, apply_bias=False, **kw)
      c3 = HipConv2d(g, 2 * g, 3, 2, 1, PAD_ZERO, apply_bias=False, **kw)
      setattr(self, 'model%d_1' % n, nn.Sequential(_Slot(), c7, _Slot(), _Slot(), c3, _Slot(), _Slot()))
      self._down[n] = [ConvNormAct(c7, InstNormAct(ACT_RELU)), ConvNormAct(c3, InstNormAct(ACT_RELU))]
      blocks = [HipResnetBlock(2 * g, **kw) for _ in range(n_blocks_local)]
      ct = HipConv2d(2 * g, g, 3, 2, 1, transposed=True, apply_bias=False, **kw)
      mods = blocks + [ct, _Slot(), _Slot()]
      stages = blocks + [ConvNormAct(ct, InstNormAct(ACT_RELU))]
      if n == n_local_enhancers:
        head = HipConv2d(ngf, output_nc, 7, 1, 3, PAD_REFLECT, act=ACT_TANH, apply_bias=True, **kw)
        mods += [_Slot(), head, _Slot()]
        stages.append(head)
      setattr(self, 'model%d_2' % n, nn.Sequential(*mods))
      self._up[n] = stages

  def fwd(self, x):
    nl = self.n_local_enhancers
    pyramid = [x]
    for _ in range(nl):
      pyramid.append(ops.avgpool3s2_fwd(pyramid[-1]))
    out, core_ctx = run_chain_fwd(self._core, pyramid[-1])
    levels = []
    for n in range(1, nl + 1):
      h, dctx = run_chain_fwd(self._down[n], pyramid[nl - n])
      h = ops.add_(h, out)
      out, uctx = run_chain_fwd(self._up[n], h)
      levels.append((dctx, uctx))
    return out, (core_ctx, levels)

  def bwd(self, ctxs, dy, need_dx=False, need_dw=True):
    if need_dx:
      raise NotImplementedError('gradient w.r.t. the generator input is never needed on this path')
    core_ctx, levels = ctxs
    for n in range(self.n_local_enhancers, 0, -1):
      dctx, uctx = levels[n - 1]
      dh = run_chain_bwd(self._up[n], uctx, dy, True, need_dw)
      run_chain_bwd(self._down[n], dctx, dh, False, need_dw)
      dy = dh                       # the sum feeds both branches
    if any(p.requires_grad for p in self.model.parameters()):     # frozen during the niter_fix_global phase
      run_chain_bwd(self._core, core_ctx, dy, False, need_dw)
    return None

  def forward(self, input):
    y, _ = self.fwd(_to_act(input, self.cdtype))
    return ops.nhwc_to_nchw(y)


class Encoder(nn.Module):
  """Feature encoder of the learned codec (networks.py:307-369): [ReflPad3, Conv7, IN, ReLU], n x [Conv3 s2, IN, ReLU],
  the Binarizer (optional: the bitstream), n x [ConvT3 s2, IN, ReLU], [ReflPad3, Conv7, Tanh].  Same Sequential indices as
  the reference, so `state_dict()` keys / shapes equal a reference net_E.pth (every conv carries its bias; the ones in
  front of an affine-less InstanceNorm are not applied -- the norm cancels them).
  quantizer='s2hvq' (extension): the bottleneck slot holds a HipVQBottleneck -- 1x1 conv and soft-to-hard vector
  quantizer over groups of vq_center_size channels -- instead of the Binarizer; binarizer_out_channels still names the
  bottleneck's channel count.  Its code is vq_code / decode_vq_code; code / code_shape / decode_code stay the binarizer's.
  vq_stages > 1: the slot holds a HipResidualVQBottleneck of that many code books; vq_code is then int32
  [N, stages, indices] and every stage prefix of it decodes."""

  QUANTIZERS = ('binarizer', 's2hvq')

  def __init__(self, input_nc, output_nc, ngf=32, n_downsampling=4, norm_layer=None, binarize=False,
               binarizer_out_channels=128, groups=1, compute_dtype='fp32', device=None, quantizer='binarizer',
               vq_n_center=64, vq_center_size=8, vq_sigma=10.0, vq_hard_forward=True, vq_stages=1):
    super(Encoder, self).__init__()
    if quantizer not in self.QUANTIZERS:
      raise ValueError('Encoder: quantizer must be one of %s, got %r' % (self.QUANTIZERS, quantizer))
    self.quantizer = quantizer if binarize else None
    if self.quantizer == 's2hvq':          # before any layer exists
      vq_bottleneck_check(binarizer_out_channels, int(vq_n_center), int(vq_center_size), vq_sigma, 'Encoder')
    if groups != 1:
      raise NotImplementedError('grouped encoder convolutions (--netE_groups != 1) are not implemented on the HIP path')
    if n_downsampling < 1:
      raise NotImplementedError('an encoder without downsampling (--n_downsample_E 0) is not implemented on the HIP path')
    self.output_nc, self.binarize, self.n_downsampling = output_nc, binarize, n_downsampling
    self.cdtype = dtype_code(compute_dtype)
    kw = dict(dtype=self.cdtype, device=device)
    n, B = n_downsampling, binarizer_out_channels
    o = 4 + 3 * n + (1 if binarize else 0)            # first up-sampling conv
    last = o + 3 * n + 1
    slots = [_Slot() for _ in range(last + 2)]
    slots[1] = HipConv2d(input_nc, ngf, 7, 1, 3, PAD_REFLECT, apply_bias=False, **kw)
    self._pre = [ConvNormAct(slots[1], InstNormAct(ACT_RELU))]
    for i in range(n):
      c = ngf * 2 ** i
      slots[4 + 3 * i] = HipConv2d(c, 2 * c, 3, 2, 1, PAD_ZERO, apply_bias=False, **kw)
      self._pre.append(ConvNormAct(slots[4 + 3 * i], InstNormAct(ACT_RELU)))
    if binarize and quantizer == 's2hvq' and int(vq_stages) > 1:
      if not vq_hard_forward:
        raise ValueError('Encoder: vq_stages = %d with the soft forward, which is built for one stage' % int(vq_stages))
      slots[4 + 3 * n] = HipResidualVQBottleneck(ngf * 2 ** n, B, vq_n_center, vq_center_size, int(vq_stages), vq_sigma, **kw)
    elif binarize and quantizer == 's2hvq':
      slots[4 + 3 * n] = HipVQBottleneck(ngf * 2 ** n, B, vq_n_center, vq_center_size, vq_sigma, vq_hard_forward, **kw)
    elif binarize:
      slots[4 + 3 * n] = HipBinarizer(ngf * 2 ** n, B, **kw)
    self._post = []
    for i in range(n):
      c = ngf * 2 ** (n - i)
      cin = B if (i == 0 and binarize) else c
      slots[o + 3 * i] = HipConv2d(cin, c // 2, 3, 2, 1, transposed=True, apply_bias=False, **kw)
      self._post.append(ConvNormAct(slots[o + 3 * i], InstNormAct(ACT_RELU)))
    slots[last] = HipConv2d(ngf, output_nc, 7, 1, 3, PAD_REFLECT, act=ACT_TANH, apply_bias=True, **kw)
    self._post.append(slots[last])
    self.model = nn.Sequential(*slots)

  @property
  def _binarizer(self):
    """model[4 + 3n] (a property, so the module is registered once, under its reference key)."""
    return self.model[4 + 3 * self.n_downsampling] if self.quantizer == 'binarizer' else None

  @property
  def _vq(self):
    """model[4 + 3n] when it is the vector-quantizer bottleneck."""
    return self.model[4 + 3 * self.n_downsampling] if self.quantizer == 's2hvq' else None

  @property
  def _bottleneck(self):
    return self.model[4 + 3 * self.n_downsampling] if self.quantizer is not None else None

  def fwd(self, x):
    """(features, ctx); the bottleneck's mode follows its `training` flag."""
    h, c_pre = run_chain_fwd(self._pre, x)
    c_bin = None
    if self._bottleneck is not None:
      h, c_bin = self._bottleneck.fwd(h)
    y, c_post = run_chain_fwd(self._post, h)
    return y, (c_pre, c_bin, c_post)

  def bwd(self, ctxs, dy, need_dw=True):
    """Weight gradients of every layer from dy = d loss / d features.  No gradient w.r.t. the encoder input (the image)."""
    c_pre, c_bin, c_post = ctxs
    d = run_chain_bwd(self._post, c_post, dy, True, need_dw)
    if self._bottleneck is not None:
      d = self._bottleneck.bwd(c_bin, d, True, need_dw)
    run_chain_bwd(self._pre, c_pre, d, False, need_dw)

  def code(self, x):
    """The binarizer's output (+-1; 0 where eval-mode tanh is exactly 0) as an NHWC Act: model[:4 + 3n + 1](x)."""
    binarizer = self._require_binarizer()
    h, _ = run_chain_fwd(self._pre, x)
    b, _ = binarizer.fwd(h)
    return b

  def code_shape(self, H, W):
    """(C, h, w) of the code of an H x W image: the binarizer's channels at 1 / 2^n of the resolution."""
    n = self.n_downsampling
    return (self._require_binarizer().conv.cout, H >> n, W >> n)

  def decode_code(self, b):
    """The receiver's half: features from a code Act (+-1, e.g. ops.code_import of a stored bitstream): model[4 + 3n + 1:](b)."""
    self._require_binarizer()
    y, _ = run_chain_fwd(self._post, b)
    return y

  def _require_binarizer(self):
    if self._binarizer is None:
      raise AttributeError('Encoder: no binarizer found')
    return self._binarizer

  def _require_vq(self):
    if self._vq is None:
      raise AttributeError('Encoder: no vector quantizer found (quantizer=%r)' % (self.quantizer,))
    return self._vq

  @property
  def vq_stages(self):
    """Code books of the vector-quantizer bottleneck: 1 for HipVQBottleneck."""
    return getattr(self._require_vq(), 'n_stages', 1)

  def vq_code_len(self, H, W):
    """Indices per image AND STAGE of an H x W input: (H / 2^n) (W / 2^n) cout / D."""
    vq, n = self._require_vq(), self.n_downsampling
    return (H >> n) * (W >> n) * (vq.cout // vq.center_size)

  def vq_code(self, x, stages=None):
    """int32 [N, h * w * cout / D]: the nearest centre of every channel group of every pixel of the bottleneck's features, pixel
    by pixel, groups ascending inside a pixel: model[:4 + 3n + 1](x) as indices.  With vq_stages > 1: int32 [N, stages, h * w *
    cout / D], the first `stages` (default: all) stages; with one stage `stages` must be None or 1."""
    vq = self._require_vq()
    if self.vq_stages == 1:
      if stages not in (None, 1) or isinstance(stages, bool):
        raise ValueError('Encoder.vq_code: stages = %r, the bottleneck has one stage (vq_stages = 1)' % (stages,))
      h, _ = run_chain_fwd(self._pre, x)
      return vq.code(h)
    vq._stages(stages)                     # before any device work
    h, _ = run_chain_fwd(self._pre, x)
    return vq.code(h, stages)

  def vq_code_ec(self, x, lam, n_iter=2):
    """(index, reports): vq_code under the entropy constraint: the first half runs once, then the bottleneck's
    code_ec assigns image by image with the rate multiplier lam."""
    vq = self._require_vq()
    h, _ = run_chain_fwd(self._pre, x)
    return vq.code_ec(h, lam, n_iter)

  def _require_stages(self, who):
    vq = self._require_vq()
    if self.vq_stages == 1:
      raise ValueError('Encoder.%s: a call of the residual bottleneck, this one has one stage (vq_stages = 1)' % who)
    return vq

  def vq_stage_code_ec(self, x, lam, n_iter=2, stages=None):
    """(index, reports): vq_code of a residual bottleneck under the entropy constraint: int32 [N, stages, h * w
    * cout / D] and the per-image reports of ResidualS2HVQ.encode_ec.  The first half runs once."""
    vq = self._require_stages('vq_stage_code_ec')
    vq._stages(stages)                     # before any device work
    h, _ = run_chain_fwd(self._pre, x)
    return vq.code_ec(h, lam, n_iter, stages)

  def vq_stage_usage(self, x):
    """int64 [vq_stages, cout / D, n_center]: the histogram of every stage of vq_code(x) per channel group over the batch."""
    vq = self._require_stages('vq_stage_usage')
    h, _ = run_chain_fwd(self._pre, x)
    return vq.usage(h)

  def vq_features(self, x):
    """The [M, D] matrix the bottleneck's quantizer sees for x (M = N h w cout / D, vector m = pixel * (cout / D) + group): what
    vq_code assigns and what the code-book fit of DESIGN.md 4.21 runs on."""
    vq = self._require_vq()
    h, _ = run_chain_fwd(self._pre, x)
    return vq.features(h)

  def vq_usage(self, x):
    """fp32 [cout / D, n_center]: the histogram of vq_code(x) per channel group over the batch."""
    vq = self._require_vq()
    h, _ = run_chain_fwd(self._pre, x)
    return vq.usage(h)

  def vq_rate(self, x, denom):
    """fp32 [1]: the zero-order entropy of vq_code(x) per channel group over the batch, in bits / denom."""
    vq = self._require_vq()
    h, _ = run_chain_fwd(self._pre, x)
    return vq.rate(h, denom)

  def decode_vq_code(self, index, H, W):
    """The receiver's half: (features, status) from the int32 [N, h * w * cout / D] indices of an H x W image (ops.vq_decode,
    then model[4 + 3n + 1:]); status: the device word of ops.vq_decode, non-zero for an index outside the code book.  With
    vq_stages > 1 the indices are int32 [N, S', h * w * cout / D], any stage prefix 1 <= S' <= vq_stages (ops.vq_res_decode)."""
    vq, n = self._require_vq(), self.n_downsampling
    b, status = vq.decode(index, int(index.shape[0]), H >> n, W >> n, self.cdtype)
    y, _ = run_chain_fwd(self._post, b)
    return y, status

  def forward(self, input, inst=None, mode='get_continuous_img', inst_wise_pool=False):
    if mode == 'get_binary_code':
      self._require_binarizer()
      return ops.nhwc_to_nchw(self.code(_to_act(input, self.cdtype)))
    if mode != 'get_continuous_img':
      raise ValueError('Invalid encoding mode: {}'.format(mode))
    if inst_wise_pool:
      raise NotImplementedError('instance-wise pooling of the encoder output (--inst_wise_pool) is not implemented')
    y, _ = self.fwd(_to_act(input, self.cdtype))
    return ops.nhwc_to_nchw(y)


def define_G(input_nc, output_nc, ngf, netG, n_downsample_global=3, n_blocks_global=9, n_local_enhancers=1,
             n_blocks_local=3, norm='instance', gpu_ids=[], binarize_encoder=False,
             encoder_binarizer_out_channels=128, encoder_groups=1, binarize_generator=False,
             bin_generator_before_res=True, generator_binarizer_out_channels=128, compute_dtype='fp32',
             encoder_quantizer='binarizer', vq_n_center=64, vq_center_size=8, vq_sigma=10.0, vq_hard_forward=True, vq_stages=1):
  get_norm_layer(norm)
  device = torch.device('cuda', gpu_ids[0]) if len(gpu_ids) > 0 else None
  if device is not None:
    require_gpu(gpu_ids[0])
  if netG == 'global':
    net = GlobalGenerator(input_nc, output_nc, ngf, n_downsample_global, n_blocks_global,
                          binarize=binarize_generator, compute_dtype=compute_dtype, device=device)
  elif netG == 'local':
    net = LocalEnhancer(input_nc, output_nc, ngf, n_downsample_global, n_blocks_global, n_local_enhancers,
                        n_blocks_local, compute_dtype=compute_dtype, device=device)
  elif netG == 'encoder':
    net = Encoder(input_nc, output_nc, ngf, n_downsample_global, binarize=binarize_encoder,
                  binarizer_out_channels=encoder_binarizer_out_channels, groups=encoder_groups,
                  compute_dtype=compute_dtype, device=device, quantizer=encoder_quantizer, vq_n_center=vq_n_center,
                  vq_center_size=vq_center_size, vq_sigma=vq_sigma, vq_hard_forward=vq_hard_forward, vq_stages=vq_stages)
  else:
    raise ValueError('generator not implemented!')
  return net


# =============================================================================================
# discriminator
# =============================================================================================
class NLayerDiscriminator(nn.Module):
  """One PatchGAN scale with every intermediate feature returned (networks.py:422-471)."""

  def __init__(self, input_nc, ndf=64, n_layers=3, norm_layer=None, use_sigmoid=False, getIntermFeat=True,
               compute_dtype='fp32', device=None):
    super(NLayerDiscriminator, self).__init__()
    if use_sigmoid:
      raise NotImplementedError('--no_lsgan (sigmoid discriminator) is outside the JPD-SE hot path')
    self.n_layers = n_layers
    self.fuse_lrelu0 = True     # False: stage 0's LeakyReLU backward as its own pass (tests compare the two forms)
    self.cdtype = dtype_code(compute_dtype)
    kw = dict(dtype=self.cdtype, device=device)
    chans = [input_nc, ndf]
    nf = ndf
    for _ in range(1, n_layers):
      nf = min(nf * 2, 512)
      chans.append(nf)
    chans.append(min(nf * 2, 512))
    chans.append(1)
    self._stages = []
    for j in range(n_layers + 2):
      stride = 2 if j < n_layers else 1
      if j == 0:
        conv = HipConv2d(chans[0], chans[1], 4, stride, 2, PAD_ZERO, act=ACT_LRELU, slope=0.2, **kw)
        seq, stage = nn.Sequential(conv, _Slot()), conv
      elif j <= n_layers:
        conv = HipConv2d(chans[j], chans[j + 1], 4, stride, 2, PAD_ZERO, apply_bias=False, **kw)
        seq, stage = nn.Sequential(conv, _Slot(), _Slot()), ConvNormAct(conv, InstNormAct(ACT_LRELU, 0.2))
      else:
        conv = HipConv2d(chans[j], 1, 4, 1, 2, PAD_ZERO, **kw)
        seq, stage = nn.Sequential(conv), conv
      setattr(self, 'model' + str(j), seq)
      self._stages.append(stage)

  def fwd(self, x):
    feats, ctxs = [], []
    for st in self._stages:
      x, c = st.fwd(x)
      feats.append(x)
      ctxs.append(c)
    return feats, ctxs

  def bwd(self, ctxs, dfeats, need_dx=False, need_dw=True, dx_channels=None):
    """dfeats[j]: gradient w.r.t. feature j (Act) or None.  dx_channels=(c0, c1): return the input gradient of
    those channels only (needs need_dw False: the generator's pass through D)."""
    d = None
    fused = False           # dfeats[j] already summed into d by the data-gradient epilogue of stage j+1
    dz0 = False             # d is already the gradient w.r.t. stage 0's pre-activation
    for j in range(len(self._stages) - 1, -1, -1):
      if dfeats[j] is not None and not fused:
        d = dfeats[j] if d is None else ops.add_(d, dfeats[j])
      fused = False
      if d is None:
        continue
      # stage 1's input is stage 0's LeakyReLU(0.2) output: that activation's backward rides in the epilogue of
      # stage 1's data gradient (after the feature-matching addend), and stage 0 then starts from dz
      lrelu0 = dict(relu_input=True, input_slope=self._stages[0].slope) if (j == 1 and self.fuse_lrelu0) else {}
      if j == 0 and dx_channels is not None and need_dx and not need_dw:
        d = self._stages[0].bwd_input_slice(ctxs[0], d, dx_channels[0], dx_channels[1], dy_is_dz=dz0)
      elif j == 0:
        d = self._stages[0].bwd(ctxs[0], d, need_dx, need_dw, dy_is_dz=dz0)
      elif dfeats[j - 1] is not None:
        # the feature-matching gradient of feature j-1 joins in the epilogue of this stage's data gradient
        d = self._stages[j].bwd(ctxs[j], d, True, need_dw, addend=dfeats[j - 1], **lrelu0)
        fused = True
      else:
        d = self._stages[j].bwd(ctxs[j], d, True, need_dw, **lrelu0)
      dz0 = bool(lrelu0)
    return d


  def bwd_batched(self, ctxs, dfeats, dpred, B, later, dx_channels):
    """The backward walks of loss_G and loss_D as one: ctxs is the saved forward of [fake ; real] (2B images),
    dpred the gradient w.r.t. the last feature for 3B images [loss_G on fake ; loss_D on fake ; loss_D on real], dfeats[j]
    (j < last; B images or None) loss_G's feature-matching gradients.  Every stage's norm backward and data gradient run
    once over the 3B images; the weight gradients (loss_D's: images B..3B) are appended to `later` as calls for the owner to
    make.  Returns the gradient w.r.t. input channels dx_channels of the B fake images (loss_G's).  Needs fuse_lrelu0."""
    assert self.fuse_lrelu0
    d = dpred
    for j in range(len(self._stages) - 1, 0, -1):
      lrelu0 = dict(relu_input=True, input_slope=self._stages[0].slope) if j == 1 else {}
      d = self._stages[j].bwd_batched(ctxs[j], d, B, later, addend=dfeats[j - 1], **lrelu0)
    # stage 0 starts from dz: loss_D needs its weight gradient only, loss_G the gradient to the image channels only
    st0 = self._stages[0]
    if st0.weight.requires_grad:
      later.append(lambda: st0.bwd(ctxs[0], d.batch_slice(B, d.N), need_dx=False, need_dw=True, dy_is_dz=True))
    return st0.bwd_input_slice(ctxs[0].slice(0, B), d.batch_slice(0, B), dx_channels[0], dx_channels[1], dy_is_dz=True)


class MultiscaleDiscriminator(nn.Module):
  """networks.py:371-419 with getIntermFeat hard-wired True (pix2pixHD_model.py:162-163)."""

  def __init__(self, input_nc, ndf=64, n_layers=3, norm_layer=None, use_sigmoid=False, num_D=3,
               getIntermFeat=True, compute_dtype='fp32', device=None):
    super(MultiscaleDiscriminator, self).__init__()
    if not getIntermFeat:
      raise NotImplementedError('the JPD-SE model always requests intermediate features')
    self.num_D, self.n_layers, self.getIntermFeat = num_D, n_layers, True
    self.cdtype = dtype_code(compute_dtype)
    self._scales = []
    for i in range(num_D):
      netD = NLayerDiscriminator(input_nc, ndf, n_layers, norm_layer, use_sigmoid, True, compute_dtype, device)
      for j in range(n_layers + 2):
        setattr(self, 'scale' + str(i) + '_layer' + str(j), getattr(netD, 'model' + str(j)))
      self._scales.append(netD)     # plain list: parameters are registered through scale{i}_layer{j}

  def fwd(self, x):
    """Returns (result, ctx); result[i][j] is feature j of the i-times pooled input, computed by
    the sub-network stored as scale{num_D-1-i} (networks.py:408-418)."""
    result, ctxs, h = [], [], x
    for i in range(self.num_D):
      feats, c = self._scales[self.num_D - 1 - i].fwd(h)
      result.append(feats)
      ctxs.append((c, h.H, h.W))
      if i != self.num_D - 1:
        h = ops.avgpool3s2_fwd(h)
    return result, ctxs

  def bwd(self, ctxs, dresult, need_dx=False, need_dw=True, batch=None, dx_channels=None):
    """dresult[i][j]: Act or None.  `batch=(b0,b1)` back-propagates only that sub-batch of the
    saved forward (per-sample InstanceNorm makes sub-batches independent).  dx_channels=(c0, c1): the returned
    input gradient covers those input channels only (AvgPool between the scales acts per channel)."""
    dx = None
    for i in range(self.num_D - 1, -1, -1):
      c, H, W = ctxs[i]
      if batch is not None:
        c = [ci.slice(batch[0], batch[1]) for ci in c]
      d = self._scales[self.num_D - 1 - i].bwd(c, dresult[i], need_dx, need_dw, dx_channels)
      if need_dx:
        if dx is not None:          # gradient arriving from the coarser scale through AvgPool
          d = ops.add_(d, ops.avgpool3s2_bwd(dx, H, W))
        dx = d
    return dx

  def bwd_batched(self, ctxs, dfeats, dpred, B, dx_channels):
    """NLayerDiscriminator.bwd_batched for every scale.  dfeats[i][j] / dpred[i]: scale i's arguments.  Returns (the gradient
    w.r.t. input channels dx_channels of the B fake images, the weight-gradient calls still to be made, in walk order)."""
    dx, later = None, []
    for i in range(self.num_D - 1, -1, -1):
      c, H, W = ctxs[i]
      d = self._scales[self.num_D - 1 - i].bwd_batched(c, dfeats[i], dpred[i], B, later, dx_channels)
      if dx is not None:          # gradient arriving from the coarser scale through AvgPool
        d = ops.add_(d, ops.avgpool3s2_bwd(dx, H, W))
      dx = d
    return dx, later

  def can_bwd_batched(self):
    return all(s.fuse_lrelu0 for s in self._scales)

  def forward(self, input, keep_input=False):
    if keep_input:
      raise NotImplementedError('--match_raw_feat is outside the JPD-SE hot path')
    result, _ = self.fwd(_to_act(input, self.cdtype))
    return [[ops.nhwc_to_nchw(f) for f in scale] for scale in result]


def define_D(input_nc, ndf, n_layers_D, norm='instance', use_sigmoid=False, num_D=1, getIntermFeat=False,
             gpu_ids=[], compute_dtype='fp32'):
  get_norm_layer(norm)
  device = torch.device('cuda', gpu_ids[0]) if len(gpu_ids) > 0 else None
  if device is not None:
    require_gpu(gpu_ids[0])
  return MultiscaleDiscriminator(input_nc, ndf, n_layers_D, None, use_sigmoid, num_D, getIntermFeat,
                                 compute_dtype, device)


# =============================================================================================
# VGG19 feature pyramid + losses
# =============================================================================================
class Vgg19(nn.Module):
  """torchvision vgg19.features[0:30] cut after relu1_1, 2_1, 3_1, 4_1, 5_1 (networks.py:474-504).
  Frozen.  Weights: `load_torchvision_state_dict` (keys `features.<i>.weight/bias`) or, with no
  checkpoint available offline, the seeded He-normal initialisation the oracle also uses."""

  def __init__(self, requires_grad=False, compute_dtype='fp32', device=None, seed=20):
    super(Vgg19, self).__init__()
    self.cdtype = dtype_code(compute_dtype)
    convs, cin = [], 3
    g = torch.Generator().manual_seed(seed)
    for item in VGG_CFG:
      if item == 'M':
        continue
      conv = HipConv2d(cin, item, 3, 1, 1, PAD_ZERO, act=ACT_RELU, dtype=self.cdtype, device=device)
      std = (2.0 / (cin * 9)) ** 0.5
      with torch.no_grad():
        conv.weight.copy_(torch.randn(item, cin, 3, 3, generator=g) * std)
        conv.bias.copy_(torch.randn(item, generator=g) * 0.01)
      convs.append(conv)
      cin = item
    self.convs = nn.ModuleList(convs)
    for p in self.parameters():
      p.requires_grad = requires_grad

  def load_torchvision_state_dict(self, sd):
    idx, ci = 0, 0
    with torch.no_grad():
      for item in VGG_CFG:
        if item == 'M':
          idx += 1
          continue
        self.convs[ci].weight.copy_(sd['features.%d.weight' % idx])
        self.convs[ci].bias.copy_(sd['features.%d.bias' % idx])
        idx, ci = idx + 2, ci + 1

  def fwd(self, x, save=True):
    maps, ctxs, ci = [], [], 0
    pooled = None
    for pos, item in enumerate(VGG_CFG):
      if item == 'M':
        y = pooled if pooled is not None else ops.maxpool2_fwd(x)     # written by the conv in front of it (jpdse_conv_fwd_pool)
        pooled = None
        ctxs.append(Ctx(x) if save else None)
        x = y
        continue
      if pos + 1 < len(VGG_CFG) and VGG_CFG[pos + 1] == 'M' and x.H % 2 == 0 and x.W % 2 == 0:
        x, pooled, c = self.convs[ci].fwd_pool(x)
      else:
        x, c = self.convs[ci].fwd(x)
      ctxs.append(c if save else None)
      if ci in VGG_TAPS:
        maps.append(x)
      ci += 1
    return maps, ctxs

  def bwd(self, ctxs, dmaps):
    """Gradient w.r.t. the input image given the gradients of the five taps (dgrad only).
    Every ReLU backward is fused: `dmaps` must already be masked by their tap's ReLU
    (ops.l1_bwd(..., relu_a=True)), and each conv's data gradient is masked by its own input
    (a ReLU output or the max-pool of one) in the GEMM epilogue, so the gradient that reaches a
    conv is always w.r.t. its pre-activation."""
    order, ci = [], 0
    for item in VGG_CFG:
      order.append(('M', None) if item == 'M' else ('C', ci))
      if item != 'M':
        ci += 1
    d = None
    for pos in range(len(order) - 1, -1, -1):
      kind, ci = order[pos]
      if kind == 'C' and ci in VGG_TAPS and d is None:
        d = dmaps[VGG_TAPS.index(ci)]            # deepest tap: nothing to add to
      if d is None:
        continue
      if kind == 'M':
        (x,) = ctxs[pos].items
        d = ops.maxpool2_bwd(x, d)
      else:
        # the loss gradient of the tap that is this conv's INPUT (relu{k}_1 feeds conv{k}_2) is summed in the epilogue
        tap = dmaps[VGG_TAPS.index(ci - 1)] if (ci - 1) in VGG_TAPS and order[pos - 1][0] == 'C' else None
        d = self.convs[ci].bwd(ctxs[pos], d, True, False, dy_is_dz=True, relu_input=ci > 0, addend=tap)
    return d

  def forward(self, X):
    maps, _ = self.fwd(_to_act(X, self.cdtype), save=False)
    return [ops.nhwc_to_nchw(m) for m in maps]


class VGGLoss(nn.Module):
  """networks.py:124-139."""
  weights = [1.0 / 32, 1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0]

  def __init__(self, gpu_ids, compute_dtype='fp32'):
    super(VGGLoss, self).__init__()
    device = torch.device('cuda', gpu_ids[0]) if len(gpu_ids) else None
    self.vgg = Vgg19(compute_dtype=compute_dtype, device=device)

  def forward(self, x, y):
    dt = self.vgg.cdtype
    fx, _ = self.vgg.fwd(_to_act(x, dt), save=False)
    fy, _ = self.vgg.fwd(_to_act(y, dt), save=False)
    slots = torch.zeros(len(fx), dtype=torch.float32, device=fx[0].t.device)
    for i in range(len(fx)):
      ops.l1_fwd(fx[i], fy[i], slots[i:i + 1])
    vals = slots.cpu().tolist()
    return torch.tensor(sum(w * v for w, v in zip(self.weights, vals)), device=fx[0].t.device)


class GANLoss(nn.Module):
  """LSGAN objective on the last feature of every scale (networks.py:80-122)."""

  def __init__(self, use_lsgan=True, target_real_label=1.0, target_fake_label=0.0, tensor=None):
    super(GANLoss, self).__init__()
    if not use_lsgan:
      raise NotImplementedError('--no_lsgan is outside the JPD-SE hot path')
    self.real_label, self.fake_label = target_real_label, target_fake_label

  def __call__(self, input, target_is_real):
    t = self.real_label if target_is_real else self.fake_label
    preds = [s[-1] for s in input] if isinstance(input[0], list) else [input[-1]]
    dev = preds[0].t.device if isinstance(preds[0], Act) else preds[0].device
    slots = torch.zeros(len(preds), dtype=torch.float32, device=dev)
    for i, p in enumerate(preds):
      a = p if isinstance(p, Act) else ops.nchw_to_nhwc(p.float().contiguous(), F32)
      ops.mse_const_fwd(a, t, slots[i:i + 1])
    return torch.tensor(sum(slots.cpu().tolist()), device=dev)
