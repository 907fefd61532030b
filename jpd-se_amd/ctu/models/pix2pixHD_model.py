"""JPD-SE model on the MI355X-native kernels, behind the reference's `Pix2PixHDModel` API.

Reference: /root/reference/ctu/models/pix2pixHD_model.py
  __init__ :105-220   forward :231-245   create_optimizers :248-280   preprocess :362-412
  discriminate :451-460   _get_img :508-618   get_eval_loss :621-643   get_train_loss :709-771
  get_edges :774-783   save :786-792

What changed structurally (results identical; DESIGN.md "schedule"):
  * no autograd: `train_step` runs an explicit forward/backward program over libjpdse_hip.so;
  * the discriminator sees ONE batched pass [label|fake ; label|real] (InstanceNorm is per
    sample, so this equals the reference's separate passes) and the reference's third pass
    D(label|fake) -- numerically the same forward as D((label|fake).detach()) -- is not
    recomputed: its gradient w.r.t. the fake image is back-propagated through the saved fake
    half with weight gradients skipped (the reference computes and then discards them);
  * the one-hot / edge / concat input builder writes the 39-channel NHWC tensor directly.
Only the flag subset used by scripts/pix2pixHD_bpg_train.sh is accelerated; other branches
raise NotImplementedError.

Three modules: ctu.models.model_options owns the flags, their defaults and every refusal of a flag;
ctu.models.coded_calls (CodedCalls) the coded-stream and receiver calls; this one the networks, the input builders, the
inference calls and the training program.
"""
import contextlib
import os

import torch
import torch.distributed as dist

from jpdse_hip import F32, JpdseError, require_gpu
from jpdse_hip import ops
from jpdse_hip.ops import Act
from jpdse_hip.optim import FusedAdam
from jpdse_hip.layers import PackBatcher
from ctu.utils.image_pool import ImagePool
from ctu.models.codec import CODECS, VQDepthCodec, VQStagesCodec
from ctu.models.coded_calls import CodedCalls
from ctu.models.model_options import add_model_options, parse_class_distortion_weights, resolve_model_options, resolve_vq_class_stages  # noqa: F401
from ctu.models.pix2pixHD_networks.base_model import BaseModel
from ctu.models.pix2pixHD_networks import networks

LOSS_NAMES = ('G_GAN', 'G_GAN_Feat', 'G_VGG', 'G_Distortion', 'D_real', 'D_fake')
# forward(mode=...): the method a mode runs and its keyword arguments
FORWARD_MODES = {m: (m, {}) for m in ('get_img', 'get_train_loss', 'get_eval_loss', 'get_code', 'get_eval_rate',
                                      'get_eval_metrics', 'get_rate_map', 'get_class_rates')}
FORWARD_MODES['get_eval_metrics_per_class'] = ('get_eval_metrics', dict(per_class=True))


class Pix2PixHDModel(CodedCalls, BaseModel):

  modify_commandline_options = staticmethod(add_model_options)

  codec = None              # ctu.models.codec: set by __init__ when the encoder has a bottleneck
  no_instance = False       # --no_instance: set by __init__

  # ------------------------------------------------------------------------------------------
  def __init__(self, opt):
    super(Pix2PixHDModel, self).__init__(opt)
    o = resolve_model_options(opt)      # every refusal of a flag: before any network (hence any device allocation) exists
    self.use_features = True
    self.lambda_rate, self.lambda_vq_rate, self.vq_context_coder = o.lambda_rate, o.lambda_vq_rate, o.vq_context_coder
    self.lambda_vq_stage_rate = o.lambda_vq_stage_rate
    self.sem_weights, self.cdtype = o.sem_weights, networks.dtype_code(o.compute_dtype)
    self.n_onehot, self.label_nc, self.feat_nc, self.use_feat_encoding = o.n_onehot, o.label_nc, o.feat_nc, o.feat_enc
    self.zero_vis, self.zero_sem, self.zero_ins, self.no_instance = o.zero_vis, o.zero_sem, o.zero_ins, o.no_instance
    if self.use_gpu():
      require_gpu(opt.gpu_ids[0])
    self.netG = networks.define_G(self.label_nc + self.feat_nc, opt.num_out_channels, opt.ngf, opt.netG,
                                  opt.n_downsample_global, opt.n_blocks_global, opt.n_local_enhancers,
                                  opt.n_blocks_local, opt.norm, gpu_ids=self.gpu_ids, compute_dtype=o.compute_dtype)
    if o.checkpoint_resblocks:
      from jpdse_hip.layers import HipResnetBlock
      for m in self.netG.modules():
        if isinstance(m, HipResnetBlock):
          m.recompute = True
    if self.is_train:
      self.netD = networks.define_D(self.label_nc + opt.num_out_channels, opt.ndf, opt.n_layers_D, opt.norm, False, opt.num_D,
                                    True, gpu_ids=self.gpu_ids, compute_dtype=o.compute_dtype)
    # feature encoder of the learned codec, built after G and D as in the reference (model.py:167-175)
    self.netE = None
    if o.feat_enc:
      self.netE = networks.define_G(opt.input_nc, o.feat_nc, o.nef, 'encoder', o.n_downsample_E, norm=opt.norm,
                                    gpu_ids=self.gpu_ids, compute_dtype=o.compute_dtype, **o.encoder_args)
    # the codec of the encoder's bottleneck and the weight of its rate term, --lambda_rate, --lambda_vq_rate or
    # opt.lambda_vq_stage_rate:
    # resolve_model_options leaves a positive weight to the quantizer in use only
    self.rate_weight = 0.0
    if self.netE is not None and self.netE.quantizer is not None:
      # more than one stage of the vector quantizer (opt.vq_stages): the subclass that writes .jpdr files
      staged = self.netE.quantizer == 's2hvq' and o.vq_stages > 1
      # opt.vq_class_stages: the stage depth of a code cell follows its classes; None: today's model
      class_stages = resolve_vq_class_stages(opt)
      kind = VQDepthCodec if class_stages is not None else (VQStagesCodec if staged else CODECS[self.netE.quantizer])
      self.codec = kind(self.netE, self.cdtype)
      self.codec.class_stages = class_stages
      self.rate_weight = getattr(self, self.codec.RATE_OPTION)
      if self.vq_context_coder:
        self.codec.context_coder = True
    # binarizer noise: Philox key = the run's seed, counter = (element, image index in the global batch,
    # number of training forwards so far)
    self.codec_seed, self.codec_draw = o.codec_seed, 0
    self.vq_stages, self.vq_train_stages = o.vq_stages, o.vq_train_stages
    print('---------- networks initialized -------------')
    if not self.is_train or o.load_model:
      self.load_network(self.netG, 'G', opt)
      if self.is_train:
        self.load_network(self.netD, 'D', opt)
      if self.netE is not None:
        self.load_network(self.netE, 'E', opt)
    if self.is_train:
      if opt.pool_size > 0 and len(self.gpu_ids) > 1:
        raise NotImplementedError('Fake Pool Not Implemented for MultiGPU')
      self.fake_pool = ImagePool(opt.pool_size)
      self.criterionGAN = networks.GANLoss(use_lsgan=True)
      self.criterionVGG = networks.VGGLoss(self.gpu_ids, compute_dtype=o.compute_dtype)
      # The reference always optimises against ImageNet VGG19 features (networks.py:477).  A random-weight VGG is a
      # different objective, so it must be asked for by name; it is what tests and bench.py use (same FLOPs / bytes).
      if o.vgg19_state_dict:
        self.criterionVGG.vgg.load_torchvision_state_dict(torch.load(o.vgg19_state_dict, map_location='cpu'))
      elif not o.no_vgg_loss and not o.vgg_random_init:
        raise ValueError('the VGG loss needs ImageNet weights: pass --vgg19_state_dict <torchvision vgg19 state_dict> '
                         '(the reference downloads them, networks.py:477), or --vgg_random_init to accept a seeded '
                         'random-weight VGG19 (tests / benchmarks only), or --no_vgg_loss')
      self.loss_names = LOSS_NAMES
    else:
      self.loss_names = ('G_Distortion')      # a string, not a 1-tuple (no trailing comma): kept as it is
    self.grad_buckets = {}           # 'G' / 'D' -> jpdse_hip.ddp.GradBuckets (set by the trainer for DDP)
    self._one = None

  def use_gpu(self):
    return len(self.opt.gpu_ids) > 0

  def _device(self):
    if not self.use_gpu():
      raise JpdseError('the JPD-SE HIP path needs --gpu_ids >= 0: there is no CPU fallback')
    return torch.device('cuda', self.opt.gpu_ids[0])

  # ------------------------------------------------------------------------------------------
  def forward(self, x_dict, opt=None, mode='get_train_loss'):
    if mode not in FORWARD_MODES:
      raise ValueError('Invalid forward mode: {}'.format(mode))
    name, kw = FORWARD_MODES[mode]
    return getattr(self, name)(x_dict, **kw)

  def create_optimizers(self, opt):
    """Two Adams, lr/betas from opt (pix2pixHD_model.py:248-280); with niter_fix_global > 0 only
    the outermost enhancer (`model<n>_*`) is trained."""
    if opt.niter_fix_global > 0:
      prefix = 'model' + str(opt.n_local_enhancers)
      params = [p for k, p in self.netG.named_parameters() if k.startswith(prefix)]
      # the reference leaves requires_grad on and lets autograd compute gradients nobody applies; here the fixed
      # parameters are frozen, so their weight gradients -- and the whole backward of the coarse generator, which
      # only leads to frozen weights -- are not computed at all (LocalEnhancer.bwd)
      keep = {id(p) for p in params}
      for p in self.netG.parameters():
        p.requires_grad_(id(p) in keep)
      print('------------- only training the local enhancer network (for %d epochs) ------------'
            % opt.niter_fix_global)
    else:
      params = list(self.netG.parameters())
    e_modules = []
    if self.netE is not None:      # one Adam over G then E, the reference's order (model.py:269-270)
      params += list(self.netE.parameters())
      e_modules = list(self.netE.modules())
    for m in list(self.netG.modules()) + list(self.netD.modules()) + e_modules:
      if hasattr(m, 'ensure_grads'):
        m.ensure_grads()
    optimizer_G = FusedAdam(params, lr=opt.lr, betas=(opt.beta1, opt.beta2))
    optimizer_D = FusedAdam(list(self.netD.parameters()), lr=opt.lr, betas=(opt.beta1, opt.beta2))
    return optimizer_G, optimizer_D

  # ---- external codec hook (config 1 plumbing; CPU, third-party) -----------------------------
  @staticmethod
  def converter(filename, ext, quality):
    """Round-trip `filename` through an outside codec, return the path of the decoded image
    (pix2pixHD_model.py:287-321).  BPG shells out to bpgenc/bpgdec when they are installed."""
    from ctu.utils import codec
    return codec.converter(filename, ext, quality)

  def compress(self, x_dict, tmp_folder=None):
    """Decoded frame(s) of x_dict['image'] after the codec, normalised like the input (pix2pixHD_model.py:324-359).
    Synchronous fallback for batches that arrive without 'compressed_img'; unlike the reference it handles any batch
    size and never shares file names between processes (ctu.utils.codec).  The prefetched form is
    ctu.utils.codec.CodecCollate in the DataLoader."""
    from ctu.utils import codec
    return codec.compress_images(x_dict['image'], self.opt, tmp_folder)

  # ---- input builder ------------------------------------------------------------------------
  def preprocess(self, x_dict, build_base=True):
    """x_dict (CPU or cuda tensors from the loader) -> NHWC device activations.
    Returns dict(base=Act[B,H,W,label_nc+3] with one-hot+edge filled (model.py:375-394) -- None when build_base is False:
    the train step writes the network inputs directly (ops.input_builder) --, real=Act 3ch, src=Act 3ch (decoded frame
    when use_compressed else real), label / inst = the device label and instance maps)."""
    dev = self._device()
    opt = self.opt
    comp = None
    if opt.use_compressed:
      comp = x_dict.get('compressed_img')
      if comp is None:
        comp = self.compress(x_dict, os.path.join(opt.save_dir, 'tmp_imgs'))   # a private sub-directory per process
    label, inst = self._semantics(x_dict)
    inst_raw = None
    if self.sem_weights is not None and self.sem_weights[1] != 1.0:
      # the loss weights read the dataset's own instance map: --zero_ins blanks the networks' edge lane, not the weights
      inst_raw = inst if not self.zero_ins else x_dict['instance'].to(dev, dtype=torch.int64, non_blocking=True).contiguous()
    image = x_dict['image'].to(dev, dtype=torch.float32, non_blocking=True).contiguous()
    total_c = self.label_nc + self.feat_nc
    base = ops.onehot_edge(label, inst, self.n_onehot, total_c, self.cdtype) if build_base else None
    real = ops.nchw_to_nhwc(image, self.cdtype)
    src = real
    if comp is not None:
      src = ops.nchw_to_nhwc(comp.to(dev, dtype=torch.float32, non_blocking=True).contiguous(), self.cdtype)
    return dict(base=base, real=real, src=src, image_nchw=image, label=label, inst=inst, inst_raw=inst_raw, total_c=total_c)

  def _semantics(self, x_dict):
    """The device label and instance maps of x_dict, as the input builders read them."""
    dev = self._device()
    label = x_dict['label'].to(dev, dtype=torch.float32, non_blocking=True).contiguous()
    inst = x_dict['instance'].to(dev, dtype=torch.int64, non_blocking=True).contiguous()
    if self.no_instance:
      inst = torch.zeros_like(inst)      # a constant map has no edges; its channel is not part of label_nc
    elif self.zero_ins:
      # --zero_ins: the reference zeroes the edge channel of input_label IN PLACE (model.py:591) and hands that tensor on to
      # the discriminator (:610, :717-733), so G and D both see a zero edge lane: a constant instance map everywhere
      inst = torch.zeros_like(inst)
    return label, inst

  def _with_image(self, base, img, out=None):
    """torch.cat((input_label, img), dim=1) in NHWC: copy of `base` with the image channels filled."""
    dst = out if out is not None else base.empty_like()
    return ops.concat_channels(base, img, self.label_nc, dst)

  # ---- learned codec ---------------------------------------------------------------------------
  def _encoder_eval(self, fn):
    """Run fn() with netE in eval mode (deterministic sign binarizer), restoring its mode afterwards."""
    was = self.netE.training
    self.netE.train(False)
    try:
      return fn()
    finally:
      self.netE.train(was)

  def _g_input_zero_sem(self, vis, N, H, W):
    """--zero_sem (model.py:585-587): G's input [N, H, W] with all label_nc semantic lanes zero and `vis` (Act or None) in the
    visual lanes.  Only G's input: the discriminator keeps the real semantics (_get_img returns input_label untouched)."""
    g_in = Act.empty(N, H, W, self.label_nc + self.feat_nc, self.cdtype, self._device())
    ops.zero_(g_in.t)
    return g_in if vis is None else ops.insert_channels(g_in, vis, self.label_nc)

  def _g_input_eval(self, pre):
    """The generator input of the inference paths: [semantics | image], or [semantics | netE(image)] (model.py:568-595), with
    the --zero_vis / --zero_sem lanes blanked (:583-587; --zero_ins is already in the edge lane, see preprocess)."""
    vis = None if self.zero_vis else pre['src']      # --zero_vis: nothing visual reaches the generator
    if vis is not None and self.netE is not None:
      with self.codec.depth_term(pre['label']) if self.codec is not None else contextlib.nullcontext():
        vis, _ = self._encoder_eval(lambda: self.netE.fwd(vis))
    return self._g_input_from_vis(vis, pre['base'], pre['real'].N, pre['real'].H, pre['real'].W)

  def _g_input_from_vis(self, vis, base, N, H, W):
    """[semantics | vis] with the --zero_sem lanes blanked; vis None: the visual lanes stay zero.  `base` is preprocess's
    one-hot + edge tensor (unused, and may be None, under --zero_sem)."""
    if self.zero_sem:
      return self._g_input_zero_sem(vis, N, H, W)
    if vis is None:
      return base                        # onehot_edge leaves every lane behind the semantics zero
    return self._with_image(base, vis)

  def train_stage_count(self, step):
    """Stages the residual bottleneck uses in training forward `step`: all of them, or with vq_train_stages =
    'uniform' a draw from 1 .. vq_stages that is a pure host-side function of (seed, step) -- every rank draws the same."""
    if self.vq_train_stages != 'uniform':
      return self.vq_stages
    gen = torch.Generator().manual_seed(self.codec_seed * 1000003 + int(step))
    return 1 + int(torch.randint(self.vq_stages, (1,), generator=gen))

  def _set_codec_rng(self, local_batch):
    """Point the binarizer at this call's images: n_global = rank * local_batch + i.  A residual bottleneck gets this training
    forward's stage count instead (eval mode ignores it)."""
    if isinstance(self.codec, VQStagesCodec):
      self.netE._vq.train_stages = self.train_stage_count(self.codec_draw)
      return
    b = self.netE._binarizer
    if b is None:
      return
    # the rank within the group the gradients are reduced over (set by the trainer's enable_data_parallel)
    group = getattr(self, 'codec_process_group', None)
    rank = dist.get_rank(group) if dist.is_available() and dist.is_initialized() else 0
    b.seed, b.draw, b.n_global0 = self.codec_seed, self.codec_draw, rank * local_batch

  # ---- inference ------------------------------------------------------------------------------
  def _generate_eval(self, x_dict):
    """The eval-mode reconstruction of x_dict: (the generator's NHWC output, preprocess's dict)."""
    pre = self.preprocess(x_dict, build_base=not self.zero_sem)
    return self.netG.fwd(self._g_input_eval(pre))[0], pre

  def get_img(self, x_dict):
    with torch.no_grad():
      return ops.nhwc_to_nchw(self._generate_eval(x_dict)[0])

  def _require_ms_ssim_size(self, x_dict):
    """--distortion_loss_fn ms_ssim: five scales of an 11x11 window need a shorter side of 176; refused before any device work."""
    if self.opt.distortion_loss_fn != 'ms_ssim':
      return
    h, w = int(x_dict['label'].shape[-2]), int(x_dict['label'].shape[-1])
    if min(h, w) < ops.MSSSIM_MIN_SIDE:
      raise ValueError('distortion_loss_fn ms_ssim: the shorter image side must be at least %d (five MS-SSIM scales of an '
                       '11x11 window), got %d x %d' % (ops.MSSSIM_MIN_SIDE, h, w))

  def _distortion(self, fake, real, label, inst_raw, out, scale=None):
    """The training distortion of `fake` against `real` into the slot `out`: the one statement of which op runs.  With `scale`
    the op that has a one-pass gradient also produces scale * d out / d fake and that Act is returned; None otherwise (a
    value-only call, and the plain mse, whose gradient is backward_G's ops.mse_bwd)."""
    opt = self.opt
    if opt.distortion_loss_fn == 'ms_ssim':
      # its own final kernel writes the slot (no jpdse_loss_finalize term): valid where the other slots are
      if scale:
        return ops.msssim_loss_fwd_bwd(fake, real, opt.normalize_mean, opt.normalize_std, out, scale)
      ops.msssim_loss_fwd(fake, real, opt.normalize_mean, opt.normalize_std, out)
    elif self.sem_weights is not None:
      # value and, with `scale`, gradient from one pass; its own final kernel writes the slot
      table, edge_w = self.sem_weights
      return ops.sem_weighted_loss(fake, real, label, inst_raw, table, edge_w, opt.distortion_loss_fn, out, scale or None)
    elif opt.distortion_loss_fn == 'l1' and scale:
      return ops.l1_fwd_bwd(fake, real, out, scale)
    else:
      (ops.l1_fwd if opt.distortion_loss_fn == 'l1' else ops.mse_fwd)(fake, real, out)

  def get_weighted_distortion(self, x_dict):
    """The training distortion of the eval-mode reconstruction as a Python float: un-quantised (the normalised images, as
    G_Distortion), under the model's class and edge weights (the kernel of the train step, value only).  With
    trivial weights the plain l1 / mse mean.  get_eval_loss / get_eval_metrics stay the unweighted, quantised figures."""
    if self.opt.distortion_loss_fn == 'ms_ssim':
      raise ValueError('get_weighted_distortion covers the l1 and mse distortions, not --distortion_loss_fn ms_ssim')
    with torch.no_grad():
      fake, pre = self._generate_eval(x_dict)
      slot = torch.zeros(1, dtype=torch.float32, device=self._device())
      self._distortion(fake, pre['real'], pre['label'], pre['inst_raw'], slot)
      return float(slot.item())

  def get_eval_loss(self, x_dict):
    """Distortion on de-normalised, clipped, uint8-truncated images (0..255 scale), as the reference computes it on
    the host through tensor2im (pix2pixHD_model.py:636-641, utils/misc.py:64-95) -- here one device pass
    (jpdse_quant_loss: the same float64 arithmetic, bit-identical quantisation, no device->host image copies).
    Under --distortion_loss_fn ms_ssim (extension): 1 - ms_ssim of the same quantised images, from the jpdse_eval_metrics
    pass (get_eval_metrics' figure)."""
    self._require_ms_ssim_size(x_dict)
    if self.opt.distortion_loss_fn == 'ms_ssim':
      m = self.get_eval_metrics(x_dict)
      return torch.tensor(1.0 - m['ms_ssim'], dtype=torch.float32, device=self._device())
    with torch.no_grad():
      fake, pre = self._generate_eval(x_dict)
      real32 = ops.nchw_to_nhwc(pre['image_nchw'], F32)       # the original image un-rounded, as the reference uses it
      slot = torch.zeros(1, dtype=torch.float32, device=self._device())
      ops.quant_loss(fake, real32, self.opt.normalize_mean, self.opt.normalize_std,
                     self.opt.distortion_loss_fn == 'mse', slot)
      return slot[0]

  def get_eval_metrics(self, x_dict, per_class=False):
    """Every distortion figure of the reference's test loop (test.py:114-125) from ONE generator forward: dict(l1, mse,
    psnr, ms_ssim, per_image) on the 0..255 scale of the quantised images (ops.eval_metrics; MS-SSIM: DESIGN.md 4.5).
    l1 / mse are the numbers get_eval_loss returns for --distortion_loss_fn l1 / mse.  per_class=True adds `per_class`:
    L1, MSE and PSNR of each of the n_onehot semantic classes from the same device pass (the intent of the reference's
    get_sem_wise_distortion, model.py:646-706; ops.eval_metrics_per_class)."""
    with torch.no_grad():
      fake, pre = self._generate_eval(x_dict)
      return self._eval_metrics_of(fake, pre['image_nchw'], pre['label'], per_class)

  # ---- training -------------------------------------------------------------------------------
  def _forward_losses(self, x_dict, grad_w=None):
    """Forward pass of the whole loss graph.  Returns (state for backward, slots tensor, layout).
    grad_w = dict(feat=, vgg=, dist=) (train_step): the gradients of the L1 terms -- whose upstream
    gradient is just that constant weight -- are produced in the same pass as the loss values
    (jpdse_l1_fwd_bwd) and handed to backward_G through `state`."""
    opt = self.opt
    self._require_ms_ssim_size(x_dict)
    dev = self._device()
    skip = bool(getattr(opt, 'skip_unused_losses', False))
    run_d = not (skip and opt.no_g_gan_loss and opt.no_gan_feat_loss and opt.no_d_gan_loss)
    run_vgg = not (skip and opt.no_vgg_loss)

    # Input builder, one pass (ops.input_builder): the generator input [label | edge | decoded frame] and both halves of the
    # ONE batched discriminator pass [label | edge | fake ; label | edge | real] (model.py:375-394, 595, 456, 717-733) are
    # written straight from the label / instance maps; the fake half gets its image channels once G has produced them.
    pre = self.preprocess(x_dict, build_base=False)
    real, src, label, inst = pre['real'], pre['src'], pre['label'], pre['inst']
    B, H, W = real.N, real.H, real.W
    e_ctx = None
    rate_on = self.rate_weight > 0.0 and grad_w is not None      # a training step with a rate term
    if self.zero_vis:
      src = None
    # --zero_vis: without a source the visual lanes of G's input stay zero (input_builder zeroes them for a missing image) and the
    # encoder, whose output the reference replaces by zeros (model.py:583-584: no gradient reaches it), is not run.
    # --zero_sem: G's input is built apart with blank semantic lanes; D's halves keep the real semantics (model.py:585-587).
    if self.netE is not None or self.zero_sem:
      # learned codec: G sees [semantics | netE(image)] (model.py:568-595), netE in the trainer's mode (stochastic binarizer
      # when training); D sees [semantics | real / fake] as always
      vis = src
      if self.netE is not None and src is not None:
        self._set_codec_rng(B)
        # --lambda_rate / --lambda_vq_rate: a training step's forward also asks the bottleneck for its rate
        # term and the gradient, scaled like the distortion gradient: the weight, the kernel's mean over the local batch, and
        # the ranks' average in Adam's grad_scale
        with self.codec.rate_term(self.rate_weight, B, H, W) if rate_on else contextlib.nullcontext(), \
            self.codec.depth_term(label) if self.codec is not None else contextlib.nullcontext():
          vis, e_ctx = self.netE.fwd(src)
        if self.netE.training:
          self.codec_draw += 1
      if self.zero_sem:
        g_in = self._g_input_zero_sem(vis, B, H, W)
      else:
        g_in = Act.empty(B, H, W, self.label_nc + self.feat_nc, self.cdtype, dev)
        ops.input_builder(label, inst, self.n_onehot, [g_in], [vis], self.label_nc)
      d_in = Act.empty(2 * B, H, W, self.label_nc + real.C, self.cdtype, dev) if run_d else None
      if run_d:
        ops.input_builder(label, inst, self.n_onehot, [d_in.batch_slice(B, 2 * B), d_in.batch_slice(0, B)], [real, None],
                          self.label_nc)
    else:
      g_in = Act.empty(B, H, W, pre['total_c'], self.cdtype, dev)
      d_in = Act.empty(2 * B, H, W, pre['total_c'], self.cdtype, dev) if run_d else None
      if run_d:
        ops.input_builder(label, inst, self.n_onehot, [g_in, d_in.batch_slice(B, 2 * B), d_in.batch_slice(0, B)],
                          [src, real, None], self.label_nc)
      else:
        ops.input_builder(label, inst, self.n_onehot, [g_in], [src], self.label_nc)
    fake, g_ctx = self.netG.fwd(g_in)

    pred, d_ctx = None, None
    if run_d:
      ops.insert_channels(d_in.batch_slice(0, B), fake, self.label_nc)
      pred, d_ctx = self.netD.fwd(d_in)

    vf, vr, v_ctx = [], [], None
    n_vgg = len(networks.VGGLoss.weights)
    if run_vgg:
      # VGG19 on the generated and the real image as ONE pass over [fake ; real] (networks.py:124-139 runs vgg(x), vgg(y)):
      # the convolutions are per image, so the two halves of every feature map hold the values of the two separate passes (no
      # kernel on this path lets one image's arithmetic depend on the batch size: equal bit for bit on this build, which
      # tests/test_hip_networks.py::test_vgg19_batched_pass_equals_separate_passes checks -- a property of the kernels chosen,
      # not a contract of the ABI), the launch count halves and the deep, small layers (relu5_1: 32x64 pixels) fill the chip.
      # Backward goes through the fake half of the saved tensors only (Ctx.slice).  Memory: the real half's activations stay
      # alive until the pass ends instead of streaming through -- VGG19 to relu5_1 is ~0.33 GB of bf16 activations per
      # 1024x512 image, so +1.3 GB at batch 4; of no consequence next to 288 GB.
      vgg = self.criterionVGG.vgg
      both = Act.empty(2 * B, H, W, fake.C, self.cdtype, dev)
      ops.copy_(fake.t, both.t[:B])          # two 33 MB device-to-device copies
      ops.copy_(real.t, both.t[B:])
      maps, ctxs = vgg.fwd(both, save=not opt.no_vgg_loss)
      vf = [m.batch_slice(0, B) for m in maps]
      vr = [m.batch_slice(B, 2 * B) for m in maps]
      v_ctx = [c.slice(0, B) if c is not None else None for c in ctxs] if not opt.no_vgg_loss else None

    nD, nF = opt.num_D, opt.n_layers_D + 1
    layout = dict(D_fake=list(range(0, nD)), D_real=list(range(nD, 2 * nD)), G_GAN=list(range(2 * nD, 3 * nD)))
    o = 3 * nD
    layout['feat'] = [[o + i * nF + j for j in range(nF)] for i in range(nD)]
    o += nD * nF
    layout['vgg'] = list(range(o, o + n_vgg))
    o += n_vgg
    layout['dist'] = o
    rate_value = self.codec.rate_value if rate_on and e_ctx is not None else None
    if rate_value is not None:
      layout['rate'] = o + 1
    slots = torch.zeros(o + (1 if rate_value is None else 2), dtype=torch.float32, device=dev)
    if rate_value is not None:
      slots[o + 1:o + 2].copy_(rate_value)          # G_Rate, unscaled: read back with the six losses
    s = lambda i: slots[i:i + 1]
    gw = grad_w or {}
    d_feat, d_vgg, d_dist = None, None, None
    with ops.deferred_loss_finals():          # the second stage of all the loss terms below in ONE launch (jpdse_loss_finalize)
      for i in range(nD if run_d else 0):
        p = pred[i][-1]
        ops.mse_const_fwd(p.batch_slice(0, B), 0.0, s(layout['D_fake'][i]))
        ops.mse_const_fwd(p.batch_slice(B, 2 * B), 1.0, s(layout['D_real'][i]))
        ops.mse_const_fwd(p.batch_slice(0, B), 1.0, s(layout['G_GAN'][i]))
        for j in range(nF):
          f = pred[i][j]
          ff, fr = f.batch_slice(0, B), f.batch_slice(B, 2 * B)
          if gw.get('feat') and j < nF - 1:
            d_feat = d_feat if d_feat is not None else [[None] * nF for _ in range(nD)]
            d_feat[i][j] = ops.l1_fwd_bwd(ff, fr, s(layout['feat'][i][j]), gw['feat'] / nD)
          else:
            ops.l1_fwd(ff, fr, s(layout['feat'][i][j]))
      wk = networks.VGGLoss.weights
      for k in range(len(vf)):
        if gw.get('vgg') and v_ctx is not None:
          d_vgg = d_vgg if d_vgg is not None else [None] * len(vf)
          d_vgg[k] = ops.l1_fwd_bwd(vf[k], vr[k], s(layout['vgg'][k]), gw['vgg'] * wk[k], relu_a=True)
        else:
          ops.l1_fwd(vf[k], vr[k], s(layout['vgg'][k]))
      d_dist = self._distortion(fake, real, label, pre['inst_raw'], s(layout['dist']), gw.get('dist'))
    state = dict(B=B, fake=fake, real=real, g_ctx=g_ctx, e_ctx=e_ctx, pred=pred, d_ctx=d_ctx, vf=vf, vr=vr, v_ctx=v_ctx,
                 d_feat=d_feat, d_vgg=d_vgg, d_dist=d_dist, label=label, inst_raw=pre['inst_raw'])
    return state, slots, layout

  def _reduce_losses(self, vals, layout):
    """Host arithmetic on the slot values -> the reference's six loss scalars."""
    nD = self.opt.num_D
    w = networks.VGGLoss.weights
    L = dict(
        G_GAN=sum(vals[i] for i in layout['G_GAN']),
        G_GAN_Feat=sum((1.0 / nD) * vals[i] for row in layout['feat'] for i in row),
        G_VGG=sum(w[k] * vals[i] for k, i in enumerate(layout['vgg'])),
        G_Distortion=vals[layout['dist']],
        D_real=sum(vals[i] for i in layout['D_real']),
        D_fake=sum(vals[i] for i in layout['D_fake']))
    if 'rate' in layout:             # --lambda_rate: the unscaled rate term in bits per pixel, after the six losses
      L['G_Rate'] = vals[layout['rate']]
    return L

  def get_train_loss(self, x_dict):
    """The six losses as 0-dim device tensors in `loss_names` order (values only: the HIP path
    keeps no autograd graph -- use `train_step` to optimise)."""
    state, slots, layout = self._forward_losses(x_dict)
    L = self._reduce_losses(slots.cpu().tolist(), layout)
    return tuple(torch.tensor(L[k], device=slots.device) for k in LOSS_NAMES)

  def _ones(self, dev):
    if self._one is None or self._one.device != dev:
      self._one = torch.ones(1, dtype=torch.float32, device=dev)
    return self._one

  # One backward walk of D for loss_G and loss_D.  False: the two walks of before, loss_G's through the fake
  # half and loss_D's through the whole batch (A/B measurements, tests/test_hip_d_backward_batched.py).  Under data parallelism
  # (gradient buckets set) the two walks stay whatever this says: G's all-reduce hides behind the WHOLE D backward there, and the one
  # walk would move D's data gradients and norm backward in front of G's backward, out of that window.
  d_backward_batched = True

  def backward_G(self, state, w_gan, w_feat, w_vgg, w_dist, w_d=0.0):
    """d(loss_G)/d(netG params), loss_G = w_gan*G_GAN + w_feat*G_GAN_Feat + w_vgg*G_VGG + w_dist*G_Dist.  With w_d != 0 (train_step)
    and the batched walk on, D's data gradients of loss_D = w_d * (D_fake + D_real) ride in the same walk of D and the weight
    gradients of loss_D are left in state['d_wgrads'] for backward_D."""
    opt, B = self.opt, state['B']
    one = self._ones(state['fake'].t.device)
    fake, real = state['fake'], state['real']
    d_fake = None
    if (self.d_backward_batched and not self.grad_buckets and w_gan != 0.0 and w_d != 0.0 and state['pred'] is not None
        and self.netD.can_bwd_batched()
        and all(p.requires_grad for p in self.netD.parameters())):
      dfeats, dpred = [], []
      for i in range(opt.num_D):
        feats = state['pred'][i]
        row = []
        for j, f in enumerate(feats[:-1]):
          if w_feat == 0.0:
            row.append(None)
          elif state.get('d_feat') is not None and state['d_feat'][i][j] is not None:
            row.append(state['d_feat'][i][j])
          else:
            row.append(ops.l1_bwd(f.batch_slice(0, B), f.batch_slice(B, 2 * B), one, w_feat / opt.num_D))
        dfeats.append(row)
        # the three loss heads' gradients of this scale in one buffer: [loss_G on fake ; loss_D on fake ; loss_D on real]
        p = feats[-1]
        dp = Act.empty(3 * B, p.H, p.W, p.C, p.dtype, p.t.device)
        ops.mse_const_bwd(p.batch_slice(0, B), 1.0, one, w_gan, out=dp.batch_slice(0, B))
        ops.mse_const_bwd(p.batch_slice(0, B), 0.0, one, w_d, out=dp.batch_slice(B, 2 * B))
        ops.mse_const_bwd(p.batch_slice(B, 2 * B), 1.0, one, w_d, out=dp.batch_slice(2 * B, 3 * B))
        dpred.append(dp)
      d_fake, state['d_wgrads'] = self.netD.bwd_batched(state['d_ctx'], dfeats, dpred, B,
                                                        (self.label_nc, self.label_nc + fake.C))
    elif (w_gan != 0.0 or w_feat != 0.0) and state['pred'] is not None:
      dres = []
      for i in range(opt.num_D):
        row = []
        for j, f in enumerate(state['pred'][i]):
          ff, fr = f.batch_slice(0, B), f.batch_slice(B, 2 * B)
          if j == len(state['pred'][i]) - 1:
            row.append(ops.mse_const_bwd(ff, 1.0, one, w_gan) if w_gan != 0.0 else None)
          elif w_feat == 0.0:
            row.append(None)
          elif state.get('d_feat') is not None and state['d_feat'][i][j] is not None:
            row.append(state['d_feat'][i][j])           # produced with the loss value (l1_fwd_bwd)
          else:
            row.append(ops.l1_bwd(ff, fr, one, w_feat / opt.num_D))
        dres.append(row)
      # only the image channels of D's concatenated input carry a gradient back to G
      d_fake = self.netD.bwd(state['d_ctx'], dres, need_dx=True, need_dw=False, batch=(0, B),
                             dx_channels=(self.label_nc, self.label_nc + fake.C))
    if w_vgg != 0.0 and state['v_ctx'] is not None:
      wk = networks.VGGLoss.weights
      dmaps = state.get('d_vgg') or [ops.l1_bwd(state['vf'][k], state['vr'][k], one, w_vgg * wk[k], relu_a=True)
                                     for k in range(len(wk))]
      dv = self.criterionVGG.vgg.bwd(state['v_ctx'], dmaps)
      d_fake = dv if d_fake is None else ops.add_(d_fake, dv)
    if w_dist != 0.0:
      if state.get('d_dist') is not None:
        dd = state['d_dist']
      elif opt.distortion_loss_fn == 'ms_ssim' or self.sem_weights is not None:
        # the forward was a value-only call and these gradients need its sums (ms_ssim: the per-image means of all five scales):
        # the op runs again, the value goes to a scratch slot
        dd = self._distortion(fake, real, state['label'], state['inst_raw'],
                              torch.empty(1, dtype=torch.float32, device=fake.t.device), w_dist)
      else:
        fn = ops.l1_bwd if opt.distortion_loss_fn == 'l1' else ops.mse_bwd      # the gradient alone: no second forward
        dd = fn(fake, real, one, w_dist)
      d_fake = dd if d_fake is None else ops.add_(d_fake, dd)
    if d_fake is None:
      return False
    if state['e_ctx'] is None:           # no encoder, or --zero_vis cut it off G's input
      self.netG.bwd(state['g_ctx'], d_fake, need_dx=False, need_dw=True)
      return True
    # learned codec: the gradient w.r.t. the feature channels of G's input goes on into the encoder
    d_feat_map = self.netG.bwd(state['g_ctx'], d_fake, need_dx=True, need_dw=True,
                               dx_channels=(self.label_nc, self.label_nc + self.feat_nc))
    self.netE.bwd(state['e_ctx'], d_feat_map)
    return True

  def g_nets(self):
    """What optimizer G trains: netG, or netG and netE (one module for PackBatcher / gradient buckets; not registered)."""
    if self.netE is None:
      return self.netG
    if getattr(self, '_g_nets', None) is None:
      self.__dict__['_g_nets'] = torch.nn.ModuleList([self.netG, self.netE])
    return self._g_nets

  def _repack(self, which):
    """One-launch re-pack of the stepped network's data-gradient panels (jpdse_hip.layers.PackBatcher)."""
    if not hasattr(self, '_pack_batchers'):
      self._pack_batchers = {}
    b = self._pack_batchers.get(which)
    if b is None:
      b = self._pack_batchers[which] = PackBatcher(self.g_nets() if which == 'G' else self.netD)
    b.run()

  def backward_D(self, state, w_d):
    """d(loss_D)/d(netD params), loss_D = w_d * (D_fake + D_real)  (w_d = 0.5 in the trainer)."""
    if w_d == 0.0 or state['pred'] is None:
      return False
    if state.get('d_wgrads') is not None:
      # the batched walk of backward_G has run loss_D's data gradients: its weight gradients are what is left (one GPU only:
      # under data parallelism the two walks run)
      for call in state.pop('d_wgrads'):
        call()
      return True
    opt, B = self.opt, state['B']
    one = self._ones(state['fake'].t.device)
    dres = []
    for i in range(opt.num_D):
      p = state['pred'][i][-1]
      dp = p.empty_like()
      ops.mse_const_bwd(p.batch_slice(0, B), 0.0, one, w_d, out=dp.batch_slice(0, B))
      ops.mse_const_bwd(p.batch_slice(B, 2 * B), 1.0, one, w_d, out=dp.batch_slice(B, 2 * B))
      dres.append([None] * (len(state['pred'][i]) - 1) + [dp])
    self.netD.bwd(state['d_ctx'], dres, need_dx=False, need_dw=True)
    return True

  def train_step(self, x_dict, optimizer_G, optimizer_D, lambda_distortion_weight=1.0):
    """One optimisation step, results as the reference's (pix2pixHD_trainer.py:44-78: forward, loss_G backward + Adam(G),
    loss_D backward + Adam(D)) -- executed as forward, loss_G backward, loss_D backward, Adam(G), Adam(D): loss_D does not
    depend on G's weights, see below.  One host wait: for the loss copy queued after the forward pass."""
    opt = self.opt
    w_gan = 0.0 if opt.no_g_gan_loss else 1.0
    w_feat = 0.0 if opt.no_gan_feat_loss else opt.lambda_feat
    w_vgg = 0.0 if opt.no_vgg_loss else opt.lambda_feat
    w_dist = 0.0 if opt.no_distortion_loss else opt.lambda_distortion * lambda_distortion_weight
    state, slots, layout = self._forward_losses(x_dict, grad_w=dict(feat=w_feat, vgg=w_vgg, dist=w_dist))
    # All six losses are functions of the forward pass alone (the reference's .item() calls come after the optimizer
    # steps, pix2pixHD_trainer.py:80-85, but read values computed before them), so their device->host copy is queued HERE,
    # behind the loss kernels, and the host waits for THAT copy at the end of the step -- not for the backward passes and
    # Adam updates it has meanwhile enqueued.  step() still returns this step's losses; the host just no longer idles the
    # GPU for a launch round trip between two steps (0.3 ms per step in profiles/r02_step_breakdown.txt).
    early = getattr(self, 'early_loss_readback', True)      # False: copy after the optimizer steps (A/B measurements only)
    if early:
      loss_host, loss_ready = self._queue_loss_readback(slots)
    # Order: both backward passes first, then the two Adams.  The reference steps G before it back-propagates loss_D
    # (pix2pixHD_trainer.py:64-78), but loss_D's graph -- D on fake.detach() and on the real image -- does not contain G's
    # weights, so its gradients are the same numbers either way, bit for bit.  Under data parallelism this gives G's
    # gradient all-reduce (93 % of the bytes) the whole D backward to hide behind (launch_all below; which is why the one walk of D
    # for both losses, backward_G, is left to the single-GPU step: it would move most of that backward in front of launch_all), instead of the
    # ResnetBlock GEMMs whose grids are exactly one workgroup per CU and take a second round when RCCL holds any CU.
    bg, bd = self.grad_buckets.get('G'), self.grad_buckets.get('D')
    # Opt-in timeline of the data-parallel schedule (self.ddp_timeline = []: one dict of timing events per step, recorded on the
    # compute stream; bench.py --gpus N > 1 and tests/test_hip_ddp.py read it).  `g_reduced` is recorded right behind the waits
    # on G's all-reduce handles, so elapsed(d_bwd_end -> g_reduced) is what of the collective the D backward did NOT hide.
    tl = getattr(self, 'ddp_timeline', None)
    marks = {} if tl is not None else None

    def mark(name):
      if marks is not None:
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        marks[name] = ev

    w_d = 0.0 if opt.no_d_gan_loss else 0.5
    did_G = self.backward_G(state, w_gan, w_feat, w_vgg, w_dist, w_d)
    mark('g_bwd_end')
    if did_G and bg is not None:
      bg.launch_all()                  # no-op for buckets already started from the per-layer hooks (defer=False)
    # (Measured and not adopted, round 4: Adam(G) + the panel re-pack -- 1.2 ms of HBM-bound streaming -- on a second stream
    # beside the discriminator's backward: 26.36-26.40 ms per step against 26.15-26.33 serial, profiles/r04_adam_side_stream_ab.txt.
    # The D backward is itself half HBM-bound passes, and its GEMM launches lose more to the shared CUs than Adam gains.)
    did_D = self.backward_D(state, w_d)
    mark('d_bwd_end')
    if did_G:
      if bg is not None:
        bg.finish()
      mark('g_reduced')
      optimizer_G.step()
      self._repack('G')
      mark('adam_g_end')
    if did_D:
      if bd is not None:
        bd.finish()
      mark('d_reduced')
      optimizer_D.step()
      self._repack('D')
    mark('step_end')
    if tl is not None:
      marks['stats_G'] = dict(bg.stats) if bg is not None and bg.stats else None
      marks['stats_D'] = dict(bd.stats) if bd is not None and bd.stats else None
      tl.append(marks)
    if not early:
      loss_host, loss_ready = self._queue_loss_readback(slots)
    loss_ready.synchronize()
    return self._reduce_losses(loss_host.tolist(), layout)

  def _queue_loss_readback(self, slots):
    """Asynchronous copy of the loss slots into pinned host memory on the current stream; returns (host view, event)."""
    n = slots.numel()
    buf = getattr(self, '_loss_pinned', None)
    if buf is None or buf.numel() < n:
      buf = self._loss_pinned = torch.empty(max(n, 64), dtype=torch.float32).pin_memory()
    host = buf[:n]
    host.copy_(slots, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(slots.device))
    return host, ev

  # ------------------------------------------------------------------------------------------
  def save(self):
    self.save_network(self.netG, 'G', self.opt)
    self.save_network(self.netD, 'D', self.opt)
    if self.netE is not None:
      self.save_network(self.netE, 'E', self.opt)

  def update_fixed_params(self, optimizer_G):
    """After niter_fix_global epochs also fine-tune the coarse generator (model.py:795-804): a fresh Adam over ALL
    generator parameters (beta2 hard-wired to 0.999 as in the reference), carrying the old optimizer's gradient scale.
    Under data parallelism call Pix2PixHDTrainer.update_fixed_params, which also re-buckets the gradients."""
    for p in self.netG.parameters():
      p.requires_grad_(True)
    for m in self.netG.modules():
      if hasattr(m, 'ensure_grads'):
        m.ensure_grads()
    params = list(self.netG.parameters())
    if self.netE is not None:            # the encoder keeps training (model.py:797-799)
      params += list(self.netE.parameters())
    return FusedAdam(params, lr=self.opt.lr, betas=(self.opt.beta1, 0.999),
                     grad_scale=getattr(optimizer_G, 'grad_scale', 1.0))
