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
"""
import contextlib
import os

import torch
import torch.distributed as dist

from jpdse_hip import F32, BF16, JpdseError, require_gpu
from jpdse_hip import ops
from jpdse_hip.ops import Act
from jpdse_hip.optim import FusedAdam
from jpdse_hip.layers import PackBatcher
from ctu.utils import semantics as semantics_file
from ctu.utils.image_pool import ImagePool
from ctu.models.codec import CODECS, VQIndexCodec
from ctu.models.pix2pixHD_networks.base_model import BaseModel
from ctu.models.pix2pixHD_networks import networks

LOSS_NAMES = ('G_GAN', 'G_GAN_Feat', 'G_VGG', 'G_Distortion', 'D_real', 'D_fake')


def parse_class_distortion_weights(text, n_labels):
  """--class_distortion_weights: 'label:weight,label:weight,...' -> the table [cw[0], ..., cw[n_labels - 1]],
  1.0 for a label that is not named.  ValueError for malformed text, a label that is not an integer in [0, n_labels), a
  duplicate label, or a weight that is negative or not finite."""
  table = [1.0] * n_labels
  text = (text or '').strip()
  if not text:
    return table
  seen = set()
  for pair in text.split(','):
    parts = pair.split(':')
    if len(parts) != 2:
      raise ValueError('class_distortion_weights: %r is not a label:weight pair (expected e.g. "24:4,26:2")' % (pair,))
    try:
      label = int(parts[0].strip())
    except ValueError:
      raise ValueError('class_distortion_weights: the label %r is not an integer' % (parts[0],))
    try:
      weight = float(parts[1].strip())
    except ValueError:
      raise ValueError('class_distortion_weights: the weight %r of label %d is not a number' % (parts[1], label))
    if not 0 <= label < n_labels:
      raise ValueError('class_distortion_weights: label %d is outside [0, %d)' % (label, n_labels))
    if label in seen:
      raise ValueError('class_distortion_weights: label %d is named twice' % label)
    if not (weight >= 0.0 and weight != float('inf')):
      raise ValueError('class_distortion_weights: the weight of label %d must be a finite number >= 0, got %r' % (label, parts[1]))
    seen.add(label)
    table[label] = weight
  return table


class Pix2PixHDModel(BaseModel):

  @staticmethod
  def modify_commandline_options(parser, train):
    """Every flag of the reference setter (pix2pixHD_model.py:21-102) with the same name, type, default and choices
    (pinned by tests/golden/option_setter_flags.json, dumped from the reference), so that a reference command line or
    opt.pkl parses unchanged; flags of branches outside the accelerated path are accepted here and refused in
    __init__ when they would change the computation.  Extensions: --compute_dtype, --skip_unused_losses,
    --vgg19_state_dict, --vgg_random_init, --lambda_rate, --class_distortion_weights, --edge_distortion_weight,
    --encoder_quantizer, --vq_n_center, --vq_center_size, --vq_sigma, --vq_soft_forward, --lambda_vq_rate,
    --vq_context_coder."""
    a = parser.add_argument
    a('--num_D', type=int, default=2)
    a('--n_layers_D', type=int, default=3)
    a('--ndf', type=int, default=64)
    a('--no_lsgan', action='store_true')
    a('--pool_size', type=int, default=0)
    a('--no_instance', action='store_true')
    a('--no_label', action='store_true')
    a('--sem_masking', action='store_true')
    a('--norm', type=str, default='instance')
    a('--lambda_feat', type=float, default=10.0)
    a('--lambda_distortion', type=float, default=10.0)
    a('--anneal_lambda', action='store_true')
    a('--anneal_interval', type=int, default=5000)
    a('--anneal_factor', type=float, default=5.)
    a('--match_raw_feat', action='store_true')
    for f in ('gan_feat', 'vgg', 'distortion', 'g_gan', 'd_gan'):
      a('--no_%s_loss' % f, action='store_true')
    a('--data_type', default=32, type=int, choices=[8, 16, 32])
    a('--fp16', action='store_true', default=False)
    a('--skip_unused_losses', action='store_true',
      help='extension (SURVEY 8f-4): do not run D / VGG at all when every loss they feed is switched off by '
           '--no_*_loss (the reference runs them and discards the result, pix2pixHD_trainer.py:48-56); '
           'the skipped losses are reported as 0')
    a('--compute_dtype', type=str, default='fp32', choices=['fp32', 'bf16'],
      help='MFMA input type of the HIP kernels (fp32 accumulate either way)')
    a('--local_rank', type=int, default=0)
    a('--input_nc', type=int, default=3)
    a('--use_compressed', action='store_true')
    a('--ext', type=str, default='jpg', choices=['jpg', 'j2k', 'bpg', 'webp'])
    a('--quality', type=str, default='100')
    a('--zero_sem', action='store_true')
    a('--zero_ins', action='store_true')
    a('--zero_vis', action='store_true')
    a('--checkpoints_dir', type=str)
    a('--netG', type=str, default='global')
    a('--ngf', type=int, default=64)
    a('--n_downsample_global', type=int, default=4)
    a('--n_blocks_global', type=int, default=9)
    a('--n_blocks_local', type=int, default=3)
    a('--n_local_enhancers', type=int, default=1)
    a('--niter_fix_global', type=int, default=0)
    a('--no_feat_encoding', action='store_true')
    a('--no_feat', action='store_true')
    a('--no_label_encoding', action='store_true')
    a('--no_generator_binarization', action='store_true')
    a('--bin_generator_before_res', action='store_true')
    a('--generator_binarizer_out_channels', type=int, default=128)
    a('--use_netE_output', action='store_true')
    # learned-codec / masking branches: parsed for command-line compatibility only
    a('--binary_mask', action='store_true')
    a('--netE_groups', type=int, default=1)
    a('--inst_wise_pool', action='store_true')
    a('--use_dropout', action='store_true',
      help='declared by the reference but never read there (ResnetBlock is always built without dropout)')
    a('--feat_num', type=int, default=3)
    a('--n_downsample_E', type=int, default=4)
    a('--nef', type=int, default=64)
    a('--label_encoder_out_channels', type=int, default=36)
    a('--n_downsample_E4label', type=int, default=4)
    a('--ne4lf', type=int, default=64)
    a('--no_encoder_binarization', action='store_true')
    a('--encoder_binarizer_out_channels', type=int, default=128)
    a('--no_label_encoder_binarization', action='store_true')
    a('--label_encoder_binarizer_out_channels', type=int, default=128)
    a('--vgg19_state_dict', type=str, default=None,
      help='extension: local torchvision-format vgg19 state_dict (keys features.<i>.weight/bias) for the VGG loss; the '
           'reference downloads models.vgg19(pretrained=True) (networks.py:477), which needs network access')
    a('--checkpoint_resblocks', action='store_true',
      help='activation checkpointing of the ResnetBlocks (keep the block input, recompute in backward): the memory saver of '
           'BASELINE config 5; not needed on a 288 GB part, bit-identical results either way')
    a('--ddp_overlap', type=str, default='d_backward', choices=['d_backward', 'layers'],
      help='extension (data parallelism): where the generator gradient all-reduce runs -- behind the discriminator backward '
           '(default; keeps RCCL off the chip while the one-workgroup-per-CU ResnetBlock GEMMs run) or layer by layer from '
           'the backward hooks')
    a('--lambda_rate', type=float, default=0.0,
      help='extension (DESIGN.md 4.10): weight of the rate term in the generator / encoder loss -- the expected length of the '
           'code under a static form of the entropy coder\'s context model, in bits per pixel; needs the learned codec with '
           'encoder binarization; 0 (default): no rate term, the step is what it was')
    a('--class_distortion_weights', type=str, default='',
      help='extension (DESIGN.md 4.11): comma-separated label:weight pairs, e.g. "24:4,26:2": the l1 / mse training distortion '
           'of a pixel is multiplied by the weight of its class; a class that is not named has weight 1.  The loss is still '
           'divided by the element count, not by the sum of the weights, so all-ones weights are the reference loss: rescale '
           'with --lambda_distortion.  Default: no weights, the step is what it was')
    a('--edge_distortion_weight', type=float, default=1.0,
      help='extension (DESIGN.md 4.11): the distortion of a pixel on an instance edge (its instance id differs from a '
           '4-neighbour\'s; the dataset\'s own map, also under --zero_ins) is multiplied by this on top of its class weight; '
           'same normaliser as --class_distortion_weights (rescale with --lambda_distortion).  1 (default): no edge term')
    a('--encoder_quantizer', type=str, default='binarizer', choices=['binarizer', 's2hvq'],
      help='extension (DESIGN.md 4.15): the bottleneck of the feature encoder -- the reference\'s one-bit binarizer (default: '
           'every run is what it was) or the soft-to-hard vector quantizer over groups of --vq_center_size of the '
           '--encoder_binarizer_out_channels channels')
    a('--vq_n_center', type=int, default=64, help='--encoder_quantizer s2hvq: centres of the code book (2 .. 512)')
    a('--vq_center_size', type=int, default=8,
      help='--encoder_quantizer s2hvq: channels per vector (1 .. 32); must divide --encoder_binarizer_out_channels')
    a('--vq_sigma', type=float, default=10.0, help='--encoder_quantizer s2hvq: hardness of the soft assignment')
    a('--vq_soft_forward', action='store_true',
      help='--encoder_quantizer s2hvq: train on the soft assignment\'s mix of the centres instead of the nearest centre (the '
           'gradient is the soft form\'s either way); eval mode always takes the nearest centre')
    a('--lambda_vq_rate', type=float, default=0.0,
      help='extension (DESIGN.md 4.16): weight of the rate term of --encoder_quantizer s2hvq in the generator / encoder loss '
           '-- the entropy of the soft assignment\'s histogram per channel group (the model the .jpdv coder adapts to), in '
           'bits per pixel of the local batch; 0 (default): no rate term, the step is what it was')
    a('--vq_context_coder', action='store_true',
      help='extension (DESIGN.md 4.19): with --encoder_quantizer s2hvq, get_coded also codes each image\'s index planes with the '
           'spatial-context coder (.jpdw) and keeps whichever file is smaller, the .jpdv one on a tie; decode_coded reads '
           'either file with or without this flag.  Default: .jpdv files only, every run is what it was')
    a('--vgg_random_init', action='store_true',
      help='extension: explicitly accept a seeded random-weight VGG19 for the VGG loss (tests, benchmarks); without '
           'this flag training with the VGG loss and no --vgg19_state_dict is refused')
    return parser

  # ------------------------------------------------------------------------------------------
  def __init__(self, opt):
    super(Pix2PixHDModel, self).__init__(opt)
    g = lambda name, default=False: getattr(opt, name, default)
    unsupported = []
    # learned codec (feature encoder netE): accepted for the global generator
    feat_enc = not g('no_feat_encoding')
    if not g('no_label_encoding'):
      unsupported.append('the learned label encoder netE4label (run with --no_label_encoding)')
    if not g('no_generator_binarization'):
      unsupported.append('generator binarization (run with --no_generator_binarization)')
    if feat_enc:
      if g('netG', 'global') != 'global':
        unsupported.append('learned feature encoding with --netG %s (only the global generator back-propagates into its '
                           'input; run with --netG global or --no_feat_encoding)' % g('netG'))
      if g('netE_groups', 1) != 1:
        unsupported.append('--netE_groups %s' % g('netE_groups'))
      if g('n_downsample_E', 4) < 1:
        unsupported.append('--n_downsample_E %s (an encoder without downsampling)' % g('n_downsample_E'))
      if g('pool_size', 0) > 0:
        unsupported.append('--pool_size %s' % g('pool_size'))
    for flag in ('sem_masking', 'no_label', 'no_feat', 'match_raw_feat', 'no_lsgan', 'use_netE_output',
                 'binary_mask', 'inst_wise_pool'):
      if g(flag):
        unsupported.append('--' + flag)
    if g('norm', 'instance') != 'instance':
      unsupported.append('--norm ' + str(opt.norm))
    if unsupported:
      raise NotImplementedError('outside the accelerated JPD-SE path (SURVEY.md §2): ' + '; '.join(unsupported))
    if opt.distortion_loss_fn not in ('l1', 'mse', 'ms_ssim'):      # before any network (hence any device allocation) exists
      raise ValueError('distortion_loss_fn must be l1, mse or ms_ssim')
    self.lambda_rate = float(g('lambda_rate', 0.0) or 0.0)
    if not self.lambda_rate >= 0.0:
      raise ValueError('lambda_rate must be a non-negative number, got %r' % (g('lambda_rate'),))
    if self.lambda_rate > 0.0 and (not feat_enc or g('no_encoder_binarization') or g('zero_vis')):
      raise ValueError('lambda_rate > 0 needs the learned codec with encoder binarization (--no_feat_encoding and '
                       '--no_encoder_binarization must both be off) and an encoder that runs (no --zero_vis)')
    # rate term of the vector-quantizer bottleneck
    lvr = g('lambda_vq_rate', 0.0)
    self.lambda_vq_rate = float(0.0 if lvr is None or lvr is False else lvr)
    if not (self.lambda_vq_rate >= 0.0 and self.lambda_vq_rate != float('inf')):
      raise ValueError('lambda_vq_rate must be a finite non-negative number, got %r' % (lvr,))
    if self.lambda_vq_rate > 0.0 and (g('encoder_quantizer', 'binarizer') != 's2hvq' or g('zero_vis')):
      raise ValueError('lambda_vq_rate > 0 is the rate term of the vector-quantizer bottleneck: it needs --encoder_quantizer '
                       's2hvq and an encoder that runs (no --zero_vis)')
    # context coder of the vector-quantizer bottleneck's files
    self.vq_context_coder = bool(g('vq_context_coder'))
    if self.vq_context_coder and g('encoder_quantizer', 'binarizer') != 's2hvq':
      raise ValueError('--vq_context_coder codes the index planes of the vector-quantizer bottleneck: it needs '
                       '--encoder_quantizer s2hvq')
    # vector-quantizer bottleneck: refused combinations before any network (hence any device allocation) exists
    if g('encoder_quantizer', 'binarizer') not in ('binarizer', 's2hvq'):
      raise ValueError('encoder_quantizer must be binarizer or s2hvq, got %r' % (g('encoder_quantizer'),))
    if g('encoder_quantizer', 'binarizer') == 's2hvq':
      if not feat_enc or g('no_encoder_binarization'):
        raise ValueError('--encoder_quantizer s2hvq needs the learned codec with its bottleneck (--no_feat_encoding and '
                         '--no_encoder_binarization must both be off)')
      if self.lambda_rate > 0.0:
        raise ValueError('--lambda_rate > 0 is the binarizer\'s context-model rate term: it cannot be combined with '
                         '--encoder_quantizer s2hvq')
      from jpdse_hip.layers import vq_bottleneck_check
      vq_bottleneck_check(int(g('encoder_binarizer_out_channels', 128)), int(g('vq_n_center', 64)),
                          int(g('vq_center_size', 8)), g('vq_sigma', 10.0), '--encoder_quantizer s2hvq')
    # semantics-weighted distortion: (class table, edge weight), or None when every weight is 1 -- the
    # step then takes the plain l1 / mse path
    n_onehot = opt.num_labels + 1 if g('contain_dontcare_label') else opt.num_labels
    table = parse_class_distortion_weights(g('class_distortion_weights', ''), min(n_onehot, ops.SEM_TABLE))
    edge_w = g('edge_distortion_weight', 1.0)
    edge_w = 1.0 if edge_w is None else float(edge_w)
    if not (edge_w >= 0.0 and edge_w != float('inf')):
      raise ValueError('edge_distortion_weight must be a finite number >= 0, got %r' % (g('edge_distortion_weight'),))
    if edge_w != 1.0 and g('no_instance'):
      raise ValueError('edge_distortion_weight != 1 needs the instance map: it cannot be combined with --no_instance')
    self.sem_weights = None
    if edge_w != 1.0 or any(w != 1.0 for w in table):
      if opt.distortion_loss_fn == 'ms_ssim':
        raise ValueError('class_distortion_weights / edge_distortion_weight weight the l1 and mse distortions only: they '
                         'cannot be combined with --distortion_loss_fn ms_ssim')
      self.sem_weights = (table, edge_w)
    self.opt = opt
    self.is_train = opt.is_train
    self.use_features = True
    cd = 'bf16' if (g('compute_dtype', 'fp32') == 'bf16' or g('fp16')) else 'fp32'
    self.cdtype = networks.dtype_code(cd)
    if self.use_gpu():
      require_gpu(opt.gpu_ids[0])

    # channel bookkeeping (pix2pixHD_model.py:117-158)
    self.n_onehot = opt.num_labels + 1 if g('contain_dontcare_label') else opt.num_labels
    self.label_nc = self.n_onehot + (0 if g('no_instance') else 1)
    self.use_feat_encoding = feat_enc
    # ablation inputs (model.py:583-606): blank the visual lanes, every semantic lane, or the instance-edge lane of G's input
    self.zero_vis, self.zero_sem = bool(g('zero_vis')), bool(g('zero_sem'))
    # the edge lane is only consulted when the semantics stay and an edge lane exists (model.py:588)
    self.zero_ins = bool(g('zero_ins')) and not self.zero_sem and not g('no_instance')
    # generator input: semantics + encoded image (feat_num channels) or + the image itself (model.py:135-139)
    self.feat_nc = g('feat_num', 3) if feat_enc else opt.input_nc
    netG_input_nc = self.label_nc + self.feat_nc
    netD_input_nc = self.label_nc + opt.num_out_channels

    self.netG = networks.define_G(netG_input_nc, opt.num_out_channels, opt.ngf, opt.netG,
                                  opt.n_downsample_global, opt.n_blocks_global, opt.n_local_enhancers,
                                  opt.n_blocks_local, opt.norm, gpu_ids=self.gpu_ids, compute_dtype=cd)
    if g('checkpoint_resblocks', False):
      from jpdse_hip.layers import HipResnetBlock
      for m in self.netG.modules():
        if isinstance(m, HipResnetBlock):
          m.recompute = True
    if self.is_train:
      self.netD = networks.define_D(netD_input_nc, opt.ndf, opt.n_layers_D, opt.norm, False, opt.num_D, True,
                                    gpu_ids=self.gpu_ids, compute_dtype=cd)
    # feature encoder of the learned codec, built after G and D as in the reference (model.py:167-175)
    self.netE = None
    if feat_enc:
      self.netE = networks.define_G(opt.input_nc, g('feat_num', 3), g('nef', 64), 'encoder', g('n_downsample_E', 4),
                                    norm=opt.norm, gpu_ids=self.gpu_ids,
                                    binarize_encoder=not g('no_encoder_binarization'),
                                    encoder_binarizer_out_channels=g('encoder_binarizer_out_channels', 128),
                                    encoder_groups=g('netE_groups', 1), compute_dtype=cd,
                                    encoder_quantizer=g('encoder_quantizer', 'binarizer'), vq_n_center=g('vq_n_center', 64),
                                    vq_center_size=g('vq_center_size', 8), vq_sigma=g('vq_sigma', 10.0),
                                    vq_hard_forward=not g('vq_soft_forward'))
    # the codec of the encoder's bottleneck and the weight of its rate term, --lambda_rate or --lambda_vq_rate:
    # the checks above leave a positive weight to the quantizer in use only
    self.rate_weight = 0.0
    if self.netE is not None and self.netE.quantizer is not None:
      self.codec = CODECS[self.netE.quantizer](self.netE, self.cdtype)
      self.rate_weight = getattr(self, self.codec.RATE_OPTION)
      if self.vq_context_coder:
        self.codec.context_coder = True
    # binarizer noise: Philox key = the run's seed, counter = (element, image index in the global batch,
    # number of training forwards so far)
    self.codec_seed = int(g('seed', None) or 0)
    self.codec_draw = 0
    print('---------- networks initialized -------------')
    if not self.is_train or g('load_model'):
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
      self.criterionVGG = networks.VGGLoss(self.gpu_ids, compute_dtype=cd)
      # The reference always optimises against ImageNet VGG19 features (networks.py:477).  A random-weight VGG is a
      # different objective, so it must be asked for by name; it is what tests and bench.py use (same FLOPs / bytes).
      vgg_path = g('vgg19_state_dict', None)
      vgg_needed = not (g('no_vgg_loss') and g('skip_unused_losses'))
      if vgg_path:
        self.criterionVGG.vgg.load_torchvision_state_dict(torch.load(vgg_path, map_location='cpu'))
      elif vgg_needed and not g('no_vgg_loss') and not g('vgg_random_init'):
        raise ValueError('the VGG loss needs ImageNet weights: pass --vgg19_state_dict <torchvision vgg19 state_dict> '
                         '(the reference downloads them, networks.py:477), or --vgg_random_init to accept a seeded '
                         'random-weight VGG19 (tests / benchmarks only), or --no_vgg_loss')
      self.loss_names = LOSS_NAMES
    else:
      self.loss_names = ('G_Distortion')
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
    if mode == 'get_img':
      return self.get_img(x_dict)
    if mode == 'get_train_loss':
      return self.get_train_loss(x_dict)
    if mode == 'get_eval_loss':
      return self.get_eval_loss(x_dict)
    if mode == 'get_code':
      return self.get_code(x_dict)
    if mode == 'get_eval_rate':
      return self.get_eval_rate(x_dict)
    if mode == 'get_eval_metrics':
      return self.get_eval_metrics(x_dict)
    if mode == 'get_eval_metrics_per_class':
      return self.get_eval_metrics(x_dict, per_class=True)
    if mode == 'get_rate_map':
      return self.get_rate_map(x_dict)
    if mode == 'get_class_rates':
      return self.get_class_rates(x_dict)
    raise ValueError('Invalid forward mode: {}'.format(mode))

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
    if getattr(self.opt, 'no_instance', False):
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

  def _set_codec_rng(self, local_batch):
    """Point the binarizer at this call's images: n_global = rank * local_batch + i."""
    b = self.netE._binarizer
    if b is None:
      return
    # the rank within the group the gradients are reduced over (set by the trainer's enable_data_parallel)
    group = getattr(self, 'codec_process_group', None)
    rank = dist.get_rank(group) if dist.is_available() and dist.is_initialized() else 0
    b.seed, b.draw, b.n_global0 = self.codec_seed, self.codec_draw, rank * local_batch

  codec = None      # ctu.models.codec: set by __init__ when the encoder has a bottleneck

  def _binary_codec(self, who='binary codes'):
    """The binarizer's codec, or the refusal.  The calls that serve either form take `self.codec or self._binary_codec()`:
    without a bottleneck they refuse as the binary calls do."""
    if isinstance(self.codec, VQIndexCodec):
      raise ValueError('%s: a call of the one-bit binarizer\'s code, not available with --encoder_quantizer s2hvq (its code: '
                       'get_vq_code / get_coded / get_coded_rate)' % who)
    if self.codec is None:
      raise ValueError('binary codes need the learned codec with encoder binarization '
                       '(--no_feat_encoding and --no_encoder_binarization must both be off)')
    return self.codec

  def _vq_codec(self, who):
    """The vector quantizer's codec, or the refusal."""
    if not isinstance(self.codec, VQIndexCodec):
      raise ValueError('%s: the vector-quantised code needs --encoder_quantizer s2hvq' % who)
    return self.codec

  def _eval_code(self, codec, x_dict):
    """The encoder's eval-mode code of x_dict (the decoded frame with --use_compressed) in the codec's form."""
    pre = self.preprocess(x_dict, build_base=False)
    return self._encoder_eval(lambda: codec.code(pre['src']))

  def _code_act(self, x_dict, who='binary codes'):
    """The encoder's eval-mode bitstream of x_dict as an NHWC Act."""
    return self._eval_code(self._binary_codec(who), x_dict)

  def get_code(self, x_dict, packed=False):
    """[image_code] (model.py:494-505, 557-563): (b + 1) / 2 as fp32 [N, bits] in NCHW flatten order -- or, packed=True
    (extension), the bitstream itself, uint8 [N, ceil(bits / 8)] MSB first."""
    with torch.no_grad():
      return [ops.code_export(self._code_act(x_dict, 'get_code'), packed)]

  def get_context_rate(self, x_dict):
    """The hard-mode rate term of the eval-mode code, batch mean in bits per pixel, a Python float: the code's
    conditional entropy under the static, Laplace-smoothed form of the 4.8 coder's context model, counted on the code itself.
    An estimate that stays below the coded size (no flush, no adaptation cost) -- not a size; get_coded_rate measures files."""
    with torch.no_grad():
      b = self._code_act(x_dict, 'get_context_rate')
      pixels = int(x_dict['image'].shape[-2]) * int(x_dict['image'].shape[-1])
      value, _, _, _ = ops.code_rate_loss(b, None, pixels, want_grad=False)
      return float(value.item())

  def get_eval_rate(self, x_dict):
    """(Shannon bpp, raw bpp) averaged over the batch, with the reference's formula and types (model.py:468-491): per image
    p = mean((b + 1) / 2), entropy -p ln p - (1 - p) ln(1 - p) -- in NATS, as the reference computes it (torch.log) --
    times bits / pixels; nan when p is 0 or 1.  First value a 0-dim float tensor, second a Python float.  p comes from the
    integer per-image counts of jpdse_code_stats (exact: torch.mean's fp32 sum of halves is exact below 2^24 bits)."""
    with torch.no_grad():
      b = self._code_act(x_dict, 'get_eval_rate')
      counts = ops.code_stats(b).to(torch.float64)
      bits = b.C * b.H * b.W
      pixels = int(x_dict['image'].shape[-2]) * int(x_dict['image'].shape[-1])
      p_all = ((2.0 * counts[:, 0] + counts[:, 1]) / (2.0 * bits)).to(torch.float32)
      shannon, actual = 0., 0.
      for j in range(b.N):
        p = p_all[j]
        ent = - p * torch.log(p) - (1 - p) * torch.log(1 - p)
        shannon += ent * bits / pixels
        actual += bits / pixels
      return shannon / b.N, actual / b.N

  # ---- inference ------------------------------------------------------------------------------
  def get_img(self, x_dict):
    with torch.no_grad():
      pre = self.preprocess(x_dict, build_base=not self.zero_sem)
      fake, _ = self.netG.fwd(self._g_input_eval(pre))
      return ops.nhwc_to_nchw(fake)

  def _require_ms_ssim_size(self, x_dict):
    """--distortion_loss_fn ms_ssim: five scales of an 11x11 window need a shorter side of 176; refused before any device work."""
    if self.opt.distortion_loss_fn != 'ms_ssim':
      return
    h, w = int(x_dict['label'].shape[-2]), int(x_dict['label'].shape[-1])
    if min(h, w) < ops.MSSSIM_MIN_SIDE:
      raise ValueError('distortion_loss_fn ms_ssim: the shorter image side must be at least %d (five MS-SSIM scales of an '
                       '11x11 window), got %d x %d' % (ops.MSSSIM_MIN_SIDE, h, w))

  def _sem_weighted(self, fake, real, label, inst_raw, out, scale=None):
    """The weighted l1 / mse distortion of DESIGN.md 4.11 under the model's weights into `out`; the gradient Act when `scale`
    is given."""
    table, edge_w = self.sem_weights
    return ops.sem_weighted_loss(fake, real, label, inst_raw, table, edge_w, self.opt.distortion_loss_fn, out, scale)

  def get_weighted_distortion(self, x_dict):
    """The training distortion of the eval-mode reconstruction as a Python float: un-quantised (the normalised images, as
    G_Distortion), under the model's class and edge weights (the kernel of the train step, value only).  With
    trivial weights the plain l1 / mse mean.  get_eval_loss / get_eval_metrics stay the unweighted, quantised figures."""
    if self.opt.distortion_loss_fn == 'ms_ssim':
      raise ValueError('get_weighted_distortion covers the l1 and mse distortions, not --distortion_loss_fn ms_ssim')
    with torch.no_grad():
      pre = self.preprocess(x_dict, build_base=not self.zero_sem)
      fake, _ = self.netG.fwd(self._g_input_eval(pre))
      slot = torch.zeros(1, dtype=torch.float32, device=self._device())
      if self.sem_weights is not None:
        self._sem_weighted(fake, pre['real'], pre['label'], pre['inst_raw'], slot)
      else:
        (ops.l1_fwd if self.opt.distortion_loss_fn == 'l1' else ops.mse_fwd)(fake, pre['real'], slot)
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
      pre = self.preprocess(x_dict, build_base=not self.zero_sem)
      fake, _ = self.netG.fwd(self._g_input_eval(pre))
      real32 = ops.nchw_to_nhwc(pre['image_nchw'], F32)       # the original image un-rounded, as the reference uses it
      slot = torch.zeros(1, dtype=torch.float32, device=self._device())
      ops.quant_loss(fake, real32, self.opt.normalize_mean, self.opt.normalize_std,
                     self.opt.distortion_loss_fn == 'mse', slot)
      return slot[0]

  # ---- the vector-quantised code (extension) ------------------------------------------------------------------
  def get_vq_code(self, x_dict):
    """The eval-mode code of the vector-quantizer bottleneck: int64 [N, h * w * C / D] on the device, per image the index of
    the nearest centre of every group of D channels, pixel by pixel, groups ascending inside a pixel."""
    codec = self._vq_codec('get_vq_code')
    with torch.no_grad():
      return self._eval_code(codec, x_dict)

  def get_vq_rate(self, x_dict):
    """The hard-mode rate term of the eval-mode code in bits per pixel of the batch, a Python float: the
    zero-order entropy of get_vq_code(x_dict) per channel group, histograms taken over the batch.  An estimate, not a size:
    get_coded_rate measures the .jpdv files, whose adaptive coder may land on either side of it."""
    self._vq_codec('get_vq_rate')
    with torch.no_grad():
      pre = self.preprocess(x_dict, build_base=False)
      src = pre['src']
      value = self._encoder_eval(lambda: self.netE.vq_rate(src, src.N * src.H * src.W))
      return float(value.item())

  def _decode_act(self, code, x_dict):
    """decode() up to the generator's NHWC output; also returns the device label map."""
    codec = self.codec or self._binary_codec()
    geo = codec.check_code(code, x_dict, 'decode')
    return self._generate_from_code(codec.features_of_code(code, geo, self._device, 'decode'), x_dict, *geo[:3])

  def _generate_from_code(self, features, x_dict, N, H, W):
    """The receiver's device work, shared by decode and decode_coded: features() gives the encoder's output from the code."""
    label, inst = self._semantics(x_dict)
    vis = None if self.zero_vis else features()      # --zero_vis: nothing visual reaches the generator, the code is not read
    base = None if self.zero_sem else ops.onehot_edge(label, inst, self.n_onehot, self.label_nc + self.feat_nc, self.cdtype)
    fake, _ = self.netG.fwd(self._g_input_from_vis(vis, base, N, H, W))
    return fake, label

  def decode(self, code, x_dict):
    """The receiver (extension; the reference never decodes a stored code): the reconstructed image, NCHW as get_img returns
    it, from `code` -- what get_code returned, float32 [N, bits] or (packed) uint8 [N, ceil(bits / 8)], on the CPU or the
    device -- and the semantics x_dict['label'], x_dict['instance'].  Neither 'image' nor 'compressed_img' is read.  The
    code goes through ops.code_import and the encoder's second half (Encoder.decode_code); the generator input is then
    built as get_img builds it from the features, --zero_sem / --zero_ins / --zero_vis included (--zero_vis ignores the code
    as get_img ignores the image).
    Zero rule: decode(get_code(x)) equals get_img(x) bit for bit when the eval code has no exact zero (ops.code_stats column
    1).  Where the encoder's tanh is exactly 0, get_img feeds sign(0) = 0 forward but the stored bit is 0, so the decoder
    sees -1 there: the stored code, not the tensor get_img used, is what a receiver reconstructs from.
    ValueError without an encoder or a binarizer, and for a code whose size does not fit the label map (before any device
    work).
    With --encoder_quantizer s2hvq the code is what get_vq_code returned, int64 [N, indices]: decode(get_vq_code(x), x)
    equals get_img(x) bit for bit, with no zero rule -- both sides see code_book[index]."""
    with torch.no_grad():
      fake, _ = self._decode_act(code, x_dict)
      return ops.nhwc_to_nchw(fake)

  # ---- entropy-coded bitstream (extension) ------------------------------------------------------------------
  def get_coded(self, x_dict):
    """The entropy-coded form of get_code(x_dict, packed=True): a list of N `bytes`, per image the C stream lengths and the C
    range-coded streams (ops.code_entropy_encode).  Lossless: decode_coded(get_coded(x), x) equals
    decode(get_code(x, packed=True), x) bit for bit.
    With --encoder_quantizer s2hvq: a list of N .jpdv blobs (ctu.utils.vqstream), one per image, of that image's
    get_vq_code row; with --vq_context_coder an item is the image's .jpdw blob (ctu.utils.vqplane) where
    that is the smaller of the two."""
    codec = self.codec or self._binary_codec()
    with torch.no_grad():
      return codec.payloads(self._eval_code(codec, x_dict), x_dict)

  def decode_coded(self, payloads, x_dict):
    """decode() from what get_coded returned: a list of one `bytes` payload per label map.  ValueError, before any device
    work, without an encoder or a binarizer, for a label map that is no multiple of the encoder's down-sampling factor, a
    wrong payload count, an item that is not bytes, and a payload whose length table does not add up.
    With --encoder_quantizer s2hvq the items are the .jpdv blobs of get_coded; each header's n * code_len and L must fit the
    label map and the code book (checked on the host first); decode_coded(get_coded(x), x) equals get_img(x) bit for bit.
    A .jpdw blob (--vq_context_coder at the sender; told by its magic, no flag needed here) is taken in any item: its h, w, G
    and L must fit in the same way."""
    codec = self.codec or self._binary_codec()
    geo = codec.check_payloads(payloads, x_dict, 'decode_coded')
    with torch.no_grad():
      features = codec.features_of_payloads(payloads, geo, self._device, 'decode_coded')
      fake, _ = self._generate_from_code(features, x_dict, *geo[:3])
      return ops.nhwc_to_nchw(fake)

  def get_coded_rate(self, x_dict):
    """(coded bpp, raw bpp) averaged over the batch, two Python floats: 8 * file bytes / pixels of the .jpda file
    (ctu.utils.entropy: 24-byte header, and the raw payload where coding does not pay) and of the .jpdc file
    (ctu.utils.bitstream: 20-byte header) of each image.  Sizes of real files, not estimates; get_eval_rate is the
    reference's Shannon figure.  With --encoder_quantizer s2hvq: the .jpdv blobs, and the packed-index file of the same code."""
    payloads = self.get_coded(x_dict)
    return self.codec.file_rates(payloads, int(x_dict['image'].shape[-2]), int(x_dict['image'].shape[-1]))

  # ---- where the bits go (extension) ------------------------------------------------------------------------
  def get_rate_map(self, x_dict):
    """The code length of the eval-mode code (the one get_code / get_coded produce) under the 4.8 coder's own adaptive model,
    symbol by symbol (ops.code_cost): dict of float64 CPU tensors, `map` [N, h, w] bits per code cell, `per_channel` [N, C]
    bits, `bits` [N] and `bpp` [N] = bits / (H * W).  map and per_channel each sum to bits.  The model's ideal length, not a
    file size: get_coded_rate measures files, and stays within the bound of DESIGN.md 4.12 of this figure."""
    with torch.no_grad():
      r = ops.code_cost(self._code_act(x_dict, 'get_rate_map'))
      cell, channel = r['cell'].cpu(), r['channel'].cpu()
    pixels = int(x_dict['image'].shape[-2]) * int(x_dict['image'].shape[-1])
    unit = float(ops.CODE_COST_UNIT)
    bits = cell.sum(dim=(1, 2)).to(torch.float64) / unit            # integer sums first: exact
    return dict(map=cell.to(torch.float64) / unit, per_channel=channel.to(torch.float64) / unit, bits=bits, bpp=bits / pixels)

  def get_class_rates(self, x_dict):
    """The same code length attributed to the semantic classes of the pixels each code cell covers -- a cell's bits are
    shared evenly among its s*s pixels, s the encoder's down-sampling factor.  Rows: the n_onehot classes of
    get_eval_metrics(per_class=True) in its order, then one row for the pixels without a class.  dict(pixels int64, bits, bpp,
    share float64, each [n_classes + 1], over the batch: bits summed, bpp = bits of the class / pixels of the class (nan for
    an absent class), share = the class's fraction of all bits; per_image: the same four keys [N, n_classes + 1], share being
    the fraction of that image's bits)."""
    with torch.no_grad():
      b = self._code_act(x_dict, 'get_class_rates')
      label, _ = self._semantics(x_dict)
      r = ops.code_cost(b, label, self.n_onehot)
      units, pix = r['class_units'].cpu(), r['class_pixels'].cpu()
    s = int(label.shape[-1]) // b.W
    den = float(ops.CODE_COST_UNIT) * s * s

    def figures(u, p):                  # integer tensors [..., rows]
      bits = u.to(torch.float64) / den
      seen = p > 0
      nan = torch.full_like(bits, float('nan'))
      bpp = torch.where(seen, bits / torch.where(seen, p, torch.ones_like(p)).to(torch.float64), nan)
      total = u.sum(dim=-1, keepdim=True).to(torch.float64) / den
      return dict(pixels=p.clone(), bits=bits, bpp=bpp, share=bits / total)

    out = figures(units.sum(dim=0), pix.sum(dim=0))
    out['per_image'] = figures(units, pix)
    return out

  # ---- coded label and instance maps (extension) --------------------------------------------------------------
  def _label_set(self):
    """The label values a decoded map may hold: what the one-hot lanes of the input builder cover, 256 at the most."""
    return min(self.n_onehot, 256)

  def get_coded_semantics(self, x_dict, strip_rows=8):
    """The label and instance maps of x_dict as the receiver needs them, coded losslessly on the device
    (ops.semantics_encode): a list of N `bytes`, each the body of a .jpds file (ctu.utils.semantics).  The maps are coded as
    the dataset gives them -- --zero_ins / --zero_sem act where decode builds the generator input, not here; with
    --no_instance there is no instance plane.  ValueError for a label that is not an integer in [0, 255] or an instance id
    outside [0, 2^31)."""
    dev = self._device()
    label = x_dict['label'].to(dev, dtype=torch.float32, non_blocking=True).contiguous()
    inst = None
    if not getattr(self.opt, 'no_instance', False):
      inst = x_dict['instance'].to(dev, dtype=torch.int64, non_blocking=True).contiguous()
    if label.dim() != 4 or label.shape[1] != 1:
      raise ValueError('get_coded_semantics: the label map is [N, 1, H, W], got %s' % (tuple(label.shape),))
    H, W = int(label.shape[-2]), int(label.shape[-1])
    with torch.no_grad():
      items = ops.semantics_encode(label, inst, strip_rows)
    return [semantics_file.pack(H, W, strip_rows, item) for item in items]

  def decode_semantics(self, blobs):
    """{'label': float32 [N, 1, H, W], 'instance': int64 [N, 1, H, W]} on the device from what get_coded_semantics returned
    (or ctu.utils.semantics.read read): an x_dict for decode / decode_coded.  Without an instance plane the instance map is
    zeros.  ValueError, before any device work, for anything ctu.utils.semantics.unpack refuses and for blobs of different
    shapes; ValueError for a map that holds a label outside the label set, before the input builder sees it."""
    if not isinstance(blobs, (list, tuple)) or len(blobs) == 0:
      raise ValueError('decode_semantics: expected a list of .jpds bodies, one per image')
    parsed = [semantics_file.unpack(b, 'decode_semantics: blob %d' % j) for j, b in enumerate(blobs)]
    H, W, strip_rows, mask, _ = parsed[0]
    for j, q in enumerate(parsed):
      if q[:4] != (H, W, strip_rows, mask):
        raise ValueError('decode_semantics: blob %d is %d x %d, strips of %d rows, plane mask %d; blob 0 is %d x %d, %d, %d'
                         % ((j,) + q[:4] + (H, W, strip_rows, mask)))
    want = 1 if getattr(self.opt, 'no_instance', False) else 3
    if mask != want:
      raise ValueError('decode_semantics: the blobs have plane mask %d, this model reads %d (%s)'
                       % (mask, want, 'label only: --no_instance' if want == 1 else 'label and instance'))
    with torch.no_grad():
      label, inst = ops.semantics_decode([q[4] for q in parsed], H, W, strip_rows, self._label_set(), self._device())
    return {'label': label, 'instance': inst}

  def decode_from_files(self, coded_payloads, semantics_blobs):
    """The receiver from bytes alone: decode_coded(coded_payloads, decode_semantics(semantics_blobs))."""
    return self.decode_coded(coded_payloads, self.decode_semantics(semantics_blobs))

  def get_total_rate(self, x_dict, strip_rows=8):
    """(code bpp, semantics bpp, total bpp), Python floats, batch means: 8 * file bytes / pixels of the .jpda file of the
    code (get_coded_rate's first figure) and of the .jpds file of the maps, headers and raw fallbacks included -- the rate
    of everything decode_from_files needs."""
    code_bpp, _ = self.get_coded_rate(x_dict)
    blobs = self.get_coded_semantics(x_dict, strip_rows)
    H, W = int(x_dict['label'].shape[-2]), int(x_dict['label'].shape[-1])
    sem_bpp = sum(8.0 * len(b) / (H * W) for b in blobs) / len(blobs)
    return code_bpp, sem_bpp, code_bpp + sem_bpp

  def _eval_metrics_of(self, fake, image, label, per_class):
    """The tail get_eval_metrics and get_eval_metrics_decoded share: `fake` (the generator's NHWC output) against the original
    image (NCHW, any device), un-rounded as the reference uses it."""
    image = image.to(self._device(), dtype=torch.float32, non_blocking=True).contiguous()
    real32 = ops.nchw_to_nhwc(image, F32)
    if per_class:
      return ops.eval_metrics(fake, real32, self.opt.normalize_mean, self.opt.normalize_std, label, self.n_onehot)
    return ops.eval_metrics(fake, real32, self.opt.normalize_mean, self.opt.normalize_std)

  def get_eval_metrics_decoded(self, code, x_dict, per_class=False):
    """get_eval_metrics of the image a receiver reconstructs: the same dict, computed on decode(code, x_dict) against
    x_dict['image'].  Equal to get_eval_metrics(x_dict) for code = get_code(x_dict) under decode's zero rule: where the eval
    code holds an exact zero the decoder sees -1 and get_eval_metrics, like get_img, sees 0."""
    with torch.no_grad():
      fake, label = self._decode_act(code, x_dict)
      return self._eval_metrics_of(fake, x_dict['image'], label, per_class)

  def get_eval_metrics(self, x_dict, per_class=False):
    """Every distortion figure of the reference's test loop (test.py:114-125) from ONE generator forward: dict(l1, mse,
    psnr, ms_ssim, per_image) on the 0..255 scale of the quantised images (ops.eval_metrics; MS-SSIM: DESIGN.md 4.5).
    l1 / mse are the numbers get_eval_loss returns for --distortion_loss_fn l1 / mse.  per_class=True adds `per_class`:
    L1, MSE and PSNR of each of the n_onehot semantic classes from the same device pass (the intent of the reference's
    get_sem_wise_distortion, model.py:646-706; ops.eval_metrics_per_class)."""
    with torch.no_grad():
      pre = self.preprocess(x_dict, build_base=not self.zero_sem)
      fake, _ = self.netG.fwd(self._g_input_eval(pre))
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
        with self.codec.rate_term(self.rate_weight, B, H, W) if rate_on else contextlib.nullcontext():
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
      if opt.distortion_loss_fn == 'ms_ssim':
        # its own final kernel writes the slot (no jpdse_loss_finalize term): valid where the other slots are
        if gw.get('dist'):
          d_dist = ops.msssim_loss_fwd_bwd(fake, real, opt.normalize_mean, opt.normalize_std, s(layout['dist']), gw['dist'])
        else:
          ops.msssim_loss_fwd(fake, real, opt.normalize_mean, opt.normalize_std, s(layout['dist']))
      elif self.sem_weights is not None:
        # value and, in a training step, gradient from one pass; its own final kernel writes the slot
        d_dist = self._sem_weighted(fake, real, label, pre['inst_raw'], s(layout['dist']), gw.get('dist') or None)
      elif opt.distortion_loss_fn == 'l1' and gw.get('dist'):
        d_dist = ops.l1_fwd_bwd(fake, real, s(layout['dist']), gw['dist'])
      else:
        (ops.l1_fwd if opt.distortion_loss_fn == 'l1' else ops.mse_fwd)(fake, real, s(layout['dist']))
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

  def backward_G(self, state, w_gan, w_feat, w_vgg, w_dist):
    """d(loss_G)/d(netG params), loss_G = w_gan*G_GAN + w_feat*G_GAN_Feat + w_vgg*G_VGG + w_dist*G_Dist."""
    opt, B = self.opt, state['B']
    one = self._ones(state['fake'].t.device)
    fake, real = state['fake'], state['real']
    d_fake = None
    if (w_gan != 0.0 or w_feat != 0.0) and state['pred'] is not None:
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
      elif opt.distortion_loss_fn == 'ms_ssim':
        # the gradient needs the per-image means of all five scales: the op runs its forward again (the value goes to a scratch slot)
        dd = ops.msssim_loss_fwd_bwd(fake, real, opt.normalize_mean, opt.normalize_std,
                                     torch.empty(1, dtype=torch.float32, device=fake.t.device), w_dist)
      elif self.sem_weights is not None:
        # the forward was a value-only call: the op runs again for the gradient (the value goes to a scratch slot)
        dd = self._sem_weighted(fake, real, state['label'], state['inst_raw'],
                                torch.empty(1, dtype=torch.float32, device=fake.t.device), w_dist)
      else:
        fn = ops.l1_bwd if opt.distortion_loss_fn == 'l1' else ops.mse_bwd
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
    # gradient all-reduce (93 % of the bytes) the whole D backward to hide behind (launch_all below), instead of the
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

    did_G = self.backward_G(state, w_gan, w_feat, w_vgg, w_dist)
    mark('g_bwd_end')
    if did_G and bg is not None:
      bg.launch_all()                  # no-op for buckets already started from the per-layer hooks (defer=False)
    # (Measured and not adopted, round 4: Adam(G) + the panel re-pack -- 1.2 ms of HBM-bound streaming -- on a second stream
    # beside the discriminator's backward: 26.36-26.40 ms per step against 26.15-26.33 serial, profiles/r04_adam_side_stream_ab.txt.
    # The D backward is itself half HBM-bound passes, and its GEMM launches lose more to the shared CUs than Adam gains.)
    did_D = self.backward_D(state, 0.0 if opt.no_d_gan_loss else 0.5)
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
