"""The option surface of Pix2PixHDModel: the flag table (add_model_options), the --class_distortion_weights parser and
resolve_model_options, the ONE place where a flag meets its default and its checks.  Host code only: nothing here loads the
shared library or asks for a device, so every refusal comes before any network (hence any device allocation) exists.
tests/golden/model_option_refusals.json pins every refusal and the order of the checks, tests/golden/model_option_table.json
the flag table."""
import collections

from jpdse_hip import ops


def add_model_options(parser, train):
  """Every flag of the reference setter (pix2pixHD_model.py:21-102) with the same name, type, default and choices
  (pinned by tests/golden/option_setter_flags.json, dumped from the reference), so that a reference command line or
  opt.pkl parses unchanged; flags of branches outside the accelerated path are accepted here and refused in
  resolve_model_options when they would change the computation.  Extensions: --compute_dtype, --skip_unused_losses,
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


# feat_enc: the learned codec, G sees [semantics | netE(image)]; quantizer: --encoder_quantizer as given; encoder_runs: an encoder
# with its bottleneck whose output reaches the generator (no --zero_vis); sem_weights: (class table, edge weight), or None when
# every weight is 1; compute_dtype: 'fp32' / 'bf16'; feat_nc (the encoder's output channels), nef, n_downsample_E and the keyword
# arguments encoder_args: what networks.define_G takes for the encoder; the last five: what the constructor reads behind network
# construction; lambda_vq_stage_rate: the weight of the residual bottleneck's rate term; vq_stages /
# vq_train_stages: the residual bottleneck's code books and its training schedule
ModelOptions = collections.namedtuple('ModelOptions', [
    'feat_enc', 'quantizer', 'encoder_runs', 'lambda_rate', 'lambda_vq_rate', 'vq_context_coder', 'sem_weights', 'compute_dtype',
    'n_onehot', 'label_nc', 'feat_nc', 'zero_vis', 'zero_sem', 'zero_ins', 'no_instance', 'codec_seed',
    'nef', 'n_downsample_E', 'encoder_args',
    'checkpoint_resblocks', 'load_model', 'vgg19_state_dict', 'no_vgg_loss', 'vgg_random_init', 'lambda_vq_stage_rate',
    'vq_stages', 'vq_train_stages'])


def parse_vq_class_stages(spec, vq_stages, n_classes):
  """opt.vq_class_stages, a string such as '24:3,26:3,*:1' -- class id : stage depth, '*' the depth of every class
  not named (default: vq_stages) -> (table, default): table a tuple of n_classes depths, default the depth of a pixel whose label
  is no class of the table.  None for None.  ValueError naming the field for a malformed entry, a class outside [0, n_classes), a
  class or '*' named twice, and a depth outside 1 .. vq_stages."""
  if spec is None:
    return None
  if not isinstance(spec, str) or not spec.strip():
    raise ValueError("vq_class_stages must be a string such as '24:3,26:3,*:1' (class:depth, '*' for the others), got %r" % (spec,))
  named, default = {}, None
  for item in spec.split(','):
    parts = item.strip().split(':')
    if len(parts) != 2 or not parts[1].strip().isdigit() or not (parts[0].strip() == '*' or parts[0].strip().isdigit()):
      raise ValueError("vq_class_stages: malformed entry %r in %r (class:depth, '*' for the others)" % (item, spec))
    key, depth = parts[0].strip(), int(parts[1])
    if not 1 <= depth <= vq_stages:
      raise ValueError('vq_class_stages: depth %d of %r is outside 1 .. vq_stages = %d' % (depth, key, vq_stages))
    if key == '*':
      if default is not None:
        raise ValueError("vq_class_stages: malformed entry %r in %r ('*' is named twice)" % (item, spec))
      default = depth
      continue
    if not 0 <= int(key) < n_classes:
      raise ValueError('vq_class_stages: malformed entry %r in %r (class %d is outside the %d classes of the label map)'
                       % (item, spec, int(key), n_classes))
    if int(key) in named:
      raise ValueError('vq_class_stages: malformed entry %r in %r (class %d is named twice)' % (item, spec, int(key)))
    named[int(key)] = depth
  default = vq_stages if default is None else default
  return tuple(named.get(k, default) for k in range(n_classes)), default


def resolve_vq_class_stages(opt):
  """(table, default) of opt.vq_class_stages, or None when the field is absent or None: today's model.  The refusals that need the
  other options: vq_stages == 1, lambda_vq_stage_rate > 0, --zero_sem.  resolve_model_options calls this after
  its own checks of those options, so ModelOptions stays the record it was; the model's constructor reads the value here."""
  spec = getattr(opt, 'vq_class_stages', None)
  if spec is None:
    return None
  vq_stages = getattr(opt, 'vq_stages', 1)
  if vq_stages == 1 or getattr(opt, 'encoder_quantizer', 'binarizer') != 's2hvq':
    raise ValueError('vq_class_stages sets the stage depth of the residual bottleneck per class: it needs --encoder_quantizer s2hvq '
                     'and vq_stages > 1')
  if float(getattr(opt, 'lambda_vq_stage_rate', 0.0) or 0.0) > 0.0:
    raise ValueError('vq_class_stages cannot be combined with lambda_vq_stage_rate > 0: the rate term has no depth form')
  if getattr(opt, 'zero_sem', False):
    raise ValueError('vq_class_stages cannot be combined with --zero_sem: the generator sees no semantics there')
  n_onehot = opt.num_labels + 1 if getattr(opt, 'contain_dontcare_label', False) else opt.num_labels
  return parse_vq_class_stages(spec, vq_stages, n_onehot)


def resolve_model_options(opt):
  """opt -> ModelOptions, or the refusal.  The order of the checks is part of the contract: first everything outside the
  accelerated path in ONE NotImplementedError, then distortion_loss_fn, lambda_rate, lambda_vq_rate, vq_context_coder,
  encoder_quantizer (with the bottleneck's own check), vq_stages and vq_train_stages (opt fields without a flag),
  lambda_vq_stage_rate (an opt field without a flag), then the class weights, the edge weight and their conflict with ms_ssim."""
  g = lambda name, default=False: getattr(opt, name, default)
  feat_enc = not g('no_feat_encoding')
  bottleneck = feat_enc and not g('no_encoder_binarization')
  zero_vis, zero_sem, no_instance = bool(g('zero_vis')), bool(g('zero_sem')), bool(g('no_instance'))
  encoder_runs = bottleneck and not zero_vis
  quantizer = g('encoder_quantizer', 'binarizer')
  netG, n_downsample_E, pool_size, norm = g('netG', 'global'), g('n_downsample_E', 4), g('pool_size', 0), g('norm', 'instance')
  enc = dict(binarize_encoder=not g('no_encoder_binarization'), encoder_groups=g('netE_groups', 1), encoder_quantizer=quantizer,
             encoder_binarizer_out_channels=g('encoder_binarizer_out_channels', 128), vq_n_center=g('vq_n_center', 64),
             vq_center_size=g('vq_center_size', 8), vq_sigma=g('vq_sigma', 10.0), vq_hard_forward=not g('vq_soft_forward'))

  unsupported = []
  # learned codec (feature encoder netE): accepted for the global generator
  if not g('no_label_encoding'):
    unsupported.append('the learned label encoder netE4label (run with --no_label_encoding)')
  if not g('no_generator_binarization'):
    unsupported.append('generator binarization (run with --no_generator_binarization)')
  if feat_enc:
    if netG != 'global':
      unsupported.append('learned feature encoding with --netG %s (only the global generator back-propagates into its '
                         'input; run with --netG global or --no_feat_encoding)' % netG)
    if enc['encoder_groups'] != 1:
      unsupported.append('--netE_groups %s' % enc['encoder_groups'])
    if n_downsample_E < 1:
      unsupported.append('--n_downsample_E %s (an encoder without downsampling)' % n_downsample_E)
    if pool_size > 0:
      unsupported.append('--pool_size %s' % pool_size)
  for flag in ('sem_masking', 'no_label', 'no_feat', 'match_raw_feat', 'no_lsgan', 'use_netE_output', 'binary_mask',
               'inst_wise_pool'):
    if g(flag):
      unsupported.append('--' + flag)
  if norm != 'instance':
    unsupported.append('--norm ' + str(norm))
  if unsupported:
    raise NotImplementedError('outside the accelerated JPD-SE path (SURVEY.md §2): ' + '; '.join(unsupported))
  if opt.distortion_loss_fn not in ('l1', 'mse', 'ms_ssim'):
    raise ValueError('distortion_loss_fn must be l1, mse or ms_ssim')
  lambda_rate = float(g('lambda_rate', 0.0) or 0.0)
  if not lambda_rate >= 0.0:
    raise ValueError('lambda_rate must be a non-negative number, got %r' % (g('lambda_rate'),))
  if lambda_rate > 0.0 and not encoder_runs:
    raise ValueError('lambda_rate > 0 needs the learned codec with encoder binarization (--no_feat_encoding and '
                     '--no_encoder_binarization must both be off) and an encoder that runs (no --zero_vis)')
  # rate term of the vector-quantizer bottleneck
  lvr = g('lambda_vq_rate', 0.0)
  lambda_vq_rate = float(0.0 if lvr is None or lvr is False else lvr)
  if not (lambda_vq_rate >= 0.0 and lambda_vq_rate != float('inf')):
    raise ValueError('lambda_vq_rate must be a finite non-negative number, got %r' % (lvr,))
  if lambda_vq_rate > 0.0 and (quantizer != 's2hvq' or zero_vis):
    raise ValueError('lambda_vq_rate > 0 is the rate term of the vector-quantizer bottleneck: it needs --encoder_quantizer '
                     's2hvq and an encoder that runs (no --zero_vis)')
  # context coder of the vector-quantizer bottleneck's files
  vq_context_coder = bool(g('vq_context_coder'))
  if vq_context_coder and quantizer != 's2hvq':
    raise ValueError('--vq_context_coder codes the index planes of the vector-quantizer bottleneck: it needs '
                     '--encoder_quantizer s2hvq')
  # vector-quantizer bottleneck
  if quantizer not in ('binarizer', 's2hvq'):
    raise ValueError('encoder_quantizer must be binarizer or s2hvq, got %r' % (quantizer,))
  if quantizer == 's2hvq':
    if not bottleneck:
      raise ValueError('--encoder_quantizer s2hvq needs the learned codec with its bottleneck (--no_feat_encoding and '
                       '--no_encoder_binarization must both be off)')
    if lambda_rate > 0.0:
      raise ValueError('--lambda_rate > 0 is the binarizer\'s context-model rate term: it cannot be combined with '
                       '--encoder_quantizer s2hvq')
    from jpdse_hip.layers import vq_bottleneck_check
    vq_bottleneck_check(int(enc['encoder_binarizer_out_channels']), int(enc['vq_n_center']), int(enc['vq_center_size']),
                        enc['vq_sigma'], '--encoder_quantizer s2hvq')
  # residual bottleneck: fields a caller sets on the parsed namespace; absent or 1 / 'all': nothing changes
  vq_stages = g('vq_stages', 1)
  if isinstance(vq_stages, bool) or not isinstance(vq_stages, int) or not 1 <= vq_stages <= ops.VQ_RES_MAX_STAGES:
    raise ValueError('vq_stages must be an int in 1 .. %d, got %r' % (ops.VQ_RES_MAX_STAGES, vq_stages))
  if vq_stages > 1:
    if quantizer != 's2hvq':
      raise ValueError('vq_stages = %d is the stage count of the vector-quantizer bottleneck: it needs --encoder_quantizer s2hvq'
                       % vq_stages)
    if not enc['vq_hard_forward']:
      raise ValueError('vq_stages = %d cannot be combined with --vq_soft_forward: the soft forward is built for one stage' % vq_stages)
    if lambda_vq_rate > 0.0:
      raise ValueError('vq_stages = %d cannot be combined with --lambda_vq_rate > 0: the rate term is built for one stage' % vq_stages)
    if vq_context_coder:
      raise ValueError('vq_stages = %d cannot be combined with --vq_context_coder: the context coder is built for one stage'
                       % vq_stages)
  vq_train_stages = g('vq_train_stages', 'all')
  if vq_train_stages not in ('all', 'uniform'):
    raise ValueError("vq_train_stages must be 'all' or 'uniform', got %r" % (vq_train_stages,))
  if vq_train_stages == 'uniform' and vq_stages == 1:
    raise ValueError("vq_train_stages = 'uniform' draws a stage prefix per step: it needs vq_stages > 1")
  enc['vq_stages'] = vq_stages
  # rate term of the residual bottleneck: a field a caller sets on the parsed namespace; absent or 0: nothing changes
  lvs = g('lambda_vq_stage_rate', 0.0)
  lvs = 0.0 if lvs is None or lvs is False else lvs
  if isinstance(lvs, bool) or not isinstance(lvs, (int, float)) or not (float(lvs) >= 0.0 and float(lvs) != float('inf')):
    raise ValueError('lambda_vq_stage_rate must be a finite number >= 0, got %r' % (lvs,))
  lambda_vq_stage_rate = float(lvs)
  if lambda_vq_stage_rate > 0.0 and vq_stages == 1:
    raise ValueError('lambda_vq_stage_rate > 0 is the rate term of the residual bottleneck: it needs vq_stages > 1 (the one-stage '
                     'bottleneck takes --lambda_vq_rate)')
  if lambda_vq_stage_rate > 0.0 and zero_vis:
    raise ValueError('lambda_vq_stage_rate > 0 needs an encoder that runs: it cannot be combined with --zero_vis')
  resolve_vq_class_stages(opt)      # opt.vq_class_stages: its refusals; the value is the constructor's to read
  # semantics-weighted distortion: (class table, edge weight), or None when every weight is 1 -- the
  # step then takes the plain l1 / mse path
  n_onehot = opt.num_labels + 1 if g('contain_dontcare_label') else opt.num_labels
  table = parse_class_distortion_weights(g('class_distortion_weights', ''), min(n_onehot, ops.SEM_TABLE))
  edge_w = g('edge_distortion_weight', 1.0)
  edge_w = 1.0 if edge_w is None else float(edge_w)
  if not (edge_w >= 0.0 and edge_w != float('inf')):
    raise ValueError('edge_distortion_weight must be a finite number >= 0, got %r' % (g('edge_distortion_weight'),))
  if edge_w != 1.0 and no_instance:
    raise ValueError('edge_distortion_weight != 1 needs the instance map: it cannot be combined with --no_instance')
  sem_weights = None
  if edge_w != 1.0 or any(w != 1.0 for w in table):
    if opt.distortion_loss_fn == 'ms_ssim':
      raise ValueError('class_distortion_weights / edge_distortion_weight weight the l1 and mse distortions only: they '
                       'cannot be combined with --distortion_loss_fn ms_ssim')
    sem_weights = (table, edge_w)
  return ModelOptions(
      feat_enc=feat_enc, quantizer=quantizer, encoder_runs=encoder_runs, lambda_rate=lambda_rate, lambda_vq_rate=lambda_vq_rate,
      vq_context_coder=vq_context_coder, sem_weights=sem_weights,
      compute_dtype='bf16' if (g('compute_dtype', 'fp32') == 'bf16' or g('fp16')) else 'fp32',
      # channel bookkeeping (pix2pixHD_model.py:117-158); generator input: semantics + encoded image (feat_num channels) or +
      # the image itself (model.py:135-139)
      n_onehot=n_onehot, label_nc=n_onehot + (0 if no_instance else 1), feat_nc=g('feat_num', 3) if feat_enc else opt.input_nc,
      # ablation inputs (model.py:583-606): blank the visual lanes, every semantic lane, or the instance-edge lane of G's input;
      # the edge lane is only consulted when the semantics stay and an edge lane exists (model.py:588)
      zero_vis=zero_vis, zero_sem=zero_sem, zero_ins=bool(g('zero_ins')) and not zero_sem and not no_instance,
      no_instance=no_instance, codec_seed=int(g('seed', None) or 0), nef=g('nef', 64), n_downsample_E=n_downsample_E,
      encoder_args=enc, checkpoint_resblocks=bool(g('checkpoint_resblocks')), load_model=bool(g('load_model')),
      vgg19_state_dict=g('vgg19_state_dict', None), no_vgg_loss=bool(g('no_vgg_loss')), vgg_random_init=bool(g('vgg_random_init')),
      lambda_vq_stage_rate=lambda_vq_stage_rate, vq_stages=vq_stages, vq_train_stages=vq_train_stages)
