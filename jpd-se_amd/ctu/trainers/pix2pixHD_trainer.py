"""JPD-SE trainer on the MI355X-native model (reference: ctu/trainers/pix2pixHD_trainer.py).

`step()` keeps the reference's observable contract -- same loss weighting (:48-56), same
update order G then D (:64-78), returns the G_Distortion float (:85) -- but runs the explicit
HIP schedule of `Pix2PixHDModel.train_step` with a single host sync, and adds what the
reference lacks: per-image data parallelism over torch.distributed (RCCL) when a process
group is initialised."""
import os

import torch
import torch.distributed as dist
from torch.optim.lr_scheduler import ReduceLROnPlateau

from ctu.models.pix2pixHD_model import Pix2PixHDModel
from ctu.trainers.base_trainer import BaseTrainer
from jpdse_hip.ddp import GradBuckets
from jpdse_hip.layers import HipConv2d, HipVQBottleneck, HipResidualVQBottleneck, bump_weights_epoch


class Pix2PixHDTrainer(BaseTrainer):

  def __init__(self, opt, mode='train'):
    super(Pix2PixHDTrainer, self).__init__(opt, mode)
    self.model = Pix2PixHDModel(opt)
    self.print_losses = getattr(opt, 'print_losses', True)
    if mode == 'train':
      self.optimizer_G, self.optimizer_D = self.model.create_optimizers(opt)
      if getattr(opt, 'schedule_lr', False):
        self.scheduler_G = ReduceLROnPlateau(self.optimizer_G, 'min', factor=opt.lr_decay_factor,
                                             patience=opt.lr_decay_patience)
        self.scheduler_D = ReduceLROnPlateau(self.optimizer_D, 'min', factor=opt.lr_decay_factor,
                                             patience=opt.lr_decay_patience)
      self.lambda_distortion_weight = 1.
      self._dp = None
      if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        self.enable_data_parallel(reduce_dtype=torch.bfloat16 if getattr(opt, 'bf16_grad_reduce', False) else None)

  # ---- data parallelism (no reference counterpart: base_parser.py:234-237 refuses >1 GPU) ----
  def enable_data_parallel(self, bucket_bytes=None, process_group=None, reduce_dtype=None, overlap=None):
    """Replicate-and-average: broadcast rank 0's weights once, re-home every gradient into flat all-reduce buckets, and
    let Adam divide by the world size.  Runs for any initialised process group, world size 1 included (the RCCL
    calls are then no-ops in value, which is how the path is exercised on a one-GPU box).  reduce_dtype
    torch.bfloat16 halves the bytes on the wire (SURVEY.md 8d config 4 reports both)."""
    world = dist.get_world_size(process_group)
    nets = [self.model.netG, self.model.netD] + ([self.model.netE] if self.model.netE is not None else [])
    for net in nets:
      for p in net.parameters():
        # 4-D masters are channels_last: hand the collective the dense KRSC view of the same memory
        dense = p.data.permute(0, 2, 3, 1) if p.dim() == 4 else p.data
        assert dense.is_contiguous()
        dist.broadcast(dense, src=0, group=process_group)
    bump_weights_epoch()
    # overlap: where the generator's gradient all-reduce runs.  'd_backward' (default): all of G's buckets start when G's
    # backward has finished and overlap the discriminator's backward; 'layers': each bucket starts from the backward hook
    # of its last layer and overlaps the rest of G's backward (round 1-2 behaviour).  Same results either way.
    overlap = overlap or getattr(self.opt, 'ddp_overlap', 'd_backward')
    assert overlap in ('d_backward', 'layers'), overlap
    if bucket_bytes is None:
      # 'layers': 64 MB buckets (one ResnetBlock filter = 37.7 MB each) so that a bucket goes on the wire as soon as its layer is
      # done; 'd_backward': everything starts at once, so fewer and larger collectives (256 MB: the generator's 730 MB in 3 + the
      # small layers) -- a ring all-reduce's fixed cost (2 (N-1) hops of latency + a kernel launch) is paid per bucket
      bucket_bytes = (64 << 20) if overlap == 'layers' else (256 << 20)
    self.model.codec_process_group = process_group     # images are indexed within this group (learned-codec noise)
    self._dp = dict(bucket_bytes=bucket_bytes, process_group=process_group, reduce_dtype=reduce_dtype, world=world,
                    overlap=overlap)
    self._rebuild_buckets('G', self._g_bucket_nets(), self.optimizer_G)
    self._rebuild_buckets('D', self.model.netD, self.optimizer_D)

  def _g_bucket_nets(self):
    """The networks optimizer G trains, in forward order of the backward's reverse: netE (its gradients are written last)
    then netG -- the buckets follow reverse-backward order."""
    if self.model.netE is None:
      return self.model.netG
    return torch.nn.ModuleList([self.model.netE, self.model.netG])

  def _rebuild_buckets(self, tag, net, optim):
    """(Re)create the gradient buckets of one network over the parameters its optimizer trains, fold 1/world into the
    optimizer and point every conv's gradient-ready hook at the new buckets."""
    dp = self._dp
    trained = {id(p) for grp in optim.param_groups for p in grp['params']}
    named = [(n, p) for n, p in net.named_parameters() if id(p) in trained]
    buckets = GradBuckets(named, bucket_bytes=dp['bucket_bytes'], process_group=dp['process_group'],
                          reduce_dtype=dp['reduce_dtype'], always_reduce=True,
                          defer=(tag == 'G' and dp.get('overlap', 'd_backward') == 'd_backward'))
    self.model.grad_buckets[tag] = buckets
    optim.grad_scale = 1.0 / dp['world']
    for m in net.modules():
      if isinstance(m, HipConv2d):
        m.grad_ready_hook = (lambda mod, b=buckets: (b.mark_ready(mod.weight), b.mark_ready(mod.bias)))
      elif isinstance(m, HipVQBottleneck):
        m.grad_ready_hook = (lambda mod, b=buckets: b.mark_ready(mod.vq._code_book))
      elif isinstance(m, HipResidualVQBottleneck):
        m.grad_ready_hook = (lambda mod, b=buckets: b.mark_ready(mod.vq._code_books))

  def update_fixed_params(self):
    """End of the `niter_fix_global` phase (train.py calls model.update_fixed_params and swaps the optimizer,
    pix2pixHD_model.py:795-804): from now on the coarse generator trains too.  The trainer owns the transition so
    that, under data parallelism, the new parameters get gradient buckets, hooks and the 1/world scale as well."""
    self.optimizer_G = self.model.update_fixed_params(self.optimizer_G)
    if getattr(self, '_dp', None) is not None:
      self._rebuild_buckets('G', self._g_bucket_nets(), self.optimizer_G)
    if getattr(self.opt, 'schedule_lr', False):
      self.scheduler_G = ReduceLROnPlateau(self.optimizer_G, 'min', factor=self.opt.lr_decay_factor,
                                           patience=self.opt.lr_decay_patience)
    return self.optimizer_G

  def scheduler_step(self, val_loss_value):
    self.scheduler_G.step(val_loss_value)
    self.scheduler_D.step(val_loss_value)

  def step(self, x_dict):
    self.train()
    L = self.model.train_step(x_dict, self.optimizer_G, self.optimizer_D, self.lambda_distortion_weight)
    self.last_losses = L
    if self.print_losses:
      print('g_gan: {:.4f}, g_gan_feat_match: {:.4f}, g_vgg: {:.4f}, g_distortion ({}): {:.4f}, d_real: {:.4f}, '
            'd_fake: {:.4f}'.format(L['G_GAN'], L['G_GAN_Feat'], L['G_VGG'], self.opt.distortion_loss_fn,
                                    L['G_Distortion'], L['D_real'], L['D_fake'])
            + (', g_rate: {:.4f}'.format(L['G_Rate']) if 'G_Rate' in L else ''))
    self.steps_taken += 1
    if self.opt.anneal_lambda and not (self.steps_taken % self.opt.anneal_interval):
      self.lambda_distortion_weight *= self.opt.anneal_factor
    if getattr(self.opt, 'tf_log', False):
      self.log_loss_values(L)
    return L['G_Distortion']

  def get_eval_loss(self, x_dict):
    self.eval()
    return self.model(x_dict, self.opt, mode='get_eval_loss').item()

  def get_code(self, x_dict, packed=False):
    """The image's binary code as ONE tensor (pix2pixHD_trainer.py:100-103: torch.cat over the model's code list): fp32
    [N, bits] of 0 / 1 on the GPU, or (packed=True, extension) the uint8 bitstream [N, ceil(bits / 8)]."""
    self.eval()
    with torch.no_grad():
      return torch.cat([c for c in self.model.get_code(x_dict, packed) if c is not None], dim=-1)

  def get_vq_code(self, x_dict, rate_lambda=0.0, n_iter=2, stages=None):
    """The code of the vector-quantizer bottleneck (--encoder_quantizer s2hvq): int64 [N, h * w * C / D] on the
    device.  decode(get_vq_code(x), x) equals get_img(x) bit for bit; get_coded / decode_coded / get_coded_rate store it as
    .jpdv blobs.  rate_lambda > 0: the entropy-constrained code, a lower rate from the same trained model;
    the receiver is untouched.  With opt.vq_stages > 1: int64 [N, stages, h * w * C / D], stored as .jpdr
    blobs; every stage prefix code[:, :n] decodes."""
    self.eval()
    return self.model.get_vq_code(x_dict, rate_lambda=rate_lambda, n_iter=n_iter, stages=stages)

  def get_coded_stages(self, x_dict, stages=None):
    """get_coded of the first `stages` stages of a residual bottleneck (opt.vq_stages > 1): byte for byte
    vqstages.truncate_stages of get_coded's blobs."""
    self.eval()
    return self.model.get_coded_stages(x_dict, stages=stages)

  def get_stage_curve(self, x_dict, rate_lambda=0.0, n_iter=2):
    """The rate-distortion points of one coded stream cut after every stage (opt.vq_stages > 1): a list of
    vq_stages dicts, one per prefix n = 1 .. vq_stages: `stages`, `bpp` (8 * the bytes of vqstages.truncate_stages(blob, n) per
    pixel, batch mean) and `l1`, `mse`, `psnr`, `ms_ssim` of get_eval_metrics_decoded of that prefix.  One encoder run, one
    generator run per prefix.  rate_lambda > 0: the curve of the stream get_coded_stages_ec(x_dict, rate_lambda,
    n_iter) writes; the defaults take the plain code."""
    from ctu.models.codec import check_ec_arguments
    self.eval()
    if check_ec_arguments(rate_lambda, n_iter) > 0:
      code = self.model.get_stage_code_ec(x_dict, rate_lambda, n_iter=n_iter)
    else:
      code = self.model.get_vq_code(x_dict)
    if code.dim() != 3:
      raise ValueError('get_stage_curve: needs a residual bottleneck (opt.vq_stages > 1)')
    blobs = self.model.codec.payloads(code, x_dict)
    pixels = int(x_dict['image'].shape[-2]) * int(x_dict['image'].shape[-1])
    rows = []
    for n in range(1, int(code.shape[1]) + 1):
      m = self.model.get_eval_metrics_decoded(code[:, :n].contiguous(), x_dict)
      bpp = sum(8.0 * len(self.model.codec.truncate(b, n)) / pixels for b in blobs) / len(blobs)
      rows.append(dict(stages=n, bpp=bpp, l1=m['l1'], mse=m['mse'], psnr=m['psnr'], ms_ssim=m['ms_ssim']))
    return rows

  def _depth_codec(self, who):
    from ctu.models.codec import VQDepthCodec
    if not isinstance(self.model.codec, VQDepthCodec):
      raise ValueError('%s: needs opt.vq_class_stages (DESIGN.md 4.27)' % who)
    return self.model.codec

  def get_stage_depth(self, x_dict):
    """int64 [N, h, w] on the device: the stage depth of every code cell under opt.vq_class_stages -- the maximum
    over the cell's pixels of the depth of the pixel's class -- as every call of the model derives it from x_dict's label map."""
    codec = self._depth_codec('get_stage_depth')
    with torch.no_grad():
      label, _ = self.model._semantics(x_dict)
      return codec.device_depth(label).to(torch.int64)

  def get_depth_report(self, x_dict):
    """A list of N dicts, one per image, of the .jpdm stream get_coded writes under opt.vq_class_stages: `cells` (cells per depth
    1 .. vq_stages), `indices` and `bytes` per stage (the stage's .jpdv blob; 0 for a stage without a cell), `total_bytes` and
    `bpp` of the whole file, headers included."""
    from ctu.utils import vqdepth
    codec = self._depth_codec('get_depth_report')
    self.eval()
    blobs = self.model.get_coded(x_dict)
    depth = self.get_stage_depth(x_dict).cpu()
    S, groups = self.model.vq_stages, codec.geometry(x_dict, 'get_depth_report')[5]
    pixels = int(x_dict['image'].shape[-2]) * int(x_dict['image'].shape[-1])
    rows = []
    for j, b in enumerate(blobs):
      _, _, _, _, counts, inner = vqdepth.parse_depth_stages(b, 'get_depth_report: blob %d' % j)
      rows.append(dict(cells=[int((depth[j] == v).sum()) for v in range(1, S + 1)], indices=[c * groups for c in counts],
                       bytes=[len(i) for i in inner], total_bytes=len(b), bpp=8.0 * len(b) / pixels))
    return rows

  def get_stage_code_ec(self, x_dict, rate_lambda, n_iter=2, stages=None):
    """The entropy-constrained code of a residual bottleneck (opt.vq_stages > 1): int64 [N, stages, h * w * C /
    D]; decode takes it unchanged and every stage prefix is the shorter encoder's code."""
    self.eval()
    return self.model.get_stage_code_ec(x_dict, rate_lambda, n_iter=n_iter, stages=stages)

  def get_coded_stages_ec(self, x_dict, rate_lambda, n_iter=2, stages=None):
    """The .jpdr blobs of get_stage_code_ec: decode_coded and vqstages.truncate_stages take them unchanged."""
    self.eval()
    return self.model.get_coded_stages_ec(x_dict, rate_lambda, n_iter=n_iter, stages=stages)

  def get_stage_ec_report(self, x_dict, rate_lambda, n_iter=2, stages=None):
    """The per-image reports (distortion and bits per round and stage, cost per round) of get_stage_code_ec."""
    self.eval()
    return self.model.get_stage_ec_report(x_dict, rate_lambda, n_iter=n_iter, stages=stages)

  def get_stage_usage(self, x_dict):
    """int64 [S, G, L] on the device: how often every stage of the eval-mode code uses each centre, per channel group, over the
    batch.  A zero column is a dead centre of that stage."""
    self.eval()
    return self.model.get_stage_usage(x_dict)

  def get_stage_rates(self, x_dict):
    """A list of S floats: the zero-order entropy of every stage's code per channel group in bits per pixel of the batch
    (DESIGN.md 4.25).  An estimate next to get_stage_curve's file sizes."""
    self.eval()
    return self.model.get_stage_rates(x_dict)

  def get_vq_ec_report(self, x_dict, rate_lambda, n_iter=2):
    """The per-image reports (distortion, bits, cost per round) of the entropy-constrained code."""
    self.eval()
    return self.model.get_vq_ec_report(x_dict, rate_lambda, n_iter=n_iter)

  def get_vq_rate(self, x_dict):
    """The entropy estimate of the vector-quantised code in bits per pixel (extension), a Python float: the
    hard-mode rate term of --lambda_vq_rate on the eval-mode code -- the zero-order entropy of get_vq_code(x_dict) per channel
    group, histograms over the batch.  An estimate, not a size, with no fixed order against get_coded_rate's coded figure."""
    self.eval()
    return self.model.get_vq_rate(x_dict)

  def get_vq_usage(self, x_dict):
    """int64 [G, L] on the device: how often the eval-mode vector-quantised code of x_dict uses each centre, per channel group
    (extension).  A zero column is a dead centre."""
    self.eval()
    return self.model.get_vq_usage(x_dict)

  def fit_vq_code_book(self, x_dicts, n_iter=10, init='sample', seed=0, reseed=True):
    """Fit the vector quantizer's code book to the encoder's features of a list of batches by k-means on the device, dead
    centres reseeded (extension): Pix2PixHDModel.fit_vq_code_book.  In place -- the optimizer keeps working on
    the same tensor; deterministic and without a collective: call it on every rank with the same batches.  Returns the report
    dict (distortion, dead, reseeded, counts); with opt.vq_stages > 1 the list of per-stage reports."""
    self.eval()
    return self.model.fit_vq_code_book(x_dicts, n_iter=n_iter, init=init, seed=seed, reseed=reseed)

  def get_eval_rate(self, x_dict):
    """(Shannon bpp in nats as the reference computes it, raw bpp) of the learned codec (pix2pixHD_trainer.py:106-110)."""
    self.eval()
    return self.model(x_dict, self.opt, mode='get_eval_rate')

  def get_eval_metrics(self, x_dict, per_class=False):
    """L1, MSE, PSNR and MS-SSIM of the reconstruction (test.py:114-125) from one generator forward: dict of Python floats
    (batch means) plus `per_image`, four float64 CPU tensors [B].  per_class=True adds `per_class`: pixels, l1, mse and psnr
    of every semantic class ([n_classes], pixel-weighted over the batch, 0 for an absent class), `unlabelled` and the same
    four keys `per_image` ([B, n_classes]), from the same device pass."""
    self.eval()
    return self.model(x_dict, self.opt, mode='get_eval_metrics_per_class' if per_class else 'get_eval_metrics')

  def get_weighted_distortion(self, x_dict):
    """The training distortion (l1 / mse, un-quantised, normalised scale) of the eval-mode reconstruction under the model's
    --class_distortion_weights / --edge_distortion_weight (extension), a Python float.  With trivial weights
    the plain mean.  get_eval_loss and get_eval_metrics stay the reference's unweighted, quantised figures."""
    self.eval()
    return self.model.get_weighted_distortion(x_dict)

  def get_img(self, x_dict):
    self.eval()
    return self.model(x_dict, self.opt, mode='get_img')

  def decode(self, code, x_dict):
    """The receiver of the learned codec: the image reconstructed from `code` (what get_code returned, either form, CPU or
    device) and x_dict['label'] / x_dict['instance'] alone.  Equal to get_img(x_dict) bit for bit unless the eval code
    holds an exact zero, which is stored as a 0 bit and decoded as -1 (Pix2PixHDModel.decode)."""
    self.eval()
    return self.model.decode(code, x_dict)

  def get_eval_metrics_decoded(self, code, x_dict, per_class=False):
    """get_eval_metrics of decode(code, x_dict) against x_dict['image']: what a receiver of the stored code reconstructs."""
    self.eval()
    return self.model.get_eval_metrics_decoded(code, x_dict, per_class)

  def get_coded(self, x_dict):
    """The entropy-coded bitstream (extension): a list with one `bytes` payload per image, the lossless
    range-coded form of get_code(x_dict, packed=True).  ctu.utils.entropy.write_coded stores one as a .jpda file."""
    self.eval()
    return self.model.get_coded(x_dict)

  def get_coded_ec(self, x_dict, rate_lambda=0.0, n_iter=2):
    """get_coded of the entropy-constrained code get_vq_code(x_dict, rate_lambda, n_iter); the defaults give
    get_coded's bytes.  --encoder_quantizer s2hvq only for rate_lambda > 0."""
    self.eval()
    return self.model.get_coded_ec(x_dict, rate_lambda=rate_lambda, n_iter=n_iter)

  def decode_coded(self, payloads, x_dict):
    """decode() from the payloads get_coded returned: equal to decode(get_code(x_dict, packed=True), x_dict) bit for bit.
    A wrong payload count, an item that is not bytes or an inconsistent length table is a ValueError before device work."""
    self.eval()
    return self.model.decode_coded(payloads, x_dict)

  def get_coded_rate(self, x_dict):
    """(coded bpp, raw bpp), Python floats, batch means: the sizes of the .jpda and of the .jpdc file of each image, headers
    included, in bits per pixel.  What a coder produced -- next to get_eval_rate's Shannon estimate, which stays as it is."""
    self.eval()
    return self.model.get_coded_rate(x_dict)

  def get_coded_rate_ec(self, x_dict, rate_lambda=0.0, n_iter=2):
    """(coded bpp, raw bpp) of the files get_coded_ec(x_dict, rate_lambda, n_iter) writes."""
    self.eval()
    return self.model.get_coded_rate_ec(x_dict, rate_lambda=rate_lambda, n_iter=n_iter)

  def get_context_rate(self, x_dict):
    """The context-model estimate of the code's length in bits per pixel (extension), a Python float, batch
    mean: the hard-mode rate term of --lambda_rate on the eval-mode code.  Stays below get_coded_rate's coded figure."""
    self.eval()
    return self.model.get_context_rate(x_dict)

  def get_rate_map(self, x_dict):
    """Where the bits go (extension): the code length of the eval-mode code under the 4.8 coder's own adaptive
    model, exact per symbol.  dict of float64 CPU tensors: `map` [N, h, w] bits per code cell, `per_channel` [N, C] bits,
    `bits` [N], `bpp` [N] = bits / (H * W).  An ideal code length; get_coded_rate stays the size of the files."""
    self.eval()
    return self.model(x_dict, self.opt, mode='get_rate_map')

  def get_class_rates(self, x_dict):
    """The same bits attributed to the semantic classes of the pixels each code cell covers: dict(pixels, bits, bpp, share)
    with one row per class of get_eval_metrics(per_class=True) plus a last row for the pixels without a class, over the
    batch, and `per_image` with the same keys [N, rows].  bpp = bits of the class / pixels of the class, nan for an absent
    class; share = the class's fraction of the bits."""
    self.eval()
    return self.model(x_dict, self.opt, mode='get_class_rates')

  def get_vq_rate_map(self, x_dict, coder=None):
    """Where the bits of the vector-quantised code go (--encoder_quantizer s2hvq; extension): the code length of
    the eval-mode code under the adaptive model of its coder, exact per symbol.  coder: 'index' (the .jpdv model), 'plane' (the
    .jpdw model) or None (per image, the file get_coded keeps).  dict of float64 CPU tensors: `map` [N, h, w] bits per code
    cell, `per_group` [N, G], `bits` [N], `bpp` [N]; lists with one entry per image: `stream_bits` [S_n], `stream_decisions`
    (int64 [S_n]) and `coder` ('index' / 'plane').  get_rate_map stays the binarizer's call."""
    self.eval()
    return self.model.get_vq_rate_map(x_dict, coder)

  def get_vq_class_rates(self, x_dict, coder=None):
    """The same bits attributed to the semantic classes of the pixels each code cell covers: the dict of get_class_rates, row
    for row with get_eval_metrics(per_class=True) plus the last row for the pixels without a class."""
    self.eval()
    return self.model.get_vq_class_rates(x_dict, coder)

  def get_coded_semantics(self, x_dict, strip_rows=8):
    """The label and instance maps, coded losslessly on the device (extension): a list with the body of one
    .jpds file (ctu.utils.semantics) per image."""
    self.eval()
    return self.model.get_coded_semantics(x_dict, strip_rows)

  def decode_semantics(self, blobs):
    """{'label', 'instance'} on the device from the blobs get_coded_semantics returned: an x_dict for decode / decode_coded.
    A malformed blob or a label outside the label set is a ValueError."""
    self.eval()
    return self.model.decode_semantics(blobs)

  def decode_from_files(self, coded_payloads, semantics_blobs):
    """The image from bytes alone: decode_coded(coded_payloads, decode_semantics(semantics_blobs))."""
    self.eval()
    return self.model.decode_from_files(coded_payloads, semantics_blobs)

  def get_total_rate(self, x_dict, strip_rows=8):
    """(code bpp, semantics bpp, total bpp): the sizes of the .jpda and .jpds files of each image, headers included, in bits
    per pixel, batch means -- the rate of a complete stream."""
    self.eval()
    return self.model.get_total_rate(x_dict, strip_rows)

  # ---- checkpoints ------------------------------------------------------------------------------
  # File contract of the reference (pix2pixHD_trainer.py:119-176, base_model.py:54-59): <save_dir>/net_G.pth,
  # net_D.pth (state dicts) and stats_and_optim.pt with the keys below.  Optional entries are written / read only when
  # their feature is on, and a checkpoint without them still loads.
  _OPTIONAL_STATE = (('scheduler_G_state_dict', 'schedule_lr'), ('scheduler_D_state_dict', 'schedule_lr'),
                     ('lambda_distortion_weight', 'anneal_lambda'))

  def _is_writer(self):
    return not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0

  def save(self, epoch, val_loss_value):
    """Rank 0 writes (replicas are identical); the other ranks wait at a barrier so that nobody races ahead and
    reads a half-written checkpoint."""
    self.best_val_loss = val_loss_value
    if self._is_writer():
      os.makedirs(self.opt.save_dir, exist_ok=True)
      print('\nwriting checkpoint (epoch %d) to %s\n' % (epoch, self.opt.save_dir))
      record = dict(epoch=epoch, steps_taken=self.steps_taken, best_val_loss=self.best_val_loss,
                    optimizer_G_state_dict=self.optimizer_G.state_dict(),
                    optimizer_D_state_dict=self.optimizer_D.state_dict())
      for key, flag in self._OPTIONAL_STATE:
        if getattr(self.opt, flag, False):
          src = getattr(self, key[:-len('_state_dict')], None) if key.endswith('_state_dict') else getattr(self, key)
          record[key] = src.state_dict() if key.endswith('_state_dict') else src
      if self.model.netE is not None:
        record['codec_draw'] = self.model.codec_draw      # the binarizer's noise counter (extension)
      torch.save(record, os.path.join(self.opt.save_dir, 'stats_and_optim.pt'))
      self.model.save()
    if dist.is_available() and dist.is_initialized():
      dist.barrier()

  def load(self):
    path = os.path.join(self.opt.checkpoints_dir, 'stats_and_optim.pt')
    where = 'cuda:' + str(self.opt.gpu_ids[0]) if self.model.use_gpu() else 'cpu'
    record = torch.load(path, map_location=where)
    if self.mode != 'train':
      return
    self.optimizer_G.load_state_dict(record['optimizer_G_state_dict'])
    self.optimizer_D.load_state_dict(record['optimizer_D_state_dict'])
    for key, flag in self._OPTIONAL_STATE:
      if not getattr(self.opt, flag, False):
        continue
      if key not in record:
        print('checkpoint has no %s: keeping the fresh one' % key)
      elif key.endswith('_state_dict'):
        getattr(self, key[:-len('_state_dict')]).load_state_dict(record[key])
      else:
        setattr(self, key, record[key])
    self.best_val_loss = record['best_val_loss']
    self.steps_taken = record['steps_taken']
    if self.model.netE is not None:
      self.model.codec_draw = int(record.get('codec_draw', self.steps_taken))
    self.start_epoch = record['epoch'] + 1
    print('\nresumed %s: best val loss %.4f, continuing with epoch %d\n'
          % (path, self.best_val_loss, self.start_epoch + 1))
