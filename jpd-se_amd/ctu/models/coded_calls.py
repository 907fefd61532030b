"""The coded-stream and receiver calls of Pix2PixHDModel (extensions: the reference stops at get_code / get_eval_rate): the
encoder's code in its forms, its rate figures, the entropy-coded files, the coded label and instance maps, and the receiver
that reconstructs an image from them.  DESIGN.md 4.4, 4.8 - 4.10, 4.12, 4.15 - 4.17, 4.19 and 4.20."""
import contextlib

import torch

from jpdse_hip import F32, ops
from ctu.utils import semantics as semantics_file
from ctu.models.codec import VQDepthCodec, VQIndexCodec, VQStagesCodec, check_ec_arguments


class CodedCalls(object):
  """Mixin of Pix2PixHDModel.  What it expects from the model -- six hooks:
    _device()                              the torch device, or the refusal of a run without one
    _semantics(x_dict)                     the device label and instance maps as the input builders read them
    _encoder_eval(fn)                      fn() with netE in eval mode
    preprocess(x_dict, build_base)         the NHWC device activations of a batch
    _g_input_from_vis(vis, base, N, H, W)  the generator input [semantics | vis] under --zero_sem
    netG                                   the generator
  and the attributes of its constructor: codec (ctu.models.codec, None without a bottleneck), netE, opt (normalize_mean /
  normalize_std), cdtype, n_onehot, label_nc, feat_nc, zero_vis, zero_sem, no_instance.  A bare model (tests,
  scripts/make_codec_refusals.py) that sets the hooks on the instance short-circuits them here too."""

  @staticmethod
  def _pixels(x_dict):
    """H * W of the batch's images: what a rate in bits per pixel is divided by."""
    return int(x_dict['image'].shape[-2]) * int(x_dict['image'].shape[-1])

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

  def _one_stage(self, who):
    """The refusal of a call that is built for one stage of the vector quantizer.  Host only."""
    if isinstance(self.codec, VQStagesCodec):
      raise ValueError('%s: built for one stage of the vector quantizer, this model has vq_stages = %d'
                       % (who, self.codec._n_stages()))

  def _check_stages(self, codec, stages, who):
    """`stages` of get_vq_code / get_coded_stages against the model's stage count.  Host only."""
    if isinstance(codec, VQStagesCodec):
      codec.check_stages(stages, who)
    elif isinstance(stages, bool) or stages not in (None, 1):
      raise ValueError('%s: stages = %r, this model has vq_stages = 1: None or 1' % (who, stages))

  def _eval_code(self, codec, x_dict, rate_lambda=0.0, n_iter=2, stages=None):
    """The encoder's eval-mode code of x_dict (the decoded frame with --use_compressed) in the codec's form."""
    pre = self.preprocess(x_dict, build_base=False)
    if isinstance(codec, VQStagesCodec):
      with codec.depth_term(pre['label']):      # opt.vq_class_stages: -1 past a cell's depth
        return self._encoder_eval(lambda: codec.code(pre['src'], stages=stages))
    if rate_lambda == 0:
      return self._encoder_eval(lambda: codec.code(pre['src']))
    return self._encoder_eval(lambda: codec.code(pre['src'], rate_lambda, n_iter))

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
      pixels = self._pixels(x_dict)
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
      pixels = self._pixels(x_dict)
      p_all = ((2.0 * counts[:, 0] + counts[:, 1]) / (2.0 * bits)).to(torch.float32)
      shannon, actual = 0., 0.
      for j in range(b.N):
        p = p_all[j]
        ent = - p * torch.log(p) - (1 - p) * torch.log(1 - p)
        shannon += ent * bits / pixels
        actual += bits / pixels
      return shannon / b.N, actual / b.N

  # ---- the vector-quantised code (extension) ------------------------------------------------------------------
  def get_vq_code(self, x_dict, rate_lambda=0.0, n_iter=2, stages=None):
    """The eval-mode code of the vector-quantizer bottleneck: int64 [N, h * w * C / D] on the device, per image the index of
    the nearest centre of every group of D channels, pixel by pixel, groups ascending inside a pixel.
    rate_lambda > 0: the entropy-constrained code -- every index minimises |x - c_k|^2 + rate_lambda * the
    code length of k under the histogram of its image and channel group, n_iter rounds of S2HVQ.encode_ec per image.  An
    ordinary code: decode, get_coded's files and both cost walks take it unchanged.  ValueError, before any device work, for
    a rate_lambda that is negative or not finite and an n_iter that is no int >= 0.  The defaults give today's bits.
    With vq_stages > 1: int64 [N, stages, h * w * C / D], the first `stages` (default: all) stages; every stage
    prefix code[:, :n] is a code decode takes; rate_lambda > 0 is refused.  With one stage `stages` must be None or 1."""
    codec = self._vq_codec('get_vq_code')
    codec.check_rate_lambda(rate_lambda, n_iter, 'get_vq_code')
    self._check_stages(codec, stages, 'get_vq_code')
    with torch.no_grad():
      return self._eval_code(codec, x_dict, rate_lambda, n_iter, stages)

  def get_vq_ec_report(self, x_dict, rate_lambda, n_iter=2):
    """The per-image reports of the entropy-constrained code get_vq_code(x_dict, rate_lambda, n_iter): a list of N dicts
    (distortion, bits, cost: n_iter + 1 Python floats each; S2HVQ.encode_ec).  rate_lambda == 0 runs the same rounds with a
    zero bias: every entry repeats the plain code's figures."""
    codec = self._vq_codec('get_vq_ec_report')
    self._one_stage('get_vq_ec_report')
    codec.check_rate_lambda(rate_lambda, n_iter, 'get_vq_ec_report')
    with torch.no_grad():
      pre = self.preprocess(x_dict, build_base=False)
      _, reports = self._encoder_eval(lambda: self.netE.vq_code_ec(pre['src'], float(rate_lambda), n_iter))
      return reports

  def get_vq_rate(self, x_dict):
    """The hard-mode rate term of the eval-mode code in bits per pixel of the batch, a Python float: the
    zero-order entropy of get_vq_code(x_dict) per channel group, histograms taken over the batch.  An estimate, not a size:
    get_coded_rate measures the .jpdv files, whose adaptive coder may land on either side of it."""
    self._vq_codec('get_vq_rate')
    self._one_stage('get_vq_rate')
    with torch.no_grad():
      pre = self.preprocess(x_dict, build_base=False)
      src = pre['src']
      value = self._encoder_eval(lambda: self.netE.vq_rate(src, src.N * src.H * src.W))
      return float(value.item())

  def get_vq_usage(self, x_dict):
    """int64 [G, L] on the device: how often the eval-mode code get_vq_code(x_dict) uses each of the L centres, per channel group
    (G = C / D), counted over the batch (ops.vq_rate_fwd, hard, its histogram).  A column of zeros is a dead centre: what
    fit_vq_code_book repairs.  Every row sums to the indices per group, N h w."""
    self._vq_codec('get_vq_usage')
    self._one_stage('get_vq_usage')
    with torch.no_grad():
      pre = self.preprocess(x_dict, build_base=False)
      src = pre['src']
      hist = self._encoder_eval(lambda: self.netE.vq_usage(src))
      return hist.to(torch.int64)          # sums of ones in fp32: exact while a count stays below 2^24

  def fit_vq_code_book(self, x_dicts, n_iter=10, init='sample', seed=0, reseed=True):
    """Fit the vector quantizer's code book to the encoder's own features of a list of batches: the encoder
    runs once per batch in eval mode under no_grad, the [M, D] feature matrices (fp32 or bf16 following --compute_dtype) stay on
    the device, and S2HVQ.fit runs n_iter Lloyd iterations over all of them, in place in the code book -- the optimizer and the
    gradient buckets keep their pointers.  Arguments and the returned report (distortion, dead, reseeded, counts) are
    S2HVQ.fit's.  Several ranks: the fit is deterministic and adds no collective; every rank that calls it with the same batches
    gets the same bits, so call it on every rank with the same list (or broadcast the book afterwards).
    ValueError before any device work: without --encoder_quantizer s2hvq, with --zero_vis (the encoder does not run), for an
    empty list, and for the arguments S2HVQ.fit refuses.
    With vq_stages > 1 the books are fitted stage by stage (ResidualS2HVQ.fit) and the list of per-stage reports is returned."""
    self._vq_codec('fit_vq_code_book')
    if self.zero_vis:
      raise ValueError('fit_vq_code_book: with --zero_vis the encoder does not run, there are no features to fit')
    if not isinstance(x_dicts, (list, tuple)) or len(x_dicts) == 0:
      raise ValueError('fit_vq_code_book: expected a non-empty list of batches (x_dict)')
    if isinstance(n_iter, bool) or not isinstance(n_iter, int) or n_iter < 0:
      raise ValueError('n_iter must be an int >= 0, got {!r}'.format(n_iter))
    if init not in ('sample', 'current'):
      raise ValueError("init must be 'sample' or 'current', got {!r}".format(init))
    with torch.no_grad():
      def features(x_dict):
        src = self.preprocess(x_dict, build_base=False)['src']
        return self.netE.vq_features(src)
      mats = self._encoder_eval(lambda: [features(x_dict) for x_dict in x_dicts])
      return self.netE._vq.fit(mats, n_iter=n_iter, init=init, seed=seed, reseed=reseed)

  def _decode_act(self, code, x_dict):
    """decode() up to the generator's NHWC output; also returns the device label map."""
    codec = self.codec or self._binary_codec()
    geo = codec.check_code(code, x_dict, 'decode')
    return self._generate_from_code(codec.features_of_code(code, geo, self._device, 'decode'), x_dict, *geo[:3])

  def _generate_from_code(self, features, x_dict, N, H, W):
    """The receiver's device work, shared by decode and decode_coded: features() gives the encoder's output from the code."""
    label, inst = self._semantics(x_dict)
    with self.codec.depth_term(label) if self.codec is not None else contextlib.nullcontext():
      vis = None if self.zero_vis else features()    # --zero_vis: nothing visual reaches the generator, the code is not read
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
    that is the smaller of the two.  With vq_stages > 1: a list of N .jpdr blobs (ctu.utils.vqstages) of all stages, which
    vqstages.truncate_stages cuts after any stage without the device."""
    codec = self.codec or self._binary_codec()
    with torch.no_grad():
      return codec.payloads(self._eval_code(codec, x_dict), x_dict)

  def get_coded_stages(self, x_dict, stages=None):
    """get_coded of the first `stages` stages (vq_stages > 1): the .jpdr blobs of get_vq_code(x_dict,
    stages=stages), byte for byte what vqstages.truncate_stages makes of get_coded's.  (A call of its own: the signature of
    get_coded is pinned.)  With one stage `stages` must be None or 1 and the blobs are get_coded's."""
    codec = self._vq_codec('get_coded_stages')
    self._check_stages(codec, stages, 'get_coded_stages')
    with torch.no_grad():
      return codec.payloads(self._eval_code(codec, x_dict, stages=stages), x_dict)

  # ---- the entropy-constrained code of the residual bottleneck (extension) ------------------------------------
  def _stages_codec(self, who, instead):
    """The residual bottleneck's codec, or the refusal that names the one-stage call to use.  With opt.vq_class_stages the
    entropy-constrained code and the per-stage histograms are refused (they have no depth form).  Host only."""
    codec = self._vq_codec(who)
    if isinstance(codec, VQDepthCodec):
      raise ValueError('%s: not available with opt.vq_class_stages: the entropy-constrained code and the stage histograms are '
                       'built for a uniform stage depth' % who)
    if not isinstance(codec, VQStagesCodec):
      raise ValueError('%s: a call of the residual bottleneck, this model has vq_stages = 1: use %s' % (who, instead))
    return codec

  def _stage_code_ec(self, who, instead, x_dict, rate_lambda, n_iter, stages):
    """(codec, code): the checks of the three calls below, every one before device work, then the code."""
    codec = self._stages_codec(who, instead)
    lam = check_ec_arguments(rate_lambda, n_iter)
    codec.check_stages(stages, who)
    with torch.no_grad():
      pre = self.preprocess(x_dict, build_base=False)
      return codec, self._encoder_eval(lambda: codec.code_ec(pre['src'], lam, n_iter, stages))

  def get_stage_code_ec(self, x_dict, rate_lambda, n_iter=2, stages=None):
    """The entropy-constrained code of a residual bottleneck (vq_stages > 1): int64 [N, stages, h * w * C / D],
    the first `stages` (default: all) stages.  Stage s of every vector minimises |r_s - C_s[k]|^2 + rate_lambda * the code length
    of k under the histogram of its image, stage and channel group; n_iter rounds of ResidualS2HVQ.encode_ec per image.  An
    ordinary code: decode takes it unchanged, and code[:, :n'] is get_stage_code_ec(.., stages=n').  rate_lambda == 0 gives
    get_vq_code's indices.  ValueError before any device work: a one-stage model (use get_vq_code(rate_lambda=)), a rate_lambda
    that is negative or not finite, an n_iter that is no int >= 0, stages outside 1 .. vq_stages."""
    return self._stage_code_ec('get_stage_code_ec', 'get_vq_code(rate_lambda=)', x_dict, rate_lambda, n_iter, stages)[1]

  def get_coded_stages_ec(self, x_dict, rate_lambda, n_iter=2, stages=None):
    """get_coded_stages at another point of the rate-distortion curve: one .jpdr blob per image of get_stage_code_ec(x_dict,
    rate_lambda, n_iter, stages).  decode_coded and vqstages.truncate_stages take them unchanged; a blob cut after stage n' is
    what get_coded_stages_ec(.., stages=n') writes."""
    codec, code = self._stage_code_ec('get_coded_stages_ec', 'get_coded_ec', x_dict, rate_lambda, n_iter, stages)
    return codec.payloads(code, x_dict)

  def get_stage_ec_report(self, x_dict, rate_lambda, n_iter=2, stages=None):
    """The per-image reports of get_stage_code_ec(x_dict, rate_lambda, n_iter, stages): a list of N dicts -- distortion and
    bits: n_iter + 1 rows of one Python float per stage; cost: n_iter + 1 floats (ResidualS2HVQ.encode_ec)."""
    codec, _ = self._stage_code_ec('get_stage_ec_report', 'get_vq_ec_report', x_dict, rate_lambda, n_iter, stages)
    return codec.ec_reports

  def get_stage_usage(self, x_dict):
    """int64 [S, G, L] on the device: how often stage s of the eval-mode code get_vq_code(x_dict) uses each of the L centres, per
    channel group (G = C / D), counted over the batch.  A column of zeros is a dead centre of that stage.  Every row sums to
    the indices per group, N h w."""
    self._stages_codec('get_stage_usage', 'get_vq_usage')
    with torch.no_grad():
      src = self.preprocess(x_dict, build_base=False)['src']
      return self._encoder_eval(lambda: self.netE.vq_stage_usage(src))

  def get_stage_rates(self, x_dict):
    """A list of S Python floats: entry s the zero-order entropy of stage s of get_vq_code(x_dict) per channel group, histograms
    over the batch (get_stage_usage), in bits per pixel of the batch -- what get_vq_rate is for one stage.  An estimate next
    to get_stage_curve's file sizes, not a size."""
    self._stages_codec('get_stage_rates', 'get_vq_rate')
    hist = self.get_stage_usage(x_dict).cpu().to(torch.float64)
    n = hist.sum(dim=2, keepdim=True)
    terms = torch.where(hist > 0, hist * (torch.log2(n) - torch.log2(hist.clamp(min=1.0))), torch.zeros_like(hist))
    pixels = int(x_dict['image'].shape[0]) * self._pixels(x_dict)
    return [float(v) / pixels for v in terms.sum(dim=(1, 2)).tolist()]

  def get_coded_ec(self, x_dict, rate_lambda=0.0, n_iter=2):
    """get_coded at another point of the rate-distortion curve: the blobs of get_vq_code(x_dict, rate_lambda,
    n_iter).  decode_coded takes them unchanged.  The defaults give get_coded's bytes.  (A call of its own: the signature of
    get_coded is pinned.)  ValueError, before any device work: rate_lambda > 0 without --encoder_quantizer s2hvq, and what
    get_vq_code refuses."""
    codec = self.codec or self._binary_codec()
    self._one_stage('get_coded_ec')
    codec.check_rate_lambda(rate_lambda, n_iter, 'get_coded_ec')
    with torch.no_grad():
      return codec.payloads(self._eval_code(codec, x_dict, rate_lambda, n_iter), x_dict)

  def decode_coded(self, payloads, x_dict):
    """decode() from what get_coded returned: a list of one `bytes` payload per label map.  ValueError, before any device
    work, without an encoder or a binarizer, for a label map that is no multiple of the encoder's down-sampling factor, a
    wrong payload count, an item that is not bytes, and a payload whose length table does not add up.
    With --encoder_quantizer s2hvq the items are the .jpdv blobs of get_coded; each header's n * code_len and L must fit the
    label map and the code book (checked on the host first); decode_coded(get_coded(x), x) equals get_img(x) bit for bit.
    A .jpdw blob (--vq_context_coder at the sender; told by its magic, no flag needed here) is taken in any item: its h, w, G
    and L must fit in the same way.  With vq_stages > 1 the items are .jpdr blobs of any stage count 1 .. vq_stages, the same
    in every item: a truncated stream decodes to the image of that stage prefix."""
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

  def get_coded_rate_ec(self, x_dict, rate_lambda=0.0, n_iter=2):
    """get_coded_rate of the files get_coded_ec(x_dict, rate_lambda, n_iter) writes."""
    payloads = self.get_coded_ec(x_dict, rate_lambda, n_iter)
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
    pixels = self._pixels(x_dict)
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
    return self._class_figures(units, pix, float(ops.CODE_COST_UNIT) * s * s)

  @staticmethod
  def _class_figures(units, pix, den):
    """The dict of get_class_rates from the integer class tables [N, rows] of N images; den: units per bit."""

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

  # ---- where the bits of the vector-quantised code go (extension) ----------------------------------------------
  def _vq_cost(self, who, x_dict, coder, with_label):
    """codec.cost of the eval-mode code; every refusal comes before device work."""
    codec = self._vq_codec(who)
    codec.check_coder(coder, who)
    with torch.no_grad():
      code = self._eval_code(codec, x_dict)
      label = self._semantics(x_dict)[0] if with_label else None
      return codec.cost(code, x_dict, label, self.n_onehot if with_label else 0, coder)

  def get_vq_rate_map(self, x_dict, coder=None):
    """get_rate_map for --encoder_quantizer s2hvq: the code length of the eval-mode code (the one get_vq_code / get_coded
    produce) under the adaptive model of its coder, symbol by symbol (ops.vq_index_cost / ops.vq_plane_cost).  coder: 'index'
    prices the .jpdv model, 'plane' the .jpdw model, None the file get_coded keeps for each image (VQIndexCodec.cost).  dict of
    float64 CPU tensors: `map` [N, h, w] bits per code cell, `per_group` [N, G] bits per channel group, `bits` [N], `bpp` [N] =
    bits / (H * W); `stream_bits`: a list of N tensors [S_n], `stream_decisions`: a list of N int64 tensors [S_n] (the binary
    decisions each stream coded: what the bound of DESIGN.md 4.20 is stated in), `coder`: a list of N strings, the model each
    image was priced under.  map and per_group each sum to bits.  The model's ideal length, not a file size."""
    results = self._vq_cost('get_vq_rate_map', x_dict, coder, False)
    codec = self.codec
    _, H, W, _, _, groups = codec.geometry(x_dict, 'get_vq_rate_map')
    h, w, _ = codec._planes(H, W, groups)
    unit = float(ops.CODE_COST_UNIT)
    cell = torch.stack([r['cell'] for _, r in results]).cpu().view(len(results), h, w)
    group = torch.stack([r['group'] for _, r in results]).cpu()
    bits = cell.sum(dim=(1, 2)).to(torch.float64) / unit            # integer sums first: exact
    return dict(map=cell.to(torch.float64) / unit, per_group=group.to(torch.float64) / unit, bits=bits,
                bpp=bits / self._pixels(x_dict),
                stream_bits=[r['stream_units'].cpu().to(torch.float64) / unit for _, r in results],
                stream_decisions=[r['stream_decisions'].cpu().to(torch.int64) for _, r in results],
                coder=[c for c, _ in results])

  def get_vq_class_rates(self, x_dict, coder=None):
    """get_class_rates for --encoder_quantizer s2hvq: the code length of get_vq_rate_map(x_dict, coder) attributed to the
    semantic classes of the pixels each code cell covers.  The dict of get_class_rates, same keys, same row order."""
    results = self._vq_cost('get_vq_class_rates', x_dict, coder, True)
    units = torch.stack([r['class_units'] for _, r in results]).cpu()
    pix = torch.stack([r['class_pixels'] for _, r in results]).cpu()
    s = 1 << self.netE.n_downsampling
    return self._class_figures(units, pix, float(ops.CODE_COST_UNIT) * s * s)

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
    if not self.no_instance:
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
    want = 1 if self.no_instance else 3
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
