"""The codec of the feature encoder's bottleneck, one class per quantizer: what the model's code, decode, file
and rate-term calls need from the quantizer in use -- the geometry of a code, the host checks of a code and of payloads (every
one before any device work), the eval-mode code, the receiver's half, the payloads, the sizes of the files, and the arming of
the bottleneck layer's rate term.  The model builds one object (CODECS[--encoder_quantizer]) and calls it; its input builders,
the encoder's mode and the binarizer's counters stay the model's business.

`device` arguments are callables (the model's `_device`): nothing here touches the device before the checks have passed.
A new quantizer is a new class here and its entry in CODECS."""
import contextlib

import torch

from jpdse_hip import ops
from ctu.utils import bitstream, entropy, vqdepth, vqplane, vqstages, vqstream


def check_ec_arguments(rate_lambda, n_iter):
  """float(rate_lambda) after the refusals of S2HVQ.encode_ec, which need no device."""
  from ctu.quantizers.s2h_vq import _ec_lambda, _ec_iterations
  _ec_iterations(n_iter)
  return _ec_lambda(rate_lambda)


class _Codec:

  def __init__(self, netE, cdtype):
    self.netE, self.cdtype = netE, cdtype

  def _label_geometry(self, x_dict, who):
    """(N, H, W) of the label map; ValueError for a map that is no multiple of the encoder's down-sampling factor."""
    N, H, W = int(x_dict['label'].shape[0]), int(x_dict['label'].shape[-2]), int(x_dict['label'].shape[-1])
    step = 1 << self.netE.n_downsampling
    if H % step or W % step:
      raise ValueError('%s: a %d x %d label map is no multiple of the encoder\'s down-sampling factor %d' % (who, H, W, step))
    return N, H, W

  @contextlib.contextmanager
  def rate_term(self, weight, B, H, W):
    """Arm the bottleneck layer's rate term for one training forward of B images of H x W: the layer then leaves the unscaled
    value in `rate_value` and sends the gradient, times `weight`, along with its context.  The denominator is the form's own."""
    layer = self.netE._bottleneck
    layer.rate_scale, layer.rate_denom = weight, self.rate_denom(B, H, W)
    try:
      yield
    finally:
      layer.rate_scale = None

  @property
  def rate_value(self):
    """fp32 [1] on the device: the rate term of the last armed forward, unscaled."""
    return self.netE._bottleneck.rate_value

  def depth_term(self, label):
    """The context in which the model runs the encoder, its code and the receiver's half for the device label map `label`: only
    the codec of opt.vq_class_stages arms anything (VQDepthCodec)."""
    return contextlib.nullcontext()


class BinaryCodec(_Codec):
  """The one-bit binarizer's code: an NHWC Act of +-1, exported as bits (get_code), coded as .jpda payloads."""

  RATE_OPTION = 'lambda_rate'      # the model's weight of this form's rate term

  def geometry(self, x_dict, who):
    """(N, H, W, (C, h, w), bits per image)."""
    N, H, W = self._label_geometry(x_dict, who)
    C, h, w = self.netE.code_shape(H, W)
    return N, H, W, (C, h, w), C * h * w

  def check_code(self, code, x_dict, who):
    if not torch.is_tensor(code) or code.dim() != 2 or code.dtype not in (torch.uint8, torch.float32):
      raise ValueError('%s: the code must be what get_code returns: a uint8 [N, ceil(bits / 8)] or float32 [N, bits] tensor' % who)
    geo = N, H, W, (C, h, w), bits = self.geometry(x_dict, who)
    want = (N, (bits + 7) // 8) if code.dtype == torch.uint8 else (N, bits)
    if tuple(code.shape) != want:
      raise ValueError('%s: code of shape %s, but %d label maps of %d x %d carry a %s code of shape %s (%d x %d x %d bits '
                       'per image)' % (who, tuple(code.shape), N, H, W, 'packed' if code.dtype == torch.uint8 else 'float32',
                                       want, C, h, w))
    return geo

  def check_payloads(self, payloads, x_dict, who):
    geo = self.geometry(x_dict, who)
    N, C = geo[0], geo[3][0]
    if not isinstance(payloads, (list, tuple)) or len(payloads) != N:
      raise ValueError('%s: the payloads must be what get_coded returns: a list of %d bytes objects, one per label map'
                       % (who, N))
    for j, p in enumerate(payloads):
      entropy.check_payload(p, C, '%s: payload %d' % (who, j))
    return geo

  def check_rate_lambda(self, rate_lambda, n_iter, who):
    """ValueError for a rate_lambda > 0: the entropy-constrained assignment is the vector quantizer's.  Host only."""
    if check_ec_arguments(rate_lambda, n_iter) > 0:
      raise ValueError('%s: rate_lambda > 0 (the entropy-constrained code) needs --encoder_quantizer s2hvq' % who)

  def code(self, src, rate_lambda=0.0, n_iter=2):
    """The eval-mode code of the source Act (the caller holds the encoder in eval mode).  rate_lambda is 0 here."""
    return self.netE.code(src)

  def features_of_code(self, code, geo, device, who):
    """The receiver's half as a callable: the encoder's output from a checked tensor code."""
    N, _, _, (C, h, w), _ = geo
    return lambda: self.netE.decode_code(ops.code_import(code.to(device(), non_blocking=True), N, h, w, C, self.cdtype))

  def features_of_payloads(self, payloads, geo, device, who):
    N, _, _, (C, h, w), _ = geo
    return lambda: self.netE.decode_code(ops.code_entropy_decode(list(payloads), N, h, w, C, self.cdtype, device()))

  def payloads(self, code, x_dict):
    return ops.code_entropy_encode(code)

  def file_rates(self, payloads, H, W):
    """(coded bpp, raw bpp), batch means: the .jpda file (ctu.utils.entropy: 24-byte header, and the raw payload where coding
    does not pay) and the .jpdc file (ctu.utils.bitstream: 20-byte header) of each image."""
    shape = self.netE.code_shape(H, W)
    coded = sum(8.0 * entropy.file_bytes(len(p), shape) / (H * W) for p in payloads) / len(payloads)
    return coded, 8.0 * (bitstream.HEADER_BYTES + bitstream.payload_bytes(shape)) / (H * W)

  def rate_denom(self, B, H, W):      # bits per pixel of an image, the kernel takes the batch mean
    return H * W


def _is_plane_blob(blob):
  """A .jpdw blob by its magic; anything else is the .jpdv reader's to take or to refuse."""
  return isinstance(blob, (bytes, bytearray)) and bytes(blob[:4]) == vqplane.MAGIC


class VQIndexCodec(_Codec):
  """The S2HVQ bottleneck's code: int64 [N, indices], coded as .jpdv blobs (ctu.utils.vqstream).  With
  `context_coder` (--vq_context_coder) an image's blob is its .jpdw file (ctu.utils.vqplane) where that is the
  smaller one; the receiver's half tells the two by their magic, whatever the flag."""

  RATE_OPTION = 'lambda_vq_rate'
  context_coder = False
  ec_reports = None                           # the per-image reports of the last code() with rate_lambda > 0
  COST_CODERS = (None, 'index', 'plane')      # what cost() prices: the kept file, the .jpdv model, the .jpdw model
  INDEX_STREAMS_PER_GROUP = 8                 # payloads(): (C / D) * 8 streams per .jpdv blob

  def _planes(self, H, W, groups):
    """(h, w, G) of the index planes of an H x W image."""
    n = self.netE.n_downsampling
    return H >> n, W >> n, groups

  def geometry(self, x_dict, who):
    """(N, H, W, indices per image, n_center, channel groups)."""
    N, H, W = self._label_geometry(x_dict, who)
    vq = self.netE._vq
    return N, H, W, self.netE.vq_code_len(H, W), vq.n_center, vq.cout // vq.center_size

  def check_code(self, code, x_dict, who):
    geo = N, H, W, code_len, _, _ = self.geometry(x_dict, who)
    if not torch.is_tensor(code) or code.dim() != 2 or code.dtype not in (torch.int64, torch.int32):
      raise ValueError('%s: the code must be what get_vq_code returns: an int64 [N, indices] tensor' % who)
    if tuple(code.shape) != (N, code_len):
      raise ValueError('%s: code of shape %s, but %d label maps of %d x %d carry a code of shape %s'
                       % (who, tuple(code.shape), N, H, W, (N, code_len)))
    return geo

  def check_payloads(self, blobs, x_dict, who):
    geo = N, H, W, code_len, L, groups = self.geometry(x_dict, who)
    if not isinstance(blobs, (list, tuple)) or len(blobs) != N:
      raise ValueError('%s: the blobs must be what get_coded returns: a list of %d .jpdv bytes objects, one per '
                       'label map' % (who, N))
    for j, b in enumerate(blobs):                 # every header on the host
      if _is_plane_blob(b):
        hb, wb, Gb, Lb, _, _ = vqplane.parse_blob(b, '%s: blob %d' % (who, j))
        planes = self._planes(H, W, groups)
        if Lb != L:
          raise ValueError('%s: blob %d was coded for n_center %d, the code book has %d' % (who, j, Lb, L))
        if (hb, wb, Gb) != planes:
          raise ValueError('%s: blob %d holds planes of %d x %d x %d indices, a %d x %d label map carries %d x %d x %d'
                           % ((who, j, hb, wb, Gb, H, W) + planes))
        continue
      n, cl, Lb, _, _, _ = vqstream.parse_blob(b, '%s: blob %d' % (who, j))
      if Lb != L:
        raise ValueError('%s: blob %d was coded for n_center %d, the code book has %d' % (who, j, Lb, L))
      if n * cl != code_len:
        raise ValueError('%s: blob %d holds %d x %d indices, a %d x %d label map carries %d' % (who, j, n, cl, H, W, code_len))
    return geo

  def check_rate_lambda(self, rate_lambda, n_iter, who):
    """ValueError for a rate_lambda that is negative or not finite, or an n_iter that is no int >= 0.  Host only."""
    check_ec_arguments(rate_lambda, n_iter)

  def code(self, src, rate_lambda=0.0, n_iter=2):
    """The eval-mode code of the source Act: per image the index of the nearest centre of every group of D channels, pixel by
    pixel, groups ascending inside a pixel.  rate_lambda > 0: the entropy-constrained code instead -- the
    encoder's first half runs once, then S2HVQ.encode_ec per image with groups = C / D on that image's rows of the features;
    the per-image reports stay in `ec_reports`.  rate_lambda == 0 takes exactly the path above."""
    if rate_lambda == 0:
      self.ec_reports = None
      return self.netE.vq_code(src).to(torch.int64)
    index, self.ec_reports = self.netE.vq_code_ec(src, float(rate_lambda), n_iter)
    return index.to(torch.int64)

  def features_of_code(self, code, geo, device, who):
    _, H, W, _, L, _ = geo

    def features():
      index = code.to(device(), non_blocking=True)
      if bool(((index < 0) | (index >= L)).any()):      # before the cast to int32 could fold a far value into range
        raise ValueError('%s: an index outside [0, %d)' % (who, L))
      y, _ = self.netE.decode_vq_code(index.to(torch.int32).contiguous(), H, W)
      return y

    return features

  def features_of_payloads(self, blobs, geo, device, who):
    code_len = geo[3]
    read = lambda b: vqplane.read_planes(b, device())[0] if _is_plane_blob(b) else vqstream.read_indices(b, device())
    code = torch.cat([read(bytes(b)).view(1, code_len) for b in blobs], dim=0)
    return self.features_of_code(code, geo, device, who)

  def payloads(self, code, x_dict):
    """One .jpdv blob per image in (C / D) * 8 streams: the stream count is a multiple of the group count, so a stream holds
    indices of one channel group only (write_indices clamps the count to the number of indices).  With the context coder both
    files of every image are made and the smaller one is returned, the .jpdv one on a tie: never more bytes than without."""
    _, H, W, _, L, groups = self.geometry(x_dict, 'get_coded')
    blobs = [vqstream.write_indices(None, code[i:i + 1], L, n_streams=groups * self.INDEX_STREAMS_PER_GROUP)
             for i in range(code.shape[0])]
    if self.context_coder:
      planes = [vqplane.write_planes(None, code[i], self._planes(H, W, groups), L) for i in range(code.shape[0])]
      blobs = [p if len(p) < len(b) else b for b, p in zip(blobs, planes)]
    return blobs

  def check_coder(self, coder, who):
    """ValueError for a `coder` cost() does not know.  Host only."""
    if coder not in self.COST_CODERS:
      raise ValueError('%s: coder %r, expected None (the file get_coded keeps), \'index\' (.jpdv) or \'plane\' (.jpdw)' % (who, coder))

  def cost(self, code, x_dict, label=None, n_classes=0, coder=None):
    """Where the bits of `code` (what code() returned) go, image by image: a list of N (coder, result) pairs,
    coder 'index' or 'plane' and result the dict of device tensors of ops.vq_index_cost / ops.vq_plane_cost for that image --
    cell [h * w], group [G], stream_units, stream_decisions and, with `label` (device fp32 [N, 1, H, W]) and `n_classes`, the
    class tables.
    coder 'index': the model of the .jpdv file, in the stream count payloads() uses (groups * 8, clamped as write_indices
    clamps it); 'plane': the model of the .jpdw file, in vqplane's default strip rows; None: the file get_coded keeps for the
    image -- 'index' without the context coder; with it the blobs are made as payloads() makes them and each image's magic
    decides.  A .jpdv file that fell back to packed indices (mode 0: coding did not pay) is still priced under the index
    model: the figure is that model's ideal code length, not the size of the kept file."""
    self.check_coder(coder, 'cost')
    N, H, W, code_len, L, groups = self.geometry(x_dict, 'cost')
    h, w, G = self._planes(H, W, groups)
    kept = [coder or 'index'] * N
    if coder is None and self.context_coder:
      kept = ['plane' if _is_plane_blob(b) else 'index' for b in self.payloads(code, x_dict)]
    S = vqstream.clamp_streams(groups * self.INDEX_STREAMS_PER_GROUP, code_len)
    out = []
    for i in range(N):
      index = code[i].reshape(-1).to(torch.int32).contiguous()
      lab = label[i:i + 1] if label is not None else None
      if kept[i] == 'plane':
        r = ops.vq_plane_cost(index, (h, w, G), L, vqplane.DEFAULT_STRIP_ROWS, lab, n_classes)
      else:
        r = ops.vq_index_cost(index, L, S, G, lab, n_classes, (h, w))
      out.append((kept[i], r))
    if any(int(r['status'].item()) & 2 for _, r in out):
      raise ValueError('cost: an index outside [0, %d)' % L)
    return out

  def file_rates(self, payloads, H, W):
    """(coded bpp, raw bpp), batch means: the .jpdv blobs, and the packed-index file (mode 0) of the same code: nb bits per
    index + header."""
    coded = sum(8.0 * len(p) / (H * W) for p in payloads) / len(payloads)
    raw = vqstream.HEADER_BYTES + vqstream.packed_bytes(self.netE.vq_code_len(H, W), self.netE._vq.n_center)
    return coded, 8.0 * raw / (H * W)

  def rate_denom(self, B, H, W):      # bits per pixel of the local batch
    return B * H * W


class VQStagesCodec(VQIndexCodec):
  """The residual bottleneck's code (vq_stages > 1): int64 [N, S', indices per stage], 1 <= S' <= S, coded as one
  .jpdr blob per image (ctu.utils.vqstages) that can be cut after any stage: a code or a blob of fewer stages
  than the model's is legal everywhere on the receiver's side.  The one-stage entropy-constrained assignment, the context coder
  and the cost walks are built for one stage and refused here; the multi-stage entropy-constrained code is
  code_ec, under calls of its own.  The rate term is the multi-stage one under a weight of its own,
  opt.lambda_vq_stage_rate: rate_term / rate_denom (B H W: bits per pixel of the local batch) / rate_value are VQIndexCodec's, on
  the residual layer, which sums the stages of the training forward -- under vq_train_stages = 'uniform' the drawn prefix only.
  The model picks this class; CODECS stays by quantizer."""

  RATE_OPTION = 'lambda_vq_stage_rate'
  truncate = staticmethod(vqstages.truncate_stages)      # a blob cut after n stages: host only

  def _n_stages(self):
    return self.netE.vq_stages

  def check_code(self, code, x_dict, who):
    geo = N, H, W, code_len, _, _ = self.geometry(x_dict, who)
    S = self._n_stages()
    if not torch.is_tensor(code) or code.dim() != 3 or code.dtype not in (torch.int64, torch.int32):
      raise ValueError('%s: the code must be what get_vq_code returns with vq_stages = %d: an int64 [N, stages, indices] tensor'
                       % (who, S))
    if not 1 <= int(code.shape[1]) <= S:
      raise ValueError('%s: a code of %d stages, the model (vq_stages) has 1 .. %d' % (who, int(code.shape[1]), S))
    if (int(code.shape[0]), int(code.shape[2])) != (N, code_len):
      raise ValueError('%s: code of shape %s, but %d label maps of %d x %d carry a code of shape %s'
                       % (who, tuple(code.shape), N, H, W, (N, int(code.shape[1]), code_len)))
    return geo

  def check_payloads(self, blobs, x_dict, who):
    geo = N, H, W, code_len, L, groups = self.geometry(x_dict, who)
    S = self._n_stages()
    if not isinstance(blobs, (list, tuple)) or len(blobs) != N:
      raise ValueError('%s: the blobs must be what get_coded returns: a list of %d .jpdr bytes objects, one per '
                       'label map' % (who, N))
    counts = []
    for j, b in enumerate(blobs):                 # every header on the host
      Sb, n, cl, Lb, _ = vqstages.parse_stages(b, '%s: blob %d' % (who, j))
      if Lb != L:
        raise ValueError('%s: blob %d was coded for n_center %d, the code book has %d' % (who, j, Lb, L))
      if n * cl != code_len:
        raise ValueError('%s: blob %d holds %d x %d indices per stage, a %d x %d label map carries %d'
                         % (who, j, n, cl, H, W, code_len))
      if Sb > S:
        raise ValueError('%s: blob %d holds %d stages, the model (vq_stages) has %d' % (who, j, Sb, S))
      counts.append(Sb)
    if len(set(counts)) > 1:
      raise ValueError('%s: the blobs of one call must hold the same stage count, got %s' % (who, counts))
    return geo

  def check_rate_lambda(self, rate_lambda, n_iter, who):
    if check_ec_arguments(rate_lambda, n_iter) > 0:
      raise ValueError('%s: rate_lambda > 0 (the entropy-constrained code) is built for one stage, the model has vq_stages = %d'
                       % (who, self._n_stages()))

  def check_stages(self, stages, who):
    """ValueError for a stage count outside 1 .. vq_stages.  Host only."""
    if stages is not None and (isinstance(stages, bool) or not isinstance(stages, int) or not 1 <= stages <= self._n_stages()):
      raise ValueError('%s: stages must be an int in 1 .. %d (vq_stages), got %r' % (who, self._n_stages(), stages))

  def code(self, src, rate_lambda=0.0, n_iter=2, stages=None):
    self.ec_reports = None
    return self.netE.vq_code(src, stages).to(torch.int64)

  def code_ec(self, src, rate_lambda, n_iter=2, stages=None):
    """The entropy-constrained code of the first `stages` stages: the encoder's first half once, then
    ResidualS2HVQ.encode_ec per image with groups = C / D; int64 [N, stages, indices], the per-image reports in `ec_reports`.
    rate_lambda == 0 runs the same rounds with a zero bias: code()'s indices."""
    index, self.ec_reports = self.netE.vq_stage_code_ec(src, float(rate_lambda), n_iter, stages)
    return index.to(torch.int64)

  def features_of_payloads(self, blobs, geo, device, who):
    code_len = geo[3]

    def features():
      code = torch.stack([vqstages.read_stages(bytes(b), device()).view(-1, code_len) for b in blobs], dim=0)
      return self.features_of_code(code, geo, device, who)()

    return features

  def payloads(self, code, x_dict):
    """One .jpdr blob per image, every stage a .jpdv blob in (C / D) * 8 streams as VQIndexCodec writes its one."""
    _, _, _, code_len, L, groups = self.geometry(x_dict, 'get_coded')
    return [vqstages.write_stages(None, code[i].reshape(code.shape[1], 1, code_len).contiguous(), L,
                                  n_streams=groups * self.INDEX_STREAMS_PER_GROUP) for i in range(code.shape[0])]

  def check_coder(self, coder, who):
    raise ValueError('%s: the cost walks are built for one stage, the model has vq_stages = %d' % (who, self._n_stages()))

  def cost(self, code, x_dict, label=None, n_classes=0, coder=None):
    self.check_coder(coder, 'cost')

  def file_rates(self, payloads, H, W):
    """(coded bpp, raw bpp), batch means: the .jpdr blobs, and the packed-index files of the same stages (S' times the one-stage
    packed size)."""
    coded = sum(8.0 * len(p) / (H * W) for p in payloads) / len(payloads)
    stages = vqstages.parse_stages(payloads[0], 'file_rates')[0]
    raw = vqstream.HEADER_BYTES + vqstream.packed_bytes(self.netE.vq_code_len(H, W), self.netE._vq.n_center)
    return coded, 8.0 * stages * raw / (H * W)


class VQDepthCodec(VQStagesCodec):
  """The residual bottleneck's code under opt.vq_class_stages: the stage depth of a code cell follows the classes
  of the pixels it covers, derived on both sides from the label map -- no side information.  `class_stages` = (table, default) of
  model_options.parse_vq_class_stages.  The code is VQStagesCodec's with -1 past a cell's depth, the files are .jpdm blobs
  (ctu.utils.vqdepth).  depth_term(label) arms the bottleneck layer for one call; the host checks of payloads use the numpy
  statement of the same rule on x_dict's label map, so a blob of another label map is refused before any device call."""

  class_stages = None
  _device_table = None      # (class_stages, device, int32 table on that device): made on first use, remade when either changes
  truncate = staticmethod(vqdepth.truncate_depth_stages)

  def _step(self):
    return 1 << self.netE.n_downsampling

  def device_depth(self, label):
    """int32 [N, h, w] on the device (ops.vq_depth_map)."""
    table, default = self.class_stages
    cached = self._device_table
    if cached is None or cached[0] is not self.class_stages or cached[1] != label.device:
      cached = self._device_table = (self.class_stages, label.device, torch.tensor(table, dtype=torch.int32, device=label.device))
    return ops.vq_depth_map(label, cached[2], default, self._step())

  def host_depth(self, x_dict):
    """int64 numpy [N, h, w]: the same rule on the host."""
    table, default = self.class_stages
    return vqdepth.depth_map_host(x_dict['label'], table, default, self._step())

  @contextlib.contextmanager
  def depth_term(self, label):
    layer = self.netE._bottleneck
    layer.depth = self.device_depth(label).view(-1)
    try:
      yield
    finally:
      layer.depth = None

  def check_payloads(self, blobs, x_dict, who):
    geo = N, H, W, code_len, L, groups = self.geometry(x_dict, who)
    S = self._n_stages()
    if not isinstance(blobs, (list, tuple)) or len(blobs) != N:
      raise ValueError('%s: the blobs must be what get_coded returns: a list of %d .jpdm bytes objects, one per '
                       'label map' % (who, N))
    depth = self.host_depth(x_dict)
    counts = []
    for j, b in enumerate(blobs):                 # every header, and the counts against this label map's depths, on the host
      Sb, n, cl, Lb, _, _ = vqdepth.parse_depth_stages(b, '%s: blob %d' % (who, j), depth=depth[j])
      if Lb != L:
        raise ValueError('%s: blob %d was coded for n_center %d, the code book has %d' % (who, j, Lb, L))
      if n * cl != code_len:
        raise ValueError('%s: blob %d holds %d x %d indices per stage, a %d x %d label map carries %d'
                         % (who, j, n, cl, H, W, code_len))
      if Sb > S:
        raise ValueError('%s: blob %d holds %d stages, the model (vq_stages) has %d' % (who, j, Sb, S))
      counts.append(Sb)
    if len(set(counts)) > 1:
      raise ValueError('%s: the blobs of one call must hold the same stage count, got %s' % (who, counts))
    return geo + (depth,)

  def features_of_code(self, code, geo, device, who):
    """Runs inside depth_term: the layer's depth says which indices count; -1 (or anything) past it is not read."""
    _, H, W, _, L, groups = geo[:6]

    def features():
      index = code.to(device(), non_blocking=True)
      n = int(index.shape[1])
      depth = self.netE._bottleneck.depth.view(index.shape[0], 1, -1).clamp(1, self._n_stages())
      inside = torch.arange(n, device=index.device).view(1, n, 1) < depth.repeat_interleave(groups, dim=2)
      if bool((((index < 0) | (index >= L)) & inside).any()):
        raise ValueError('%s: an index outside [0, %d) inside its cell\'s depth' % (who, L))
      y, _ = self.netE.decode_vq_code(index.clamp(-1, L).to(torch.int32).contiguous(), H, W)
      return y

    return features

  def features_of_payloads(self, blobs, geo, device, who):
    code_len, depth = geo[3], geo[6]

    def features():
      code = torch.stack([vqdepth.read_depth_stages(bytes(b), depth[j], device()).view(-1, code_len)
                          for j, b in enumerate(blobs)], dim=0)
      return self.features_of_code(code, geo, device, who)()

    return features

  def payloads(self, code, x_dict):
    """One .jpdm blob per image: stage s holds the cells with depth > s, in (C / D) * 8 streams as VQIndexCodec writes its one."""
    _, _, _, code_len, L, groups = self.geometry(x_dict, 'get_coded')
    depth = self.host_depth(x_dict)
    return [vqdepth.write_depth_stages(None, code[i].reshape(code.shape[1], 1, code_len).contiguous(), depth[i], L, groups,
                                       n_streams=groups * self.INDEX_STREAMS_PER_GROUP) for i in range(code.shape[0])]

  def file_rates(self, payloads, H, W):
    """(coded bpp, raw bpp), batch means: the .jpdm blobs, and the packed-index files of the indices they hold (nb bits each
    + one .jpdv header per non-empty stage)."""
    coded = sum(8.0 * len(p) / (H * W) for p in payloads) / len(payloads)
    raw, groups, L = 0.0, self.netE._vq.cout // self.netE._vq.center_size, self.netE._vq.n_center
    for p in payloads:
      counts = vqdepth.parse_depth_stages(p, 'file_rates')[4]
      raw += sum(vqstream.HEADER_BYTES + vqstream.packed_bytes(c * groups, L) for c in counts if c > 0)
    return coded, 8.0 * raw / len(payloads) / (H * W)


CODECS = {'binarizer': BinaryCodec, 's2hvq': VQIndexCodec}
