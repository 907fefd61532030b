"""Thin tensor-level wrappers over the C ABI.

torch is used for device memory (caching allocator) and the current HIP stream only; all
arithmetic happens inside libjpdse_hip.so.  Activations travel as `Act`: an NHWC tensor
[N,H,W,CPAD(C)] (fp32 or bf16) plus its logical channel count.  What is more than a wrapper -- the host half of the three
device coders: buffer layout, payload rules, row staging, refusals -- lives in streams.py and is re-exported at the end.
"""
import ctypes

import torch

from . import (lib, check, JpdseError, F32, BF16, ConvDesc, PackEntry, InormDesc, EvalMetricsSemArgs, MsssimLossArgs, CodeRateArgs, SemLossArgs, CodeCostArgs, ACT_NONE, PAD_ZERO, PAD_REFLECT)
from . import (VqSoftFwdArgs, VqHardFwdArgs, VqSoftBwdArgs, VqDecodeArgs, VqDecodeBwdArgs, VqArgmaxArgs, VqPmfArgs, VqPmfBwdArgs,
               VqQuantizeFwdArgs, VqQuantizeBwdArgs, VqRateFwdArgs, VqQuantizeBwdGroupedArgs, VqLloydAccumArgs, VqLloydUpdateArgs,
               VqEcAssignArgs, VqEcLengthsArgs, VqResFwdArgs, VqResRowsFwdArgs, VqResDecodeArgs, VqResBwdArgs, VqResEcAssignArgs,
               VqResRateFwdArgs, VqResBwdGroupedArgs, VqResRowsFwdDepthArgs, VqResDecodeDepthArgs, VqResBwdDepthArgs, VqDepthMapArgs)
from . import VQ_RES_MAX_STAGES as _VQ_RES_MAX_STAGES


def cpad(c):
  return (c + 7) & ~7


def code_of(tdtype):
  if tdtype == torch.float32:
    return F32
  if tdtype == torch.bfloat16:
    return BF16
  raise TypeError('unsupported compute dtype %r' % (tdtype,))


def tdtype_of(code):
  return torch.bfloat16 if code == BF16 else torch.float32


def _p(t):
  return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Act(object):
  """NHWC activation: `t` has shape [N,H,W,CPAD(C)], padding lanes are zero."""
  __slots__ = ('t', 'C', 'nsums')

  def __init__(self, t, C):
    assert t.dim() == 4 and t.shape[3] == cpad(C) and t.is_contiguous(), (tuple(t.shape), C)
    self.t, self.C = t, C
    # a gradient tensor may carry the per-block sums of the InstanceNorm backward that consumes it, written by the epilogue
    # of the data-gradient kernel that produced it: (fp32 tensor [N][Cs][slots][2], slots, id of the norm's input tensor)
    self.nsums = None

  N = property(lambda s: s.t.shape[0])
  H = property(lambda s: s.t.shape[1])
  W = property(lambda s: s.t.shape[2])
  Cs = property(lambda s: s.t.shape[3])
  dtype = property(lambda s: code_of(s.t.dtype))

  def batch_slice(self, b0, b1):
    return Act(self.t[b0:b1], self.C)

  @staticmethod
  def empty(N, H, W, C, dtype_code, device):
    return Act(torch.empty((N, H, W, cpad(C)), dtype=tdtype_of(dtype_code), device=device), C)

  def empty_like(self):
    return Act(torch.empty_like(self.t), self.C)


# ---- shared workspace --------------------------------------------------------------------------
# One scratch arena per (device, stream): ops enqueued on one stream execute in order, so they may share scratch;
# a caller that runs a second torch stream (prefetch, eval overlap) gets its own arena instead of a silent race.
# Growing an arena hands the old buffer back to torch's caching allocator, which keeps it stream-ordered.
_ws = {}


def workspace(nbytes, device):
  index = device.index if device.index is not None else torch.cuda.current_device()
  key = (index, torch.cuda.current_stream(index).cuda_stream)
  cur = _ws.get(key)
  if cur is None or cur.numel() < nbytes:
    nbytes = int(nbytes * 1.25) + (1 << 20)
    cur = torch.empty(nbytes, dtype=torch.uint8, device=device)
    _ws[key] = cur
  return cur


# ---- convolution ------------------------------------------------------------------------------
def conv_desc(dtype, N, H, W, C, K, R, S, stride, pad, pad_mode, act=ACT_NONE, slope=0.2):
  return ConvDesc(dtype, N, H, W, C, K, R, S, stride, pad, pad_mode, act, slope)


def conv_out_shape(d):
  oh, ow = ctypes.c_int32(), ctypes.c_int32()
  check(lib().jpdse_conv_out_shape(ctypes.byref(d), ctypes.byref(oh), ctypes.byref(ow)), 'conv_out_shape')
  return oh.value, ow.value


def conv_pack(d, w_master, device):
  """fp32 KRSC master -> (fwd_pack, dgrad_pack) uint8 buffers in the compute dtype."""
  L = lib()
  nf, nd = L.jpdse_conv_fwd_pack_size(ctypes.byref(d)), L.jpdse_conv_dgrad_pack_size(ctypes.byref(d))
  fwd = torch.empty(nf, dtype=torch.uint8, device=device)
  dgr = torch.empty(nd, dtype=torch.uint8, device=device)
  check(L.jpdse_conv_pack_weights(ctypes.byref(d), _p(w_master), _p(fwd), _p(dgr), _stream()), 'conv_pack_weights')
  return fwd, dgr


def conv_pack_into(d, w_master, fwd, dgr):
  check(lib().jpdse_conv_pack_weights(ctypes.byref(d), _p(w_master), _p(fwd), _p(dgr), _stream()),
        'conv_pack_weights')


def conv_dgrad_pack_size(d):
  return int(lib().jpdse_conv_dgrad_pack_size(ctypes.byref(d)))


def conv_pack_entries(d, w_master, dgr):
  """The rows of a conv_pack_run table that rebuild data-gradient panel `dgr` from `w_master` (host only; block0 is the
  table builder's), or None when the library has no such rows for this layer."""
  buf = (PackEntry * 4)()
  n = lib().jpdse_conv_pack_entries(ctypes.byref(d), _p(w_master), _p(dgr), buf, 4)
  return [buf[i] for i in range(n)] if n >= 0 else None


def conv_pack_table(entries):
  """(ctypes array, (n, total blocks)): the rows of many conv_pack_entries calls as one conv_pack_run table."""
  arr, total = (PackEntry * len(entries))(*entries), 0       # copies of the layers' rows
  for e in arr:
    e.block0 = total
    total += e.blocks
  return arr, (len(entries), total)


def conv_pack_run(table, n, total_blocks):
  """One launch over a device table of n conv_pack_entries rows."""
  check(lib().jpdse_conv_pack_run(_p(table), n, total_blocks, _stream()), 'conv_pack_run')


def device_table(cache, slot, sig, build, device):
  """The argument table of a multi-tensor launch: (device tensor, *rest) for build() -> (ctypes array, rest), kept in
  cache[slot] and built and uploaded again only when `sig` (the pointers its rows hold) changes."""
  if cache.get(slot, (None,))[0] != sig:
    arr, rest = build()
    cache[slot] = (sig, torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)) + rest
  return cache[slot][1:]


def _conv_ws(d, device):
  n = lib().jpdse_conv_workspace_size(ctypes.byref(d))
  return workspace(n, device), n


def conv_fwd(d, x, fwd_pack, bias, out=None):
  oh, ow = conv_out_shape(d)
  y = out if out is not None else Act.empty(d.N, oh, ow, d.K, d.dtype, x.t.device)
  ws, n = _conv_ws(d, x.t.device)
  check(lib().jpdse_conv_fwd(ctypes.byref(d), _p(x.t), _p(fwd_pack), _p(bias), _p(y.t), _p(ws), ws.numel(), _stream()),
        'conv_fwd')
  return y


def conv_fwd_pool(d, x, fwd_pack, bias):
  """(y, MaxPool2d(2, 2)(y)) in one call (jpdse_conv_fwd_pool)."""
  oh, ow = conv_out_shape(d)
  y = Act.empty(d.N, oh, ow, d.K, d.dtype, x.t.device)
  yp = Act.empty(d.N, oh // 2, ow // 2, d.K, d.dtype, x.t.device)
  ws, n = _conv_ws(d, x.t.device)
  check(lib().jpdse_conv_fwd_pool(ctypes.byref(d), _p(x.t), _p(fwd_pack), _p(bias), _p(y.t), _p(yp.t), _p(ws), ws.numel(),
                                  _stream()), 'conv_fwd_pool')
  return y, yp


def conv_dgrad(d, dy, dgrad_pack, relu_input=None, addend=None, mask_slope=0.0):
  """relu_input: the conv's own input x when it is a ReLU output -- dx is then masked where x <= 0
  (the ReLU backward fused into the GEMM epilogue); with mask_slope != 0 x is a LeakyReLU(mask_slope) output and
  dx is scaled by the slope there instead.  addend: another gradient w.r.t. the same tensor (skip connection,
  loss tap), summed in the epilogue: dx = (dgrad + addend) * mask."""
  dx = Act.empty(d.N, d.H, d.W, d.C, d.dtype, dy.t.device)
  ws, n = _conv_ws(d, dy.t.device)
  if relu_input is not None and mask_slope != 0.0:
    check(lib().jpdse_conv_dgrad_fused_lrelu(ctypes.byref(d), _p(dy.t), _p(dgrad_pack), _p(relu_input.t), float(mask_slope),
                                             _p(addend.t if addend is not None else None), _p(dx.t), _p(ws),
                                             ws.numel(), _stream()), 'conv_dgrad_fused_lrelu')
    return dx
  if relu_input is not None or addend is not None:
    check(lib().jpdse_conv_dgrad_fused(ctypes.byref(d), _p(dy.t), _p(dgrad_pack),
                                       _p(relu_input.t if relu_input is not None else None),
                                       _p(addend.t if addend is not None else None), _p(dx.t), _p(ws),
                                       ws.numel(), _stream()), 'conv_dgrad_fused')
    return dx
  check(lib().jpdse_conv_dgrad(ctypes.byref(d), _p(dy.t), _p(dgrad_pack), _p(dx.t), _p(ws), ws.numel(), _stream()),
        'conv_dgrad')
  return dx


def conv_dgrad_batched(d, dy, dgrad_pack, alias, relu_input=None, addend=None, mask_slope=0.0):
  """conv_dgrad over d.N gradient images of which image n >= alias belongs to the saved forward image n - alias
  (jpdse_conv_dgrad_batched): relu_input holds d.N - alias images, and addend, when given, covers the first addend.N gradient
  images only.  Each image's dx is what conv_dgrad gives for it."""
  dx = Act.empty(d.N, d.H, d.W, d.C, d.dtype, dy.t.device)
  assert relu_input is None or relu_input.N == d.N - alias, (relu_input.N, d.N, alias)
  ws, n = _conv_ws(d, dy.t.device)
  check(lib().jpdse_conv_dgrad_batched(ctypes.byref(d), _p(dy.t), _p(dgrad_pack), _p(relu_input.t if relu_input is not None else None),
                                       float(mask_slope), _p(addend.t if addend is not None else None), int(alias),
                                       int(addend.N) if addend is not None else 0, _p(dx.t), _p(ws), ws.numel(), _stream()),
        'conv_dgrad_batched')
  return dx


def conv_dgrad_nsum_slots(d):
  """Blocks per image whose norm-backward sums the layer's data-gradient kernel can write (0: no such epilogue)."""
  return int(lib().jpdse_conv_dgrad_nsum_slots(ctypes.byref(d)))


def conv_dgrad_nsums(d, dy, dgrad_pack, slots, norm_x, norm_stats, norm_act, norm_slope, relu_input=None, addend=None):
  """conv_dgrad (+ mask / addend) whose dx feeds the backward of the InstanceNorm with input `norm_x` and statistics
  `norm_stats`: dx.nsums carries the per-block (sum dz, sum dz * yhat) slots for inorm_bwd (jpdse_conv_dgrad_fused_nsums)."""
  dx = Act.empty(d.N, d.H, d.W, d.C, d.dtype, dy.t.device)
  assert tuple(norm_x.t.shape) == tuple(dx.t.shape) and norm_x.dtype == dx.dtype
  sums = torch.empty((d.N, dx.Cs, slots, 2), dtype=torch.float32, device=dy.t.device)
  ws, n = _conv_ws(d, dy.t.device)
  check(lib().jpdse_conv_dgrad_fused_nsums(ctypes.byref(d), _p(dy.t), _p(dgrad_pack),
                                           _p(relu_input.t if relu_input is not None else None),
                                           _p(addend.t if addend is not None else None), _p(dx.t), _p(norm_x.t), _p(norm_stats),
                                           int(norm_act), float(norm_slope), _p(sums), _p(ws), ws.numel(), _stream()),
        'conv_dgrad_fused_nsums')
  dx.nsums = (sums, slots, norm_x.t.data_ptr())
  return dx


def conv_wgrad(d, x, dy, dw):
  """dw: fp32 tensor in the KRSC master layout, overwritten."""
  ws, n = _conv_ws(d, x.t.device)
  check(lib().jpdse_conv_wgrad(ctypes.byref(d), _p(x.t), _p(dy.t), _p(dw), _p(ws), ws.numel(), _stream()), 'conv_wgrad')


# ---- conv forward with the InstanceNorm moments fused into its epilogue -------------------------
def conv_moment_slots(d, transposed=False):
  """Blocks per image whose moments the layer's forward kernel writes (0: no such epilogue for this layer)."""
  fn = lib().jpdse_convT_moment_slots if transposed else lib().jpdse_conv_moment_slots
  return int(fn(ctypes.byref(d)))


def conv_fwd_moments(d, x, pack, slots, transposed=False):
  """y = conv(x) (no bias, no activation) and moments [N][CPAD(K)][slots][2] of y; for transposed=True `d` describes the
  underlying conv (its input is the ConvTranspose output) and `pack` is the data-gradient panel."""
  if transposed:
    y = Act.empty(d.N, d.H, d.W, d.C, d.dtype, x.t.device)
  else:
    oh, ow = conv_out_shape(d)
    y = Act.empty(d.N, oh, ow, d.K, d.dtype, x.t.device)
  mom = torch.empty((d.N, y.Cs, slots, 2), dtype=torch.float32, device=x.t.device)
  ws, n = _conv_ws(d, x.t.device)
  fn = lib().jpdse_convT_fwd_moments if transposed else lib().jpdse_conv_fwd_moments
  check(fn(ctypes.byref(d), _p(x.t), _p(pack), _p(y.t), _p(mom), _p(ws), ws.numel(), _stream()), 'conv_fwd_moments')
  return y, mom


def inorm_fwd_from_moments(x, mom, slots, act, slope=0.2, eps=1e-5, residual=None):
  d = InormDesc(x.dtype, x.N, x.H, x.W, x.C, act, slope, eps, 1 if residual is not None else 0)
  y = x.empty_like()
  stats = torch.empty((x.N, x.Cs, 2), dtype=torch.float32, device=x.t.device)
  check(lib().jpdse_inorm_fwd_from_moments(ctypes.byref(d), _p(x.t), _p(mom), slots,
                                           _p(residual.t if residual is not None else None), _p(y.t), _p(stats), _stream()),
        'inorm_fwd_from_moments')
  return y, stats


# ---- instance norm ----------------------------------------------------------------------------
def inorm_fwd(x, act, slope=0.2, eps=1e-5, residual=None):
  d = InormDesc(x.dtype, x.N, x.H, x.W, x.C, act, slope, eps, 1 if residual is not None else 0)
  y = x.empty_like()
  stats = torch.empty((x.N, x.Cs, 2), dtype=torch.float32, device=x.t.device)
  n = lib().jpdse_inorm_workspace_size(ctypes.byref(d))
  ws = workspace(n, x.t.device)
  check(lib().jpdse_inorm_fwd(ctypes.byref(d), _p(x.t), _p(residual.t if residual is not None else None), _p(y.t),
                              _p(stats), _p(ws), ws.numel(), _stream()), 'inorm_fwd')
  return y, stats


def inorm_bwd(x, stats, dy, act, slope=0.2, eps=1e-5):
  d = InormDesc(x.dtype, x.N, x.H, x.W, x.C, act, slope, eps, 0)
  dx = x.empty_like()
  n = lib().jpdse_inorm_workspace_size(ctypes.byref(d))
  ws = workspace(n, x.t.device)
  if dy.nsums is not None and dy.nsums[2] == x.t.data_ptr():
    # the sums were written by the epilogue of the kernel that produced dy, for THIS norm (same input tensor)
    sums, slots, _ = dy.nsums
    check(lib().jpdse_inorm_bwd_from_sums(ctypes.byref(d), _p(x.t), _p(stats), _p(dy.t), _p(sums), slots, _p(dx.t), _p(ws),
                                          ws.numel(), _stream()), 'inorm_bwd_from_sums')
    return dx
  check(lib().jpdse_inorm_bwd(ctypes.byref(d), _p(x.t), _p(stats), _p(dy.t), _p(dx.t), _p(ws), ws.numel(), _stream()),
        'inorm_bwd')
  return dx


def inorm_bwd_aliased(x, stats, dy, alias, act, slope=0.2, eps=1e-5):
  """inorm_bwd over dy.N gradient images of which image n >= alias belongs to the saved image n - alias of x / stats
  (jpdse_inorm_bwd with the descriptor's `alias`; x holds dy.N - alias images)."""
  assert x.N == dy.N - alias and tuple(x.t.shape[1:]) == tuple(dy.t.shape[1:]), (tuple(x.t.shape), tuple(dy.t.shape), alias)
  d = InormDesc(x.dtype, dy.N, x.H, x.W, x.C, act, slope, eps, 0, int(alias))
  dx = dy.empty_like()
  n = lib().jpdse_inorm_workspace_size(ctypes.byref(d))
  ws = workspace(n, x.t.device)
  check(lib().jpdse_inorm_bwd(ctypes.byref(d), _p(x.t), _p(stats), _p(dy.t), _p(dx.t), _p(ws), ws.numel(), _stream()),
        'inorm_bwd (aliased)')
  return dx


# ---- pooling ----------------------------------------------------------------------------------
def avgpool3s2_fwd(x):
  y = Act.empty(x.N, (x.H - 1) // 2 + 1, (x.W - 1) // 2 + 1, x.C, x.dtype, x.t.device)
  check(lib().jpdse_avgpool3s2_fwd(x.dtype, x.N, x.H, x.W, x.C, _p(x.t), _p(y.t), _stream()), 'avgpool3s2_fwd')
  return y


def avgpool3s2_bwd(dy, H, W):
  dx = Act.empty(dy.N, H, W, dy.C, dy.dtype, dy.t.device)
  check(lib().jpdse_avgpool3s2_bwd(dy.dtype, dy.N, H, W, dy.C, _p(dy.t), _p(dx.t), _stream()), 'avgpool3s2_bwd')
  return dx


def maxpool2_fwd(x):
  y = Act.empty(x.N, x.H // 2, x.W // 2, x.C, x.dtype, x.t.device)
  check(lib().jpdse_maxpool2_fwd(x.dtype, x.N, x.H, x.W, x.C, _p(x.t), _p(y.t), _stream()), 'maxpool2_fwd')
  return y


def maxpool2_bwd(x, dy):
  dx = x.empty_like()
  check(lib().jpdse_maxpool2_bwd(x.dtype, x.N, x.H, x.W, x.C, _p(x.t), _p(dy.t), _p(dx.t), _stream()), 'maxpool2_bwd')
  return dx


# ---- elementwise -------------------------------------------------------------------------------
def act_bwd(y, dy, act, slope=0.2):
  dz = y.empty_like()
  check(lib().jpdse_act_bwd(y.dtype, y.t.numel(), act, slope, _p(y.t), _p(dy.t), _p(dz.t), _stream()), 'act_bwd')
  return dz


def add(a, b):
  out = a.empty_like()
  check(lib().jpdse_add(a.dtype, a.t.numel(), _p(a.t), _p(b.t), _p(out.t), _stream()), 'add')
  return out


def add_(a, b):
  check(lib().jpdse_add(a.dtype, a.t.numel(), _p(a.t), _p(b.t), _p(a.t), _stream()), 'add')
  return a


def copy_(src, dst):
  """dst = src (contiguous device tensors of equal byte size, a multiple of 16; views of larger tensors are fine)."""
  nb = src.numel() * src.element_size()
  assert src.is_contiguous() and dst.is_contiguous() and nb == dst.numel() * dst.element_size()
  check(lib().jpdse_copy(nb, _p(src), _p(dst), _stream()), 'copy')
  return dst


def zero_(t):
  check(lib().jpdse_zero(code_of(t.dtype), t.numel(), _p(t), _stream()), 'zero')
  return t


def cast_(src, dst):
  """dst = src converted fp32 <-> bf16 (flat device tensors of equal numel, a multiple of 8)."""
  assert src.numel() == dst.numel() and src.is_contiguous() and dst.is_contiguous()
  check(lib().jpdse_cast(code_of(src.dtype), code_of(dst.dtype), src.numel(), _p(src), _p(dst), _stream()), 'cast')
  return dst


def quant_loss(a, b, mean, std, mse, out):
  """Distortion between the uint8-quantised de-normalised images a, b (Acts, fp32 or bf16 each) into the fp32
  device slot `out` (0..255 scale): tensor2im + L1Loss/MSELoss of get_eval_loss, on the device."""
  assert a.t.shape == b.t.shape and a.C == b.C and len(mean) == a.C and len(std) == a.C
  ws = workspace(lib().jpdse_quant_loss_workspace_size(), a.t.device)
  arr = ctypes.c_double * a.C
  check(lib().jpdse_quant_loss(a.dtype, b.dtype, a.N * a.H * a.W, a.C, _p(a.t), _p(b.t), arr(*[float(v) for v in mean]),
                               arr(*[float(v) for v in std]), int(bool(mse)), _p(out), _p(ws), ws.numel(), _stream()),
        'quant_loss')


def channel_sum(dy, out):
  """out: fp32 [>= CPAD(C)] device tensor; receives the per-channel sums (bias gradient)."""
  npix = dy.N * dy.H * dy.W
  n = lib().jpdse_channel_sum_workspace_size(npix, dy.C)
  ws = workspace(n, dy.t.device)
  check(lib().jpdse_channel_sum(dy.dtype, npix, dy.C, _p(dy.t), _p(out), _p(ws), ws.numel(), _stream()), 'channel_sum')


def channel_copy(src, src_c0, dst, dst_c0, nch):
  assert src.t.shape[:3] == dst.t.shape[:3]
  npix = src.N * src.H * src.W
  check(lib().jpdse_channel_copy(src.dtype, npix, _p(src.t), src.Cs, src_c0, _p(dst.t), dst.Cs, dst_c0, nch, _stream()),
        'channel_copy')


def concat_channels(base, img, c0, out):
  """out = base with channels [c0, c0 + img.C) replaced by img (both NHWC Acts of the same N,H,W)."""
  npix = base.N * base.H * base.W
  check(lib().jpdse_concat_channels(base.dtype, npix, _p(base.t), base.t.shape[-1], _p(img.t), img.t.shape[-1], c0,
                                    img.C, _p(out.t), _stream()), 'concat_channels')
  return out


def nchw_to_nhwc(src, dtype_code, out=None):
  """fp32 NCHW device tensor -> Act (into `out` when given: an Act of the same shape, e.g. a batch slice of a larger one)."""
  assert src.dtype == torch.float32 and src.is_contiguous() and src.dim() == 4
  N, C, H, W = src.shape
  if out is None:
    out = Act.empty(N, H, W, C, dtype_code, src.device)
  assert tuple(out.t.shape) == (N, H, W, cpad(C)) and out.dtype == dtype_code
  check(lib().jpdse_nchw_to_nhwc(dtype_code, N, C, H, W, _p(src), _p(out.t), _stream()), 'nchw_to_nhwc')
  return out


def nhwc_to_nchw(x):
  out = torch.empty((x.N, x.C, x.H, x.W), dtype=torch.float32, device=x.t.device)
  check(lib().jpdse_nhwc_to_nchw(x.dtype, x.N, x.C, x.H, x.W, _p(x.t), _p(out), _stream()), 'nhwc_to_nchw')
  return out


def onehot_edge(label, instance, num_labels, total_c, dtype_code):
  """label fp32 [N,1,H,W], instance int64 [N,1,H,W] -> Act with `total_c` logical channels whose
  channels [0,num_labels) are the one-hot map and channel num_labels the edge map."""
  assert label.dtype == torch.float32 and instance.dtype == torch.int64
  assert label.is_contiguous() and instance.is_contiguous()
  N, _, H, W = label.shape
  out = Act.empty(N, H, W, total_c, dtype_code, label.device)
  check(lib().jpdse_onehot_edge(dtype_code, N, H, W, num_labels, _p(label), _p(instance), _p(out.t), out.Cs, _stream()),
        'onehot_edge')
  return out


def input_builder(label, instance, num_labels, dsts, imgs, c0):
  """One pass: every Act of `dsts` (same N,H,W,C) gets one-hot(label) | edge(instance) | its image of `imgs` (Act or None)
  at channels [c0, c0 + 3).  Replaces onehot_edge + one concat_channels per destination.  Up to 64 storage channels take
  jpdse_input_builder (one kernel per width), wider destinations (more than 60 labels) jpdse_input_builder_wide."""
  assert label.dtype == torch.float32 and instance.dtype == torch.int64 and label.is_contiguous() and instance.is_contiguous()
  assert 1 <= len(dsts) <= 3 and len(imgs) == len(dsts)
  N, _, H, W = label.shape
  d0 = dsts[0]
  present = [im for im in imgs if im is not None]
  img_cs, nch = (present[0].Cs, present[0].C) if present else (8, 3)
  for d, im in zip(dsts, imgs):
    assert tuple(d.t.shape) == tuple(d0.t.shape) and d.t.shape[:3] == (N, H, W) and d.dtype == d0.dtype
    assert im is None or (im.Cs == img_cs and im.C == nch and im.dtype == d0.dtype and im.t.shape[:3] == (N, H, W))
  arr = ctypes.c_void_p * len(dsts)
  entry = lib().jpdse_input_builder if d0.Cs <= 64 else lib().jpdse_input_builder_wide
  check(entry(d0.dtype, N, H, W, num_labels, _p(label), _p(instance), len(dsts),
              arr(*[d.t.data_ptr() for d in dsts]), arr(*[(im.t.data_ptr() if im is not None else None) for im in imgs]),
              d0.Cs, img_cs, c0, nch, _stream()), 'input_builder')
  return dsts


def insert_channels(dst, img, c0):
  """dst[..., c0 : c0 + img.C] = img in place."""
  assert dst.t.shape[:3] == img.t.shape[:3] and dst.dtype == img.dtype
  npix = dst.N * dst.H * dst.W
  check(lib().jpdse_insert_channels(dst.dtype, npix, _p(dst.t), dst.Cs, _p(img.t), img.Cs, c0, img.C, _stream()), 'insert_channels')
  return dst


# ---- losses -------------------------------------------------------------------------------------
def _loss_ws(device):
  return workspace(lib().jpdse_loss_workspace_size(0), device)


# Deferred second stage of the loss reductions (jpdse_loss_finalize): inside `with deferred_loss_finals():` every loss
# forward leaves its block partials in its own region of a per-device buffer and ONE launch at the end of the block writes all
# the slots -- the train step computes 20 loss terms (pix2pixHD_pix2pixHD_model.py:205-221), each of which had its own 5-us final kernel.
_LOSS_TERMS_MAX = 64
import threading as _threading
_loss_tls = _threading.local()     # the open deferral list belongs to the thread that opened it (an eval pass on another
_loss_regions = {}                 # thread / stream must not share the training step's partial regions or its term list)


def _defer_list():
  return getattr(_loss_tls, 'defer', None)


class deferred_loss_finals(object):
  def __enter__(self):
    assert _defer_list() is None, 'deferred_loss_finals does not nest'
    _loss_tls.defer = []
    return self

  def __exit__(self, et, ev, tb):
    terms, _loss_tls.defer = _loss_tls.defer, None
    if et is None and terms:
      from . import LossTerm
      arr = (LossTerm * len(terms))()
      for i, (part, n, inv, out) in enumerate(terms):
        arr[i].partial, arr[i].n, arr[i].inv_count, arr[i].out = part, n, inv, out
      check(lib().jpdse_loss_finalize(arr, len(terms), _stream()), 'loss_finalize')
    return False


def _loss_target(out, device, work_items, count):
  """(ws tensor, out pointer or None): the shared loss workspace and the caller's slot, or -- deferred -- a private region and NULL."""
  defer = _defer_list()
  if defer is None:
    return _loss_ws(device), _p(out)
  per = lib().jpdse_loss_workspace_size(0) // 4
  index = device.index if device.index is not None else torch.cuda.current_device()
  key = (index, torch.cuda.current_stream(index).cuda_stream)       # one region buffer per (device, stream), as workspace()
  buf = _loss_regions.get(key)
  if buf is None:
    buf = _loss_regions[key] = torch.empty(_LOSS_TERMS_MAX * per, dtype=torch.float32, device=device)
  i = len(defer)
  if i >= _LOSS_TERMS_MAX:
    return _loss_ws(device), _p(out)                  # more terms than regions: this one finishes on its own
  region = buf[i * per:(i + 1) * per]
  defer.append((region.data_ptr(), int(lib().jpdse_loss_partial_count(int(work_items))), 1.0 / float(count), out.data_ptr()))
  return region, None


def _vec_items(a):
  return a.t.numel() // (4 if a.dtype == F32 else 8)


def l1_fwd(a, b, out):
  """out: fp32 device scalar slot (1-element view); mean over LOGICAL elements."""
  count = a.N * a.H * a.W * a.C
  ws, o = _loss_target(out, a.t.device, _vec_items(a), count)
  check(lib().jpdse_l1_fwd(a.dtype, a.t.numel(), count, _p(a.t), _p(b.t), o, _p(ws), ws.numel() * ws.element_size(), _stream()), 'l1_fwd')


def l1_fwd_bwd(a, b, out, scale, relu_a=False):
  """Loss value into `out` and its gradient w.r.t. a (times `scale`) in one pass; returns the gradient."""
  da = a.empty_like()
  count = a.N * a.H * a.W * a.C
  ws, o = _loss_target(out, a.t.device, _vec_items(a), count)
  check(lib().jpdse_l1_fwd_bwd(a.dtype, a.t.numel(), count, _p(a.t), _p(b.t), o, float(scale), int(relu_a),
                               _p(da.t), _p(ws), ws.numel() * ws.element_size(), _stream()), 'l1_fwd_bwd')
  return da


def l1_bwd(a, b, gout, scale, relu_a=False):
  """relu_a: `a` is a ReLU output; return the gradient w.r.t. its pre-activation."""
  da = a.empty_like()
  count = a.N * a.H * a.W * a.C
  fn = lib().jpdse_l1_bwd_relu if relu_a else lib().jpdse_l1_bwd
  check(fn(a.dtype, a.t.numel(), count, _p(a.t), _p(b.t), _p(gout), scale, _p(da.t), _stream()), 'l1_bwd')
  return da


def mse_fwd(a, b, out):
  count = a.N * a.H * a.W * a.C
  ws, o = _loss_target(out, a.t.device, _vec_items(a), count)
  check(lib().jpdse_mse_fwd(a.dtype, a.t.numel(), count, _p(a.t), _p(b.t), o, _p(ws), ws.numel() * ws.element_size(), _stream()), 'mse_fwd')


def mse_bwd(a, b, gout, scale):
  da = a.empty_like()
  count = a.N * a.H * a.W * a.C
  check(lib().jpdse_mse_bwd(a.dtype, a.t.numel(), count, _p(a.t), _p(b.t), _p(gout), scale, _p(da.t), _stream()), 'mse_bwd')
  return da


def mse_const_fwd(x, target, out):
  assert x.C == 1
  npix = x.N * x.H * x.W
  ws, o = _loss_target(out, x.t.device, npix, npix)
  check(lib().jpdse_mse_const_fwd(x.dtype, npix, x.Cs, target, _p(x.t), o, _p(ws), ws.numel() * ws.element_size(), _stream()),
        'mse_const_fwd')


def mse_const_bwd(x, target, gout, scale, out=None):
  dx = out if out is not None else x.empty_like()
  npix = x.N * x.H * x.W
  check(lib().jpdse_mse_const_bwd(x.dtype, npix, x.Cs, target, _p(x.t), _p(gout), scale, _p(dx.t), _stream()),
        'mse_const_bwd')
  return dx


# ---- learned codec (binarize.hip) ---------------------------------------------------------------
def binarize_fwd(t, train, seed=0, draw=0, n_global0=0, u=None, out=None):
  """b = stochastic sign of the tanh output `t` (train) or sign(t) (eval), same dtype / layout as t (jpdse_binarize_fwd).
  u: optional fp32 [N, C, H, W] noise replacing the Philox stream (test hook)."""
  b = out if out is not None else t.empty_like()
  if u is not None:
    assert u.dtype == torch.float32 and u.is_cuda and u.is_contiguous() and tuple(u.shape) == (t.N, t.C, t.H, t.W)
  m64 = (1 << 64) - 1
  check(lib().jpdse_binarize_fwd(t.dtype, t.N, t.H, t.W, t.C, _p(t.t), _p(b.t), 1 if train else 0, int(seed) & m64,
                                 int(draw) & m64, int(n_global0), _p(u), _stream()), 'binarize_fwd')
  return b


def code_stats(b):
  """int32 [N, 2] device tensor: per image the number of +1 and of 0 entries of the code `b` (jpdse_code_stats)."""
  L = lib()
  counts = torch.empty((b.N, 2), dtype=torch.int32, device=b.t.device)
  n = L.jpdse_code_stats_workspace_size(b.dtype, b.N, b.H, b.W, b.C)
  ws = workspace(n, b.t.device)
  check(L.jpdse_code_stats(b.dtype, b.N, b.H, b.W, b.C, _p(b.t), _p(counts), _p(ws), ws.numel(), _stream()), 'code_stats')
  return counts


def code_export(b, packed=False):
  """(b + 1) / 2 as fp32 [N, C*H*W] in NCHW flatten order, or (packed) the bits b > 0 as uint8 [N, ceil(C*H*W / 8)],
  MSB first (jpdse_code_export)."""
  bits = b.C * b.H * b.W
  if packed:
    out = torch.empty((b.N, (bits + 7) // 8), dtype=torch.uint8, device=b.t.device)
  else:
    out = torch.empty((b.N, bits), dtype=torch.float32, device=b.t.device)
  check(lib().jpdse_code_export(b.dtype, b.N, b.H, b.W, b.C, _p(b.t), 1 if packed else 0, _p(out), _stream()),
        'code_export')
  return out


def code_import(code, N, H, W, C, dtype_code, out=None):
  """The inverse of code_export (jpdse_code_import): `code` -- the uint8 bitstream [N, ceil(C*H*W / 8)], MSB first, or fp32
  [N, C*H*W] of 0 / 1 -- as the NHWC Act [N, H, W, C] of +1 / -1 the encoder's second half takes.  Never 0: an element that
  was an exact zero before export (bit 0, or 0.5 in the fp32 form) comes back as -1.  A wrong shape is a ValueError before
  any library call.  out: an Act [N, H, W, C] of that dtype to write into (every lane is written)."""
  bits = C * H * W
  packed = code.dtype == torch.uint8
  want = (N, (bits + 7) // 8) if packed else (N, bits)
  if tuple(code.shape) != want:
    raise ValueError('code_import: %s code of shape %s, expected %s for N %d, C %d, H %d, W %d'
                     % ('packed' if packed else 'fp32', tuple(code.shape), want, N, C, H, W))
  if not packed and code.dtype != torch.float32:
    raise ValueError('code_import: the code must be uint8 (packed) or float32, got %s' % (code.dtype,))
  assert code.is_cuda, 'code_import: the code must be on the device'
  code = code.contiguous()
  b = out if out is not None else Act.empty(N, H, W, C, dtype_code, code.device)
  assert (b.N, b.H, b.W, b.C, b.dtype) == (N, H, W, C, dtype_code) and b.t.device == code.device
  check(lib().jpdse_code_import(dtype_code, N, H, W, C, _p(code), 1 if packed else 0, _p(b.t), _stream()), 'code_import')
  return b


# ---- evaluation metrics (metrics.hip) ------------------------------------------------------------
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def eval_metrics_finish(raw):
  """The host half of eval_metrics: `raw` is the float64 CPU tensor [N, 14] jpdse_eval_metrics wrote (per image: |d| sum,
  d^2 sum, element count, 0, cs_1..5, ssim_1..5).  A few float64 operations per image:
    l1_i, mse_i = sums / count;  psnr_i = 10 log10(255^2 / mse_i) (inf when mse_i is 0);
    ms_ssim_i = prod_{j<5} cs_j^w_j * ssim_5^w_5, 0 when one of those five means is <= 0 (never nan).
  Returns dict(l1, mse, psnr, ms_ssim: Python floats, batch means of the per-image values; per_image: the four float64
  tensors [N]; raw: the input, part of the contract -- the per-scale means are only there).  l1 and mse are rounded exactly as jpdse_quant_loss rounds them (float32(total * (1 / count))), so
  they are bit-equal to get_eval_loss of the same batch."""
  import math
  raw = raw.to(torch.float64)
  n = raw.shape[0]
  count = raw[:, 2]
  l1_i, mse_i = raw[:, 0] / count, raw[:, 1] / count
  psnr_i = torch.tensor([10.0 * math.log10(255.0 ** 2 / m) if m > 0 else math.inf for m in mse_i.tolist()],
                        dtype=torch.float64)
  ms = []
  for row in raw.tolist():
    terms = row[4:8] + [row[13]]
    ms.append(0.0 if min(terms) <= 0.0 else math.prod(t ** w for t, w in zip(terms, MS_SSIM_WEIGHTS)))
  ms_i = torch.tensor(ms, dtype=torch.float64)
  inv = 1.0 / float(count.sum().item())
  as_f32 = lambda v: float(torch.tensor(v, dtype=torch.float64).to(torch.float32).item())
  return dict(l1=as_f32(float(raw[:, 0].sum().item()) * inv), mse=as_f32(float(raw[:, 1].sum().item()) * inv),
              psnr=float(psnr_i.mean().item()), ms_ssim=float(ms_i.mean().item()),
              per_image=dict(l1=l1_i, mse=mse_i, psnr=psnr_i, ms_ssim=ms_i), raw=raw)


def eval_metrics_per_class(cls):
  """The host half of the per-class breakdown: `cls` is the int64 CPU tensor [N, n_classes + 1, 3] jpdse_eval_metrics_sem
  wrote (per image and class: |d| sum, d^2 sum, pixels over the 3 channels; the last row = pixels without a class).  Returns
  dict(pixels int64 [n_classes], l1 / mse / psnr float64 [n_classes], unlabelled int, per_image: the same four keys
  [N, n_classes], raw: the input).  l1, mse = sum / (3 * pixels), 0 for a class that does not occur (the reference's rule,
  pix2pixHD_model.py:674-677); psnr = 10 log10(255^2 / mse): inf for an exact class, nan for an absent one.  The batch
  figures are pixel-weighted -- sums over the batch before the division, as the reference sums over dims [0, 2, 3] -- not
  means of the per-image figures."""
  cls = cls.to(torch.int64)

  def figures(t):                       # t: [..., n_classes, 3]
    pix = t[..., 2]
    den = (3 * pix).to(torch.float64)
    seen = pix > 0
    safe = torch.where(seen, den, torch.ones_like(den))
    zero = torch.zeros_like(den)
    l1 = torch.where(seen, t[..., 0].to(torch.float64) / safe, zero)
    mse = torch.where(seen, t[..., 1].to(torch.float64) / safe, zero)
    psnr = torch.where(mse > 0, 10.0 * torch.log10(255.0 ** 2 / torch.where(mse > 0, mse, torch.ones_like(mse))),
                       torch.full_like(mse, float('inf')))
    psnr = torch.where(seen, psnr, torch.full_like(mse, float('nan')))
    return dict(pixels=pix.clone(), l1=l1, mse=mse, psnr=psnr)

  r = figures(cls[:, :-1].sum(dim=0))
  r['unlabelled'] = int(cls[:, -1, 2].sum().item())
  r['per_image'] = figures(cls[:, :-1])
  r['raw'] = cls
  return r


def eval_metrics(fake, real32, mean, std, label=None, n_classes=None):
  """L1, MSE, PSNR and MS-SSIM (0..255 scale) of the uint8-quantised de-normalised images `fake` (Act, fp32 or bf16: the
  generator's output) against `real32` (Act, fp32), both 3-channel NHWC: one device pass (jpdse_eval_metrics), one
  read-back of 14 doubles per image, then eval_metrics_finish.  With `label` (device fp32 [N,1,H,W], the map
  input_builder reads) and `n_classes` the same pass also splits L1 and MSE by semantic class (jpdse_eval_metrics_sem): the
  class table rides in the same read-back and the result gains `per_class` (eval_metrics_per_class)."""
  assert fake.t.shape == real32.t.shape and fake.C == real32.C and len(mean) == fake.C and len(std) == fake.C
  L = lib()
  arr = ctypes.c_double * fake.C
  mean_c, std_c = arr(*[float(v) for v in mean]), arr(*[float(v) for v in std])
  dev = fake.t.device
  if label is None:
    if n_classes is not None:
      raise ValueError('eval_metrics: n_classes without a label map')
    n = L.jpdse_eval_metrics_workspace_size(fake.N, fake.H, fake.W, fake.C)
    ws = workspace(max(n, 1), dev)
    out = torch.empty((fake.N, 14), dtype=torch.float64, device=dev)
    check(L.jpdse_eval_metrics(fake.dtype, real32.dtype, fake.N, fake.H, fake.W, fake.C, _p(fake.t), _p(real32.t),
                               mean_c, std_c, _p(out), _p(ws), ws.numel(), _stream()), 'eval_metrics')
    return eval_metrics_finish(out.cpu())
  if n_classes is None:
    raise ValueError('eval_metrics: a label map needs n_classes')
  n_classes = int(n_classes)
  assert label.dtype == torch.float32 and label.is_contiguous() and label.device == dev
  assert tuple(label.shape) == (fake.N, 1, fake.H, fake.W)
  n = L.jpdse_eval_metrics_sem_workspace_size(fake.N, fake.H, fake.W, fake.C, n_classes)
  ws = workspace(max(n, 1), dev)
  rows = max(n_classes, 0) + 1
  both = torch.empty(fake.N * (14 + rows * 3), dtype=torch.int64, device=dev)      # out | cls: 8-byte words, ONE read-back
  out, cls = both[:fake.N * 14], both[fake.N * 14:]
  args = EvalMetricsSemArgs(fake.dtype, real32.dtype, fake.N, fake.H, fake.W, fake.C, fake.t.data_ptr(), real32.t.data_ptr(),
                            label.data_ptr(), n_classes, mean_c, std_c, out.data_ptr(), cls.data_ptr(), ws.data_ptr(),
                            ws.numel(), torch.cuda.current_stream().cuda_stream)
  check(L.jpdse_eval_metrics_sem(ctypes.byref(args)), 'eval_metrics_sem')
  host = both.cpu()
  r = eval_metrics_finish(host[:fake.N * 14].view(torch.float64).view(fake.N, 14))
  r['per_class'] = eval_metrics_per_class(host[fake.N * 14:].view(fake.N, rows, 3))
  return r


# ---- MS-SSIM training loss (msssim_loss.hip) -----------------------------------------------------
MSSSIM_MIN_SIDE = 176


def _msssim_loss(fake, real, mean, std, out, scale, stats):
  assert fake.t.shape == real.t.shape and fake.C == real.C and fake.dtype == real.dtype
  assert len(mean) == fake.C and len(std) == fake.C
  assert out.dtype == torch.float32 and out.numel() >= 1
  L = lib()
  dev = fake.t.device
  if stats is not None:
    assert stats.dtype == torch.float64 and stats.is_contiguous() and tuple(stats.shape) == (fake.N, 11) and stats.device == dev
  arr = ctypes.c_double * fake.C
  with_grad = scale is not None
  n = L.jpdse_msssim_loss_workspace_size(fake.N, fake.H, fake.W, fake.C, int(with_grad))
  ws = workspace(max(n, 1), dev)
  dfake = fake.empty_like() if with_grad else None
  args = MsssimLossArgs(fake.dtype, fake.N, fake.H, fake.W, fake.C, fake.t.data_ptr(), real.t.data_ptr(),
                        arr(*[float(v) for v in mean]), arr(*[float(v) for v in std]), out.data_ptr(),
                        stats.data_ptr() if stats is not None else None, dfake.t.data_ptr() if with_grad else None,
                        float(scale) if with_grad else 0.0, ws.data_ptr(), ws.numel(),
                        torch.cuda.current_stream().cuda_stream)
  check(L.jpdse_msssim_loss(ctypes.byref(args)), 'msssim_loss')    # an unsupported shape is refused here, before any launch
  return dfake


def msssim_loss_fwd(fake, real, mean, std, out, stats=None):
  """out (fp32 device slot) = mean_n (1 - ms_ssim_n) of the de-normalised, un-quantised images `fake` against `real` (Acts of
  one dtype, 3 channels).  The slot is written by the call itself, also inside deferred_loss_finals.
  stats: optional float64 device tensor [N, 11] that receives cs_1..5, ssim_1..5 and ms_ssim_n per image."""
  _msssim_loss(fake, real, mean, std, out, None, stats)


def msssim_loss_fwd_bwd(fake, real, mean, std, out, scale, stats=None):
  """msssim_loss_fwd and, from the same call, the Act scale * d out / d fake (fake's dtype and layout)."""
  return _msssim_loss(fake, real, mean, std, out, scale, stats)


# ---- semantics-weighted distortion (sem_loss.hip; definition: DESIGN.md 4.11) --------------------------------------------------
SEM_TABLE = 256
SEM_KINDS = {'l1': 0, 'mse': 1}


def sem_weighted_loss(fake, real, label, inst, table, edge_w, kind, out, scale=None):
  """out (fp32 device slot) = sum_p sum_c w(p) f(fake - real) / (N H W C), f = |.| (kind 'l1') or (.)^2 ('mse'), with
  w(p) = table[label(p)] * (edge_w on an instance edge, else 1) (jpdse_sem_weighted_loss).  label: float32
  [N,H,W] device map; inst: int64 [N,H,W] device map or None (no edge term); table: up to 256 host floats, the class weights
  of labels 0 .. len(table) - 1 (any other label has weight 1).  scale given: returns the Act scale * d out / d fake from the
  same pass; scale None: a value-only call, returns None.  The slot is written by the call itself, also inside
  deferred_loss_finals."""
  assert fake.t.shape == real.t.shape and fake.C == real.C and fake.dtype == real.dtype
  assert out.dtype == torch.float32 and out.numel() >= 1
  if kind not in SEM_KINDS:
    raise ValueError("sem_weighted_loss: kind must be 'l1' or 'mse', got %r" % (kind,))
  dev = fake.t.device
  shape = (fake.N, fake.H, fake.W)
  assert label.dtype == torch.float32 and label.is_contiguous() and label.numel() == fake.N * fake.H * fake.W and label.device == dev, \
      (label.dtype, tuple(label.shape), shape)
  if inst is not None:
    assert inst.dtype == torch.int64 and inst.is_contiguous() and inst.numel() == label.numel() and inst.device == dev, \
        (inst.dtype, tuple(inst.shape), shape)
  table = [float(v) for v in table]
  tab = (ctypes.c_float * max(len(table), 1))(*table)
  ws = _loss_ws(dev)
  dfake = fake.empty_like() if scale is not None else None
  args = SemLossArgs(fake.dtype, fake.N, fake.H, fake.W, fake.C, SEM_KINDS[kind], fake.t.data_ptr(), real.t.data_ptr(),
                     label.data_ptr(), inst.data_ptr() if inst is not None else None, tab, len(table), float(edge_w),
                     float(scale) if scale is not None else 0.0, out.data_ptr(), dfake.t.data_ptr() if dfake is not None else None,
                     ws.data_ptr(), ws.numel() * ws.element_size(), torch.cuda.current_stream().cuda_stream)
  check(lib().jpdse_sem_weighted_loss(ctypes.byref(args)), 'sem_weighted_loss')
  return dfake


# ---- learned codec: context-model rate term (code_rate.hip; definition: DESIGN.md 4.10) ----------------------------------
def code_rate_loss(b, t, pixels, scale=1.0, want_grad=True, want_counts=False, out=None):
  """The expected length R of the code `b` under the static context model of DESIGN.md 4.10, in bits per image pixel
  (`pixels` = the image's H*W), from one call (jpdse_code_rate_loss).  t: the Act of the tanh output behind b, or None for
  the hard mode (t := +1 where b > 0, -1 elsewhere: the conditional-entropy estimate of the code).  Returns
  (value, per_image, grad, counts): the fp32 device slot [1] holding R (unscaled; `out` when given), the fp32 per-image
  values [N], the Act scale * dR/dt in b's dtype (None unless want_grad; padding lanes 0) and the int32 counts
  [N, C, 16, 2] = (n0, n1) per stream and context (None unless want_counts)."""
  L = lib()
  dev = b.t.device
  if t is not None:
    assert t.t.shape == b.t.shape and t.C == b.C and t.dtype == b.dtype and t.t.device == dev
  if out is None:
    out = torch.empty(1, dtype=torch.float32, device=dev)
  assert out.dtype == torch.float32 and out.numel() >= 1 and out.device == dev
  per_image = torch.empty(b.N, dtype=torch.float32, device=dev)
  grad = b.empty_like() if want_grad else None
  counts = torch.empty((b.N, b.C, 16, 2), dtype=torch.int32, device=dev) if want_counts else None
  n = L.jpdse_code_rate_workspace_size(b.N, b.H, b.W, b.C)
  ws = workspace(max(n, 1), dev)
  args = CodeRateArgs(b.dtype, b.N, b.H, b.W, b.C, int(pixels), b.t.data_ptr(), t.t.data_ptr() if t is not None else None,
                      grad.t.data_ptr() if want_grad else None, float(scale), out.data_ptr(), per_image.data_ptr(),
                      counts.data_ptr() if want_counts else None, ws.data_ptr(), ws.numel(),
                      torch.cuda.current_stream().cuda_stream)
  check(L.jpdse_code_rate_loss(ctypes.byref(args)), 'code_rate_loss')    # a shape beyond the limits is refused here
  return out, per_image, grad, counts


# ---- learned codec: code-length map and per-class rate (code_cost.hip; definition: DESIGN.md 4.12) ------------------------
CODE_COST_UNIT = 65536        # units per bit


def code_cost(b, label=None, n_classes=0, want_symbols=False):
  """Where the bits of the code `b` go (jpdse_code_cost): the exact cost the adaptive model of the 4.8 coder assigns to every
  symbol, in units of 2^-16 bit, summed three ways.  Returns a dict of int64 device tensors: `cell` [N, h, w] (the rate map),
  `channel` [N, C], `symbol` [N, h, w, C] (int32; None unless want_symbols) and, with `label` (device fp32 [N, 1, H, W], H / h
  = W / w = s a power of two) and `n_classes`, `class_units` and `class_pixels` [N, n_classes + 1]: a cell's units go
  undivided to each of the s*s pixels it covers (divide by s*s for bits), the last row collects the pixels without a class
  (the rule of eval_metrics' per-class table).  Both are None without a label.  Integer sums throughout: two calls give
  identical tensors.  A shape or label map the library does not take is refused there, before any launch."""
  L = lib()
  dev = b.t.device
  N, h, w, C = b.N, b.H, b.W, b.C
  H = W = 0
  units = pixels = None
  if label is not None:
    n_classes = int(n_classes)
    assert label.dtype == torch.float32 and label.is_contiguous() and label.device == dev
    assert label.dim() == 4 and label.shape[0] == N and label.shape[1] == 1, (tuple(label.shape), N)
    H, W = int(label.shape[2]), int(label.shape[3])
    rows = max(n_classes, 0) + 1
    units = torch.empty((N, rows), dtype=torch.int64, device=dev)
    pixels = torch.empty((N, rows), dtype=torch.int64, device=dev)
  elif n_classes:
    raise ValueError('code_cost: n_classes without a label map')
  symbol = torch.empty((N, h, w, C), dtype=torch.int32, device=dev) if want_symbols else None
  cell = torch.empty((N, h, w), dtype=torch.int64, device=dev)
  channel = torch.empty((N, C), dtype=torch.int64, device=dev)
  n = L.jpdse_code_cost_workspace_size(N, h, w, C, 0)
  ws = workspace(max(n, 1), dev)
  args = CodeCostArgs(b.dtype, N, h, w, C, b.t.data_ptr(), H, W, label.data_ptr() if label is not None else None,
                      n_classes if label is not None else 0, symbol.data_ptr() if want_symbols else None, cell.data_ptr(),
                      channel.data_ptr(), units.data_ptr() if units is not None else None,
                      pixels.data_ptr() if pixels is not None else None, ws.data_ptr(), ws.numel(),
                      torch.cuda.current_stream().cuda_stream)
  check(L.jpdse_code_cost(ctypes.byref(args)), 'code_cost')
  return dict(symbol=symbol, cell=cell, channel=channel, class_units=units, class_pixels=pixels)


# ---- soft-to-hard vector quantizer (vq.hip; definition: DESIGN.md 4.13) -----------------------------------------------------
# x: [M, D] fp32 or bf16; code_book: fp32 [L, D]; p / dp / onehot / s / ds: fp32 [M, L]; index: int32 [M].  All contiguous, on one
# device.  The library refuses a shape beyond its limits (1 <= D <= 32, 2 <= L <= 512, M * L < 2^31) before any launch.
VQ_MAX_D, VQ_MAX_L = 32, 512


def _vq_dims(x, code_book):
  assert x.dim() == 2 and code_book.dim() == 2 and x.is_contiguous() and code_book.is_contiguous(), (tuple(x.shape), tuple(code_book.shape))
  assert code_book.dtype == torch.float32 and code_book.device == x.device and x.shape[1] == code_book.shape[1]
  return int(x.shape[0]), int(x.shape[1]), int(code_book.shape[0])


def _vq_rows(t, M=None, L=None):
  assert t.dim() == 2 and t.dtype == torch.float32 and t.is_contiguous(), (t.dtype, tuple(t.shape))
  assert (M is None or t.shape[0] == M) and (L is None or t.shape[1] == L), (tuple(t.shape), M, L)
  return int(t.shape[0]), int(t.shape[1])


def _vq_index(index, M, dev):
  assert index.dtype == torch.int32 and index.is_contiguous() and index.numel() == M and index.device == dev, (index.dtype, tuple(index.shape))


def _vq_ws(M, D, L, dev):
  return workspace(max(lib().jpdse_vq_workspace_size(M, D, L), 1), dev)


def vq_soft_fwd(x, code_book, sigma):
  """p[m][k] = softmax_k(-sigma d[m][k]) with d[m][k] = sum_j (x[m][j] - code_book[k][j])^2, the row minimum subtracted first
  (jpdse_vq_soft_fwd).  Returns fp32 [M, L]."""
  M, D, L = _vq_dims(x, code_book)
  p = torch.empty((M, L), dtype=torch.float32, device=x.device)
  args = VqSoftFwdArgs(code_of(x.dtype), M, D, L, float(sigma), x.data_ptr(), code_book.data_ptr(), p.data_ptr(),
                       torch.cuda.current_stream().cuda_stream)
  check(lib().jpdse_vq_soft_fwd(ctypes.byref(args)), 'vq_soft_fwd')
  return p


def vq_hard_fwd(x, code_book, want_onehot=False):
  """(index, onehot): int32 [M], the nearest centre of every vector (lowest index on a tie), and its fp32 one-hot [M, L]
  (None unless want_onehot) (jpdse_vq_hard_fwd)."""
  M, D, L = _vq_dims(x, code_book)
  index = torch.empty(M, dtype=torch.int32, device=x.device)
  onehot = torch.empty((M, L), dtype=torch.float32, device=x.device) if want_onehot else None
  args = VqHardFwdArgs(code_of(x.dtype), M, D, L, x.data_ptr(), code_book.data_ptr(), index.data_ptr(),
                       onehot.data_ptr() if want_onehot else None, torch.cuda.current_stream().cuda_stream)
  check(lib().jpdse_vq_hard_fwd(ctypes.byref(args)), 'vq_hard_fwd')
  return index, onehot


def vq_soft_bwd(dp, p, x, code_book, sigma, want_dx=True, want_dc=True):
  """(dx, dcode_book) of vq_soft_fwd for the upstream gradient dp, from the stored p (jpdse_vq_soft_bwd): dx in x's dtype
  [M, D], dcode_book fp32 [L, D]; either is None when not wanted."""
  M, D, L = _vq_dims(x, code_book)
  _vq_rows(dp, M, L)
  _vq_rows(p, M, L)
  dx = torch.empty_like(x) if want_dx else None
  dc = torch.empty_like(code_book) if want_dc else None
  ws = _vq_ws(M, D, L, x.device)
  args = VqSoftBwdArgs(code_of(x.dtype), M, D, L, float(sigma), dp.data_ptr(), p.data_ptr(), x.data_ptr(), code_book.data_ptr(),
                       dx.data_ptr() if want_dx else None, dc.data_ptr() if want_dc else None, ws.data_ptr(), ws.numel(),
                       torch.cuda.current_stream().cuda_stream)
  check(lib().jpdse_vq_soft_bwd(ctypes.byref(args)), 'vq_soft_bwd')
  return dx, dc


def vq_decode(index, code_book, dtype=torch.float32, status=None):
  """(y, status): y[m] = code_book[index[m]] in `dtype` [M, D] (jpdse_vq_decode).  An index outside [0, L) reads as centre 0 and
  sets the int32 device word `status` (a zeroed one is made when None); reading it is the caller's choice: it synchronises."""
  assert code_book.dim() == 2 and code_book.dtype == torch.float32 and code_book.is_contiguous()
  L, D = int(code_book.shape[0]), int(code_book.shape[1])
  M = int(index.numel())
  dev = code_book.device
  _vq_index(index, M, dev)
  if status is None:
    status = torch.zeros(1, dtype=torch.int32, device=dev)
  y = torch.empty((M, D), dtype=dtype, device=dev)
  args = VqDecodeArgs(code_of(dtype), M, D, L, index.data_ptr(), code_book.data_ptr(), y.data_ptr(), status.data_ptr(),
                      torch.cuda.current_stream().cuda_stream)
  check(lib().jpdse_vq_decode(ctypes.byref(args)), 'vq_decode')
  return y, status


def vq_decode_bwd(index, dy, L, status=None):
  """(dcode_book, status): dcode_book[k] = the sum of the rows dy[m] with index[m] == k, fp32 [L, D] (jpdse_vq_decode_bwd)."""
  assert dy.dim() == 2 and dy.is_contiguous()
  M, D = int(dy.shape[0]), int(dy.shape[1])
  dev = dy.device
  _vq_index(index, M, dev)
  if status is None:
    status = torch.zeros(1, dtype=torch.int32, device=dev)
  dc = torch.empty((int(L), D), dtype=torch.float32, device=dev)
  ws = _vq_ws(M, D, int(L), dev)
  args = VqDecodeBwdArgs(code_of(dy.dtype), M, D, int(L), index.data_ptr(), dy.data_ptr(), dc.data_ptr(), status.data_ptr(),
                         ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
  check(lib().jpdse_vq_decode_bwd(ctypes.byref(args)), 'vq_decode_bwd')
  return dc, status


def vq_argmax(s):
  """int32 [M]: the column of the largest entry of every row of the fp32 matrix s [M, L], lowest on a tie (jpdse_vq_argmax)."""
  M, L = _vq_rows(s)
  index = torch.empty(M, dtype=torch.int32, device=s.device)
  args = VqArgmaxArgs(M, L, s.data_ptr(), index.data_ptr(), torch.cuda.current_stream().cuda_stream)
  check(lib().jpdse_vq_argmax(ctypes.byref(args)), 'vq_argmax')
  return index


def vq_pmf(s):
  """fp32 [L]: the column means of the fp32 matrix s [M, L] (jpdse_vq_pmf)."""
  M, L = _vq_rows(s)
  pmf = torch.empty(L, dtype=torch.float32, device=s.device)
  ws = _vq_ws(M, 1, L, s.device)
  args = VqPmfArgs(M, L, s.data_ptr(), pmf.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
  check(lib().jpdse_vq_pmf(ctypes.byref(args)), 'vq_pmf')
  return pmf


def vq_pmf_bwd(dpmf, M):
  """fp32 [M, L]: ds[m][k] = dpmf[k] / M, the gradient of vq_pmf (jpdse_vq_pmf_bwd)."""
  assert dpmf.dim() == 1 and dpmf.dtype == torch.float32 and dpmf.is_contiguous()
  L = int(dpmf.numel())
  ds = torch.empty((int(M), L), dtype=torch.float32, device=dpmf.device)
  args = VqPmfBwdArgs(int(M), L, dpmf.data_ptr(), ds.data_ptr(), torch.cuda.current_stream().cuda_stream)
  check(lib().jpdse_vq_pmf_bwd(ctypes.byref(args)), 'vq_pmf_bwd')
  return ds


# ---- code-book fit (vq_fit.hip): one Lloyd iteration per pass over the vectors ----------------------------------
VQ_LLOYD_STATE = (('counts', torch.int64, False), ('sums', torch.float64, True), ('sse', torch.float64, False),
                  ('far_dist', torch.float32, False), ('far_vec', torch.float32, True))      # (name, dtype, [L, D] or [L])


def vq_lloyd_state(L, D, device):
  """The running state of one Lloyd iteration, a dict of five device tensors: counts int64 [L], sums float64
  [L, D], sse float64 [L], far_dist float32 [L], far_vec float32 [L, D].  Uninitialised: vq_lloyd_accum(first=True) fills it."""
  L, D = int(L), int(D)
  assert 1 <= D <= VQ_MAX_D and 2 <= L <= VQ_MAX_L, (L, D)
  return {name: torch.empty((L, D) if wide else (L,), dtype=dt, device=device) for name, dt, wide in VQ_LLOYD_STATE}


def _vq_lloyd_state_check(state, L, D, dev):
  assert isinstance(state, dict) and set(state) == {name for name, _, _ in VQ_LLOYD_STATE}, 'state: what vq_lloyd_state returns'
  for name, dt, wide in VQ_LLOYD_STATE:
    t = state[name]
    assert t.dtype == dt and t.is_contiguous() and tuple(t.shape) == ((L, D) if wide else (L,)) and t.device == dev, \
        (name, t.dtype, tuple(t.shape), str(t.device))


def vq_lloyd_accum(x, code_book, state, first):
  """One pass of x [M, D] (fp32 or bf16) under the fixed code_book fp32 [L, D] into `state` (jpdse_vq_lloyd_accum): per centre the
  number of vectors nearest to it (ops.vq_hard_fwd's assignment), their sum, the sum of their distances and the farthest of
  them.  first: initialise the state; otherwise add to it -- any number of batches stream through one iteration.  Returns state."""
  M, D, L = _vq_dims(x, code_book)
  assert x.dtype in (torch.float32, torch.bfloat16), x.dtype
  _vq_lloyd_state_check(state, L, D, x.device)
  ws = workspace(max(lib().jpdse_vq_lloyd_workspace_size(M, D, L), 1), x.device)
  args = VqLloydAccumArgs(code_of(x.dtype), M, D, L, 1 if first else 0, x.data_ptr(), code_book.data_ptr(),
                          state['counts'].data_ptr(), state['sums'].data_ptr(), state['sse'].data_ptr(),
                          state['far_dist'].data_ptr(), state['far_vec'].data_ptr(), ws.data_ptr(), ws.numel(),
                          torch.cuda.current_stream().cuda_stream)
  check(lib().jpdse_vq_lloyd_accum(ctypes.byref(args)), 'vq_lloyd_accum')
  return state


def vq_lloyd_update(code_book, state, reseed=True):
  """The next code book from `state`, written IN PLACE into code_book fp32 [L, D] (jpdse_vq_lloyd_update): a centre with members
  moves to their mean; with reseed the i-th centre without members takes the farthest member of the i-th donor (centres with at
  least two members and a positive farthest distance, by summed distance descending), the others stay.  Returns the int32 [2]
  device tensor (dead centres, reseeded centres)."""
  assert code_book.dim() == 2 and code_book.dtype == torch.float32 and code_book.is_contiguous(), (code_book.dtype, tuple(code_book.shape))
  L, D = int(code_book.shape[0]), int(code_book.shape[1])
  _vq_lloyd_state_check(state, L, D, code_book.device)
  report = torch.empty(2, dtype=torch.int32, device=code_book.device)
  args = VqLloydUpdateArgs(D, L, 1 if reseed else 0, code_book.data_ptr(), state['counts'].data_ptr(), state['sums'].data_ptr(),
                           state['sse'].data_ptr(), state['far_dist'].data_ptr(), state['far_vec'].data_ptr(), report.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
  check(lib().jpdse_vq_lloyd_update(ctypes.byref(args)), 'vq_lloyd_update')
  return report


# ---- vector-quantizer bottleneck (vq_bottleneck.hip): the quantizer in one call, no [M, L] matrix ------------
def _vq_quantize_ws(M, D, L, dev):
  return workspace(max(lib().jpdse_vq_quantize_workspace_size(M, D, L), 1), dev)


def vq_quantize_fwd(x, code_book, sigma, hard_forward=True, want_pmf=False):
  """(y, index, pmf) of x [M, D] against code_book fp32 [L, D] (jpdse_vq_quantize_fwd): index int32 [M] the nearest centre
  (lowest on a tie); y [M, D] in x's dtype, code_book[index] when hard_forward, else sum_k p[m][k] code_book[k] with the soft
  assignment p of vq_soft_fwd; pmf fp32 [L] = the column means of p (None unless want_pmf)."""
  M, D, L = _vq_dims(x, code_book)
  y = torch.empty_like(x)
  index = torch.empty(M, dtype=torch.int32, device=x.device)
  pmf = torch.empty(L, dtype=torch.float32, device=x.device) if want_pmf else None
  ws = _vq_quantize_ws(M, D, L, x.device) if want_pmf else None
  args = VqQuantizeFwdArgs(code_of(x.dtype), M, D, L, float(sigma), 1 if hard_forward else 0, x.data_ptr(), code_book.data_ptr(),
                           y.data_ptr(), index.data_ptr(), pmf.data_ptr() if want_pmf else None,
                           ws.data_ptr() if want_pmf else None, ws.numel() if want_pmf else 0,
                           torch.cuda.current_stream().cuda_stream)
  check(lib().jpdse_vq_quantize_fwd(ctypes.byref(args)), 'vq_quantize_fwd')
  return y, index, pmf


def vq_quantize_bwd(dy, x, code_book, sigma, dpmf=None, want_dx=True, want_dc=True, dc_out=None, groups=1, dhist=None):
  """(dx, dcode_book) of the SOFT form of vq_quantize_fwd -- the straight-through gradient of the hard one -- for the upstream
  gradients dy [M, D] (x's dtype) and, optionally, dpmf fp32 [L] (jpdse_vq_quantize_bwd; p is recomputed from x).  dx in x's
  dtype, dcode_book fp32 [L, D] (written into dc_out when given); either is None when not wanted.
  groups / dhist: with either given the call is jpdse_vq_quantize_bwd_grouped -- vector m belongs to group
  m % groups and dhist fp32 [groups, L], the gradient w.r.t. vq_rate_fwd's un-normalised sums, is added to dp at the vector's
  group; it excludes dpmf.  The defaults take exactly the call above."""
  M, D, L = _vq_dims(x, code_book)
  assert dy.shape == x.shape and dy.dtype == x.dtype and dy.is_contiguous() and dy.device == x.device, (dy.dtype, tuple(dy.shape))
  grouped = dhist is not None or int(groups) != 1
  if dpmf is not None:
    assert not grouped, 'dpmf and groups / dhist exclude each other'
    assert dpmf.dtype == torch.float32 and dpmf.is_contiguous() and dpmf.numel() == L and dpmf.device == x.device
  if dhist is not None:
    assert dhist.dtype == torch.float32 and dhist.is_contiguous() and dhist.numel() == int(groups) * L and dhist.device == x.device
  dx = torch.empty_like(x) if want_dx else None
  dc = None
  if want_dc:
    dc = dc_out if dc_out is not None else torch.empty_like(code_book)
    assert dc.dtype == torch.float32 and dc.is_contiguous() and tuple(dc.shape) == (L, D) and dc.device == x.device
  ws = _vq_quantize_ws(M, D, L, x.device) if want_dc else None
  tail = (dx.data_ptr() if want_dx else None, dc.data_ptr() if want_dc else None, ws.data_ptr() if want_dc else None,
          ws.numel() if want_dc else 0, torch.cuda.current_stream().cuda_stream)
  if grouped:
    args = VqQuantizeBwdGroupedArgs(code_of(x.dtype), M, D, L, int(groups), float(sigma), dy.data_ptr(), x.data_ptr(),
                                    code_book.data_ptr(), dhist.data_ptr() if dhist is not None else None, *tail)
    check(lib().jpdse_vq_quantize_bwd_grouped(ctypes.byref(args)), 'vq_quantize_bwd_grouped')
    return dx, dc
  args = VqQuantizeBwdArgs(code_of(x.dtype), M, D, L, float(sigma), dy.data_ptr(), x.data_ptr(), code_book.data_ptr(),
                           dpmf.data_ptr() if dpmf is not None else None, *tail)
  check(lib().jpdse_vq_quantize_bwd(ctypes.byref(args)), 'vq_quantize_bwd')
  return dx, dc


def vq_rate_fwd(x, code_book, sigma, G, denom, scale=1.0, hard=False, want_hist=False, want_grad=True):
  """(rate, hist, dhist) of the rate term on per-group histograms (jpdse_vq_rate_fwd): vector m of x [M, D]
  belongs to group m % G; hist fp32 [G, L] the sums of the soft assignment p per group (hard: of the one-hot of the nearest
  centre; None unless want_hist), rate fp32 [1] = -sum hist log2(hist / (M / G)) / denom, dhist fp32 [G, L] = scale * d rate /
  d hist (None unless want_grad): what vq_quantize_bwd(groups=G, dhist=...) takes."""
  M, D, L = _vq_dims(x, code_book)
  G = int(G)
  rate = torch.empty(1, dtype=torch.float32, device=x.device)
  hist = torch.empty((max(G, 0), L), dtype=torch.float32, device=x.device) if want_hist else None
  dhist = torch.empty((max(G, 0), L), dtype=torch.float32, device=x.device) if want_grad else None
  ws = workspace(max(lib().jpdse_vq_rate_workspace_size(M, D, L, G), 1), x.device)
  args = VqRateFwdArgs(code_of(x.dtype), M, D, L, G, float(sigma), 1 if hard else 0, x.data_ptr(), code_book.data_ptr(),
                       float(scale), float(denom), hist.data_ptr() if want_hist else None, rate.data_ptr(),
                       dhist.data_ptr() if want_grad else None, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
  check(lib().jpdse_vq_rate_fwd(ctypes.byref(args)), 'vq_rate_fwd')
  return rate, hist, dhist


# ---- entropy-constrained assignment (vq_ec.hip) -----------------------------------------------------------------
def vq_ec_assign(x, code_book, bias=None, groups=1, want_hist=True, want_sse=True):
  """(index, hist, sse) of x [M, D] against code_book fp32 [L, D] (jpdse_vq_ec_assign): index int32 [M], the arg-min over k of
  d[m][k] + bias[m % groups][k] (lowest index on equal cost; d as in vq_hard_fwd); bias fp32 [groups, L], already scaled, +inf
  for "never", None for all zero: then index is vq_hard_fwd's.  hist int32 [groups, L] the exact counts per group, sse float64
  [groups] the sum of the chosen d (without the bias) per group; either is None when not wanted."""
  M, D, L = _vq_dims(x, code_book)
  G = int(groups)
  if bias is not None:
    assert bias.dtype == torch.float32 and bias.is_contiguous() and tuple(bias.shape) == (G, L) and bias.device == x.device, \
        (bias.dtype, tuple(bias.shape))
  index = torch.empty(M, dtype=torch.int32, device=x.device)
  hist = torch.empty((max(G, 0), L), dtype=torch.int32, device=x.device) if want_hist else None
  sse = torch.empty(max(G, 0), dtype=torch.float64, device=x.device) if want_sse else None
  stats = want_hist or want_sse
  ws = workspace(max(lib().jpdse_vq_ec_workspace_size(M, D, L, G), 1), x.device) if stats else None
  args = VqEcAssignArgs(code_of(x.dtype), M, D, L, G, x.data_ptr(), code_book.data_ptr(), bias.data_ptr() if bias is not None else None,
                        index.data_ptr(), hist.data_ptr() if want_hist else None, sse.data_ptr() if want_sse else None,
                        ws.data_ptr() if stats else None, ws.numel() if stats else 0, torch.cuda.current_stream().cuda_stream)
  check(lib().jpdse_vq_ec_assign(ctypes.byref(args)), 'vq_ec_assign')
  return index, hist, sse


def vq_ec_lengths(hist, lam):
  """(bias, bits) from the counts hist int32 [G, L] (jpdse_vq_ec_lengths): bias fp32 [G, L] = lam * (log2 n[g] - log2 hist[g][k]),
  n[g] the row sum, +inf on an empty bin, exact zeros at lam == 0: what vq_ec_assign takes; bits float64 [G] = sum_k hist *
  (log2 n - log2 hist), the ideal code length of every group under its own histogram."""
  assert hist.dim() == 2 and hist.dtype == torch.int32 and hist.is_contiguous(), (hist.dtype, tuple(hist.shape))
  G, L = int(hist.shape[0]), int(hist.shape[1])
  bias = torch.empty((G, L), dtype=torch.float32, device=hist.device)
  bits = torch.empty(G, dtype=torch.float64, device=hist.device)
  args = VqEcLengthsArgs(G, L, float(lam), hist.data_ptr(), bias.data_ptr(), bits.data_ptr(), torch.cuda.current_stream().cuda_stream)
  check(lib().jpdse_vq_ec_lengths(ctypes.byref(args)), 'vq_ec_lengths')
  return bias, bits


# ---- residual quantizer (vq_residual.hip): S stages in one call -----------------------------------------------------
# books: fp32 [S, L, D], 1 <= S <= VQ_RES_MAX_STAGES; index: int32 [n_stages, M], stage-major: a stage prefix is contiguous.
VQ_RES_MAX_STAGES = _VQ_RES_MAX_STAGES


def _vq_res_dims(books, D=None):
  assert books.dim() == 3 and books.dtype == torch.float32 and books.is_contiguous(), (books.dtype, tuple(books.shape))
  S, L, Db = (int(v) for v in books.shape)
  assert D is None or D == Db, (D, Db)
  return S, L, Db


def _vq_res_stages(n_stages, S, lowest):
  n = S if n_stages is None else int(n_stages)
  if not lowest <= n <= S:
    raise ValueError('n_stages must be in %d .. %d, got %r' % (lowest, S, n_stages))
  return n


def _vq_res_ws(M, D, L, n, dev):
  return workspace(max(lib().jpdse_vq_res_workspace_size(M, D, L, max(n, 1)), 1), dev)


def _vq_res_depth(depth, groups, M, dev):
  """G of a depth call after the host checks: depth int32 [M / G] (any shape), contiguous, on `dev`."""
  G = int(groups)
  if G < 1 or M % G != 0:
    raise ValueError('groups must divide the %d vectors, got %r' % (M, groups))
  if not torch.is_tensor(depth) or depth.dtype != torch.int32 or not depth.is_contiguous() or depth.device != dev or \
      depth.numel() != M // G:
    raise ValueError('depth must be a contiguous int32 tensor of %d cells on %s, got %s' % (
        M // G, dev, (depth.dtype, tuple(depth.shape), depth.device) if torch.is_tensor(depth) else type(depth).__name__))
  return G


def vq_res_fwd(x, books, n_stages=None, want_sse=False, want_residual=False):
  """(y, index, sse, residual) of x [M, D] (fp32 or bf16) against the first n_stages (default: all) of books fp32 [S, L, D]
  (jpdse_vq_res_fwd): index int32 [n_stages, M], stage s the nearest centre of book s to the residual r_s (r_1 = x, r_{s+1} = r_s -
  books[s][index[s]], fp32, lowest index on a tie); y [M, D] in x's dtype the sum of the chosen centres (fp32, stage order, rounded
  once); sse float64 [n_stages] the summed |r_{s+1}|^2 after every stage; residual fp32 [M, D] = r_{n_stages + 1}.  sse and
  residual are None unless wanted.  n_stages = 0 is legal: y = 0, residual = x."""
  assert x.dim() == 2 and x.is_contiguous(), tuple(x.shape)
  M, D = int(x.shape[0]), int(x.shape[1])
  S, L, _ = _vq_res_dims(books, D)
  assert books.device == x.device
  n = _vq_res_stages(n_stages, S, 0)
  y = torch.empty_like(x)
  index = torch.empty((n, M), dtype=torch.int32, device=x.device)
  sse = torch.empty(n, dtype=torch.float64, device=x.device) if want_sse else None
  residual = torch.empty((M, D), dtype=torch.float32, device=x.device) if want_residual else None
  ws = _vq_res_ws(M, D, L, n, x.device) if want_sse and n > 0 else None
  args = VqResFwdArgs(code_of(x.dtype), M, D, L, S, n, x.data_ptr(), books.data_ptr(), y.data_ptr(), index.data_ptr(),
                      sse.data_ptr() if want_sse and n > 0 else None, residual.data_ptr() if want_residual else None,
                      ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0,
                      torch.cuda.current_stream().cuda_stream)
  check(lib().jpdse_vq_res_fwd(ctypes.byref(args)), 'vq_res_fwd')
  return y, index, sse, residual


def vq_res_rows_fwd(x, books, n_stages=None, depth=None, groups=1):
  """(y, index) of vq_res_fwd, bit for bit, from the thread-per-vector kernel with the residual in registers
  (jpdse_vq_res_rows_fwd): no sse, no residual, no workspace.  n_stages in 1 .. S (default: all).
  depth: int32 [M / groups], the stage depth of the cell m // groups of vector m (clamped to 1 .. S on the device):
  row m takes its first n_m = min(n_stages, depth) stages exactly as this call with n_stages = n_m would, and index[s][m] = -1 for
  s >= n_m (jpdse_vq_res_rows_fwd_depth).  The defaults take exactly the call above."""
  assert x.dim() == 2 and x.is_contiguous(), tuple(x.shape)
  M, D = int(x.shape[0]), int(x.shape[1])
  S, L, _ = _vq_res_dims(books, D)
  assert books.device == x.device
  n = _vq_res_stages(n_stages, S, 1)
  y = torch.empty_like(x)
  index = torch.empty((n, M), dtype=torch.int32, device=x.device)
  args = VqResRowsFwdArgs(code_of(x.dtype), M, D, L, S, n, x.data_ptr(), books.data_ptr(), y.data_ptr(), index.data_ptr(),
                          torch.cuda.current_stream().cuda_stream)
  if depth is not None:
    dargs = VqResRowsFwdDepthArgs(args, _vq_res_depth(depth, groups, M, x.device), depth.data_ptr())
    check(lib().jpdse_vq_res_rows_fwd_depth(ctypes.byref(dargs)), 'vq_res_rows_fwd_depth')
    return y, index
  check(lib().jpdse_vq_res_rows_fwd(ctypes.byref(args)), 'vq_res_rows_fwd')
  return y, index


def vq_res_decode(index, books, n_stages=None, dtype=torch.float32, status=None, depth=None, groups=1):
  """(y, status): y[m] = books[0][index[0][m]] + .. over the first n_stages (default: all the rows of index) in `dtype` [M, D],
  bit for bit the y of vq_res_fwd with the same n_stages (jpdse_vq_res_decode).  index int32 [S', M].  An index outside [0, L)
  reads as centre 0 and sets the int32 device word `status` (a zeroed one is made when None): the rule of vq_decode.
  depth / groups: row m sums its first min(n_stages, depth[m // groups]) centres, the y of vq_res_rows_fwd with
  the same depth; index[s][m] past the row's depth is never read (jpdse_vq_res_decode_depth)."""
  S, L, D = _vq_res_dims(books)
  assert index.dim() == 2 and index.dtype == torch.int32 and index.is_contiguous() and index.device == books.device, \
      (index.dtype, tuple(index.shape))
  rows, M = int(index.shape[0]), int(index.shape[1])
  assert rows <= S, (rows, S)
  n = _vq_res_stages(n_stages, rows, 1)
  if status is None:
    status = torch.zeros(1, dtype=torch.int32, device=books.device)
  y = torch.empty((M, D), dtype=dtype, device=books.device)
  args = VqResDecodeArgs(code_of(dtype), M, D, L, S, n, index.data_ptr(), books.data_ptr(), y.data_ptr(), status.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
  if depth is not None:
    dargs = VqResDecodeDepthArgs(args, _vq_res_depth(depth, groups, M, books.device), depth.data_ptr())
    check(lib().jpdse_vq_res_decode_depth(ctypes.byref(dargs)), 'vq_res_decode_depth')
    return y, status
  check(lib().jpdse_vq_res_decode(ctypes.byref(args)), 'vq_res_decode')
  return y, status


def vq_res_bwd(dy, x, books, index, sigma, want_dx=True, want_dc=True, dc_out=None, groups=1, dhist=None, depth=None):
  """(dx, dbooks) of the SOFT form of every stage of vq_res_fwd -- the straight-through gradient -- for the upstream gradient dy
  [M, D] (x's dtype) (jpdse_vq_res_bwd; the residuals are recomputed from x and index int32 [S', M]).  dx in x's dtype; dbooks
  fp32 [S, L, D] (written into dc_out when given), zero for the books beyond S'; either is None when not wanted.
  groups / dhist: with either given the call is jpdse_vq_res_bwd_grouped -- vector m belongs to group m % groups
  and dhist fp32 [S', groups, L], the gradient w.r.t. vq_res_rate_fwd's un-normalised sums, is added to dp of stage s at the
  vector's group.  The defaults take exactly the call above.
  depth: int32 [M / groups]; the call is jpdse_vq_res_bwd_depth -- `groups` is then the number of vectors of a
  cell, vector m belongs to cell m // groups, and row m runs the recursion over its first min(S', depth) stages (index[s][m]
  beyond is not read); dbooks of a stage sums over the rows that reach it.  Not together with dhist."""
  assert x.dim() == 2 and x.is_contiguous(), tuple(x.shape)
  M, D = int(x.shape[0]), int(x.shape[1])
  S, L, _ = _vq_res_dims(books, D)
  assert dy.shape == x.shape and dy.dtype == x.dtype and dy.is_contiguous() and dy.device == x.device, (dy.dtype, tuple(dy.shape))
  assert index.dim() == 2 and index.dtype == torch.int32 and index.is_contiguous() and index.device == x.device and \
      int(index.shape[1]) == M and 1 <= int(index.shape[0]) <= S, (index.dtype, tuple(index.shape))
  n = int(index.shape[0])
  dx = torch.empty_like(x) if want_dx else None
  dc = None
  if want_dc:
    dc = dc_out if dc_out is not None else torch.empty_like(books)
    assert dc.dtype == torch.float32 and dc.is_contiguous() and tuple(dc.shape) == (S, L, D) and dc.device == x.device
    if n < S:
      dc[n:].zero_()
  ws = _vq_res_ws(M, D, L, n, x.device) if want_dc else None
  args = VqResBwdArgs(code_of(x.dtype), M, D, L, S, n, float(sigma), dy.data_ptr(), x.data_ptr(), books.data_ptr(), index.data_ptr(),
                      dx.data_ptr() if want_dx else None, dc.data_ptr() if want_dc else None, ws.data_ptr() if want_dc else None,
                      ws.numel() if want_dc else 0, torch.cuda.current_stream().cuda_stream)
  if depth is not None:
    if dhist is not None:
      raise ValueError('vq_res_bwd: depth and dhist cannot be combined (the rate term has no depth form)')
    dargs = VqResBwdDepthArgs(args, _vq_res_depth(depth, groups, M, x.device), depth.data_ptr())
    check(lib().jpdse_vq_res_bwd_depth(ctypes.byref(dargs)), 'vq_res_bwd_depth')
    return dx, dc
  if dhist is not None or int(groups) != 1:
    G = int(groups)
    if dhist is not None:
      assert dhist.dtype == torch.float32 and dhist.is_contiguous() and tuple(dhist.shape) == (n, G, L) and dhist.device == x.device, \
          (dhist.dtype, tuple(dhist.shape))
    gargs = VqResBwdGroupedArgs(args, G, dhist.data_ptr() if dhist is not None else None)
    check(lib().jpdse_vq_res_bwd_grouped(ctypes.byref(gargs)), 'vq_res_bwd_grouped')
    return dx, dc
  check(lib().jpdse_vq_res_bwd(ctypes.byref(args)), 'vq_res_bwd')
  return dx, dc


def vq_depth_map(label, table, default_depth, step):
  """int32 [N, H / step, W / step]: the stage depth of every cell of step x step pixels of label fp32 [N, 1, H, W] (DESIGN.md
  4.27; jpdse_vq_depth_map): the maximum over the cell's pixels of table[class] (table int32 [n_classes] on the device, may be
  empty), a pixel whose label is no integer in [0, n_classes) taking default_depth."""
  assert label.dim() == 4 and label.size(1) == 1 and label.dtype == torch.float32 and label.is_contiguous(), \
      (label.dtype, tuple(label.shape))
  N, H, W, step = int(label.size(0)), int(label.size(2)), int(label.size(3)), int(step)
  assert table.dim() == 1 and table.dtype == torch.int32 and table.is_contiguous() and table.device == label.device, \
      (table.dtype, tuple(table.shape))
  if step < 1 or H % step or W % step:
    raise ValueError('step must divide H = %d and W = %d, got %r' % (H, W, step))
  out = torch.empty((N, H // step, W // step), dtype=torch.int32, device=label.device)
  args = VqDepthMapArgs(N, H, W, step, int(table.numel()), int(default_depth), label.data_ptr(),
                        table.data_ptr() if table.numel() else None, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
  check(lib().jpdse_vq_depth_map(ctypes.byref(args)), 'vq_depth_map')
  return out


def vq_res_rate_fwd(x, books, sigma, G, denom, scale=1.0, n_stages=None, want_code=False, want_hist=False, want_grad=True):
  """(rate, rates, hist, dhist, y, index) of the rate term of the residual quantizer (jpdse_vq_res_rate_fwd) over
  the first n_stages (default: all) of books fp32 [S, L, D]: vector m of x [M, D] belongs to group m % G; hist fp32 [n_stages, G, L]
  the per-group sums of the soft assignment of every stage's residual r_s (the hard chain of vq_res_rows_fwd; None unless
  want_hist); rates fp32 [n_stages], rates[s] = -sum hist[s] log2(hist[s] / (M / G)) / denom; rate fp32 [1] their sum in stage
  order; dhist fp32 [n_stages, G, L] = scale * d rate / d hist (None unless want_grad): what vq_res_bwd(groups=G, dhist=...) takes.
  want_code: y [M, D] and index int32 [n_stages, M] of vq_res_rows_fwd, bit for bit, from the same kernel (else None)."""
  assert x.dim() == 2 and x.is_contiguous(), tuple(x.shape)
  M, D = int(x.shape[0]), int(x.shape[1])
  S, L, _ = _vq_res_dims(books, D)
  assert books.device == x.device
  n = _vq_res_stages(n_stages, S, 1)
  G = int(G)
  dev = x.device
  rate = torch.empty(1, dtype=torch.float32, device=dev)
  rates = torch.empty(n, dtype=torch.float32, device=dev)
  hist = torch.empty((n, max(G, 0), L), dtype=torch.float32, device=dev) if want_hist else None
  dhist = torch.empty((n, max(G, 0), L), dtype=torch.float32, device=dev) if want_grad else None
  y = torch.empty_like(x) if want_code else None
  index = torch.empty((n, M), dtype=torch.int32, device=dev) if want_code else None
  ws = workspace(max(lib().jpdse_vq_res_rate_workspace_size(M, D, L, G, n), 1), dev)
  args = VqResRateFwdArgs(code_of(x.dtype), M, D, L, S, n, G, float(sigma), float(scale), float(denom), x.data_ptr(), books.data_ptr(),
                          rate.data_ptr(), rates.data_ptr(), hist.data_ptr() if want_hist else None,
                          dhist.data_ptr() if want_grad else None, y.data_ptr() if want_code else None,
                          index.data_ptr() if want_code else None, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
  check(lib().jpdse_vq_res_rate_fwd(ctypes.byref(args)), 'vq_res_rate_fwd')
  return rate, rates, hist, dhist, y, index


def vq_res_ec_assign(x, books, bias=None, groups=1, n_stages=None, want_y=True, want_stats=True):
  """(y, index, hist, sse): the entropy-constrained code of x [M, D] (fp32 or bf16) under the first n_stages (default: all) of books
  fp32 [S, L, D] (jpdse_vq_res_ec_assign).  Stage s takes the arg-min over k of d(r_s, books[s][k]) + bias[s][m %
  groups][k] (lowest index on equal cost, +inf for "never", a row of +inf alone gives 0); bias fp32 [n_stages, groups, L], already
  scaled, None for all zero: then index and y are vq_res_rows_fwd's bit for bit.  index int32 [n_stages, M]; y [M, D] in x's dtype
  the sum of the chosen centres, None unless want_y; hist int32 [n_stages, groups, L] the exact counts per stage and group and sse
  float64 [n_stages, groups] the summed chosen d without the bias (the squared error after that stage), None unless want_stats."""
  assert x.dim() == 2 and x.is_contiguous(), tuple(x.shape)
  M, D = int(x.shape[0]), int(x.shape[1])
  S, L, _ = _vq_res_dims(books, D)
  assert books.device == x.device
  n = _vq_res_stages(n_stages, S, 1)
  G = int(groups)
  if bias is not None:
    assert bias.dtype == torch.float32 and bias.is_contiguous() and tuple(bias.shape) == (n, G, L) and bias.device == x.device, \
        (bias.dtype, tuple(bias.shape))
  y = torch.empty_like(x) if want_y else None
  index = torch.empty((n, M), dtype=torch.int32, device=x.device)
  hist = torch.empty((n, max(G, 0), L), dtype=torch.int32, device=x.device) if want_stats else None
  sse = torch.empty((n, max(G, 0)), dtype=torch.float64, device=x.device) if want_stats else None
  ws = workspace(max(lib().jpdse_vq_res_ec_workspace_size(M, D, L, G, n), 1), x.device) if want_stats else None
  args = VqResEcAssignArgs(code_of(x.dtype), M, D, L, S, n, G, x.data_ptr(), books.data_ptr(),
                           bias.data_ptr() if bias is not None else None, y.data_ptr() if want_y else None, index.data_ptr(),
                           hist.data_ptr() if want_stats else None, sse.data_ptr() if want_stats else None,
                           ws.data_ptr() if want_stats else None, ws.numel() if want_stats else 0,
                           torch.cuda.current_stream().cuda_stream)
  check(lib().jpdse_vq_res_ec_assign(ctypes.byref(args)), 'vq_res_ec_assign')
  return y, index, hist, sse


# ---- the host half of the three device coders (streams.py) -----------------------------------------------------
# Re-exported here, where their callers look for them.  At the end, as is the import at the end of streams: whichever of the two
# modules is imported first finds, half-way through its own import, every name of the other that it asks for.
from .streams import (code_entropy_encode, code_entropy_decode, length_table_size, check_length_table,  # noqa: E402,F401
                      SEM_RAW, SEM_CODED, SEM_RAW_BYTES, semantics_strips, semantics_encode, semantics_check_entry, semantics_decode,
                      VQ_INDEX_MAX_S, vq_index_bits, vq_index_encode, vq_index_decode,
                      vq_plane_streams, vq_plane_capacity, vq_plane_shape, vq_plane_encode, vq_plane_decode,
                      vq_index_cost, vq_plane_cost)
