"""ctypes binding of libjpdse_hip.so (C ABI: include/jpdse.h).

The library is the product; there is deliberately NO fallback.  If the shared object is
missing or a call fails, this module raises -- it never routes to torch ops or to oracle/.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# JPDSE_HIP_LIB: developer override (same-box A/B of two builds of this library); the default is the in-tree build
LIB_PATH = os.environ.get('JPDSE_HIP_LIB') or os.path.join(_HERE, 'libjpdse_hip.so')

F32, BF16 = 0, 1
PAD_ZERO, PAD_REFLECT = 0, 1
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3


class JpdseError(RuntimeError):
  pass


class ConvDesc(ctypes.Structure):
  _fields_ = [('dtype', ctypes.c_int32), ('N', ctypes.c_int32), ('H', ctypes.c_int32),
              ('W', ctypes.c_int32), ('C', ctypes.c_int32), ('K', ctypes.c_int32),
              ('R', ctypes.c_int32), ('S', ctypes.c_int32), ('stride', ctypes.c_int32),
              ('pad', ctypes.c_int32), ('pad_mode', ctypes.c_int32), ('act', ctypes.c_int32),
              ('slope', ctypes.c_float)]


class InormDesc(ctypes.Structure):
  _fields_ = [('dtype', ctypes.c_int32), ('N', ctypes.c_int32), ('H', ctypes.c_int32),
              ('W', ctypes.c_int32), ('C', ctypes.c_int32), ('act', ctypes.c_int32),
              ('slope', ctypes.c_float), ('eps', ctypes.c_float), ('has_residual', ctypes.c_int32),
              ('alias', ctypes.c_int32)]


class PackEntry(ctypes.Structure):
  _fields_ = [('w', ctypes.c_void_p), ('out', ctypes.c_void_p)] + \
             [(n, ctypes.c_int32) for n in ('K', 'Ks', 'C', 'Cs', 'R', 'S', 'st', 'qh', 'qw', 'Uh', 'Uw', 'Lk', 'gx', 'gy',
                                            'out_f32', 'reserved_')] + \
             [('blocks', ctypes.c_int64), ('block0', ctypes.c_int64)]


class LossTerm(ctypes.Structure):
  _fields_ = [('partial', ctypes.c_void_p), ('n', ctypes.c_int32), ('inv_count', ctypes.c_float), ('out', ctypes.c_void_p)]


class AdamEntry(ctypes.Structure):
  _fields_ = [('p', ctypes.c_void_p), ('g', ctypes.c_void_p), ('m', ctypes.c_void_p),
              ('v', ctypes.c_void_p), ('n', ctypes.c_int64), ('block0', ctypes.c_int64),
              ('cast_bf16', ctypes.c_void_p)]


class EvalMetricsSemArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('dtype_fake', 'dtype_real', 'N', 'H', 'W', 'C')] + \
             [('fake', ctypes.c_void_p), ('real', ctypes.c_void_p), ('label', ctypes.c_void_p), ('n_classes', ctypes.c_int32),
              ('mean', ctypes.POINTER(ctypes.c_double)), ('std', ctypes.POINTER(ctypes.c_double)), ('out', ctypes.c_void_p),
              ('cls', ctypes.c_void_p), ('ws', ctypes.c_void_p), ('ws_bytes', ctypes.c_size_t), ('stream', ctypes.c_void_p)]


class MsssimLossArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('dtype', 'N', 'H', 'W', 'C')] + \
             [('fake', ctypes.c_void_p), ('real', ctypes.c_void_p), ('mean', ctypes.POINTER(ctypes.c_double)),
              ('std', ctypes.POINTER(ctypes.c_double)), ('out', ctypes.c_void_p), ('stats', ctypes.c_void_p),
              ('dfake', ctypes.c_void_p), ('scale', ctypes.c_float), ('ws', ctypes.c_void_p), ('ws_bytes', ctypes.c_size_t),
              ('stream', ctypes.c_void_p)]


class CodeRateArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('dtype', 'N', 'H', 'W', 'C')] + \
             [('pixels', ctypes.c_int64), ('b', ctypes.c_void_p), ('t', ctypes.c_void_p), ('grad', ctypes.c_void_p),
              ('scale', ctypes.c_float), ('out', ctypes.c_void_p), ('per_image', ctypes.c_void_p), ('counts', ctypes.c_void_p),
              ('ws', ctypes.c_void_p), ('ws_bytes', ctypes.c_size_t), ('stream', ctypes.c_void_p)]


class SemLossArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('dtype', 'N', 'H', 'W', 'C', 'kind')] + \
             [('fake', ctypes.c_void_p), ('real', ctypes.c_void_p), ('label', ctypes.c_void_p), ('inst', ctypes.c_void_p),
              ('table', ctypes.POINTER(ctypes.c_float)), ('n_table', ctypes.c_int32), ('edge_w', ctypes.c_float),
              ('scale', ctypes.c_float), ('out', ctypes.c_void_p), ('dfake', ctypes.c_void_p), ('ws', ctypes.c_void_p),
              ('ws_bytes', ctypes.c_size_t), ('stream', ctypes.c_void_p)]


class CodeCostArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('dtype', 'N', 'h', 'w', 'C')] + \
             [('b', ctypes.c_void_p), ('H', ctypes.c_int32), ('W', ctypes.c_int32), ('label', ctypes.c_void_p),
              ('n_classes', ctypes.c_int32), ('symbol', ctypes.c_void_p), ('cell', ctypes.c_void_p), ('channel', ctypes.c_void_p),
              ('class_units', ctypes.c_void_p), ('class_pixels', ctypes.c_void_p), ('ws', ctypes.c_void_p),
              ('ws_bytes', ctypes.c_size_t), ('stream', ctypes.c_void_p)]


# the jpdse_vq_* calls (vq.hip)
class VqSoftFwdArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('dtype', 'M', 'D', 'L')] + \
             [('sigma', ctypes.c_float), ('x', ctypes.c_void_p), ('code_book', ctypes.c_void_p), ('p', ctypes.c_void_p),
              ('stream', ctypes.c_void_p)]


class VqHardFwdArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('dtype', 'M', 'D', 'L')] + \
             [('x', ctypes.c_void_p), ('code_book', ctypes.c_void_p), ('index', ctypes.c_void_p), ('onehot', ctypes.c_void_p),
              ('stream', ctypes.c_void_p)]


class VqSoftBwdArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('dtype', 'M', 'D', 'L')] + \
             [('sigma', ctypes.c_float), ('dp', ctypes.c_void_p), ('p', ctypes.c_void_p), ('x', ctypes.c_void_p),
              ('code_book', ctypes.c_void_p), ('dx', ctypes.c_void_p), ('dcode_book', ctypes.c_void_p), ('ws', ctypes.c_void_p),
              ('ws_bytes', ctypes.c_size_t), ('stream', ctypes.c_void_p)]


class VqDecodeArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('dtype', 'M', 'D', 'L')] + \
             [('index', ctypes.c_void_p), ('code_book', ctypes.c_void_p), ('y', ctypes.c_void_p), ('status', ctypes.c_void_p),
              ('stream', ctypes.c_void_p)]


class VqDecodeBwdArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('dtype', 'M', 'D', 'L')] + \
             [('index', ctypes.c_void_p), ('dy', ctypes.c_void_p), ('dcode_book', ctypes.c_void_p), ('status', ctypes.c_void_p),
              ('ws', ctypes.c_void_p), ('ws_bytes', ctypes.c_size_t), ('stream', ctypes.c_void_p)]


class VqArgmaxArgs(ctypes.Structure):
  _fields_ = [('M', ctypes.c_int32), ('L', ctypes.c_int32), ('s', ctypes.c_void_p), ('index', ctypes.c_void_p),
              ('stream', ctypes.c_void_p)]


class VqPmfArgs(ctypes.Structure):
  _fields_ = [('M', ctypes.c_int32), ('L', ctypes.c_int32), ('s', ctypes.c_void_p), ('pmf', ctypes.c_void_p),
              ('ws', ctypes.c_void_p), ('ws_bytes', ctypes.c_size_t), ('stream', ctypes.c_void_p)]


class VqPmfBwdArgs(ctypes.Structure):
  _fields_ = [('M', ctypes.c_int32), ('L', ctypes.c_int32), ('dpmf', ctypes.c_void_p), ('ds', ctypes.c_void_p),
              ('stream', ctypes.c_void_p)]


# the jpdse_vq_index_* calls (vq_coder.hip)
class VqIndexEncodeArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('M', 'L', 'S')] + \
             [('index', ctypes.c_void_p), ('out', ctypes.c_void_p), ('out_bytes', ctypes.c_int64), ('size', ctypes.c_void_p),
              ('status', ctypes.c_void_p), ('ws', ctypes.c_void_p), ('ws_bytes', ctypes.c_size_t), ('stream', ctypes.c_void_p)]


class VqIndexDecodeArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('M', 'L', 'S')] + \
             [('in_', ctypes.c_void_p), ('in_bytes', ctypes.c_int64), ('index', ctypes.c_void_p), ('status', ctypes.c_void_p),
              ('stream', ctypes.c_void_p)]


# the jpdse_vq_plane_* calls (vq_plane.hip)
class VqPlaneEncodeArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('h', 'w', 'G', 'L', 'strip_rows')] + \
             [('index', ctypes.c_void_p), ('out', ctypes.c_void_p), ('out_bytes', ctypes.c_int64), ('size', ctypes.c_void_p),
              ('status', ctypes.c_void_p), ('ws', ctypes.c_void_p), ('ws_bytes', ctypes.c_size_t), ('stream', ctypes.c_void_p)]


class VqPlaneDecodeArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('h', 'w', 'G', 'L', 'strip_rows')] + \
             [('in_', ctypes.c_void_p), ('in_bytes', ctypes.c_int64), ('index', ctypes.c_void_p), ('status', ctypes.c_void_p),
              ('stream', ctypes.c_void_p)]


# the jpdse_vq_*_cost calls (vq_cost.hip)
_VQ_COST_TAIL = [('H', ctypes.c_int32), ('W', ctypes.c_int32), ('label', ctypes.c_void_p), ('n_classes', ctypes.c_int32),
                 ('symbol', ctypes.c_void_p), ('cell', ctypes.c_void_p), ('group', ctypes.c_void_p),
                 ('stream_units', ctypes.c_void_p), ('stream_decisions', ctypes.c_void_p), ('status', ctypes.c_void_p),
                 ('class_units', ctypes.c_void_p), ('class_pixels', ctypes.c_void_p), ('ws', ctypes.c_void_p),
                 ('ws_bytes', ctypes.c_size_t), ('stream', ctypes.c_void_p)]


class VqIndexCostArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('M', 'L', 'S', 'G')] + \
             [('index', ctypes.c_void_p), ('h', ctypes.c_int32), ('w', ctypes.c_int32)] + _VQ_COST_TAIL


class VqPlaneCostArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('h', 'w', 'G', 'L', 'strip_rows')] + [('index', ctypes.c_void_p)] + _VQ_COST_TAIL


# the jpdse_vq_quantize_* calls (vq_bottleneck.hip)
class VqQuantizeFwdArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('dtype', 'M', 'D', 'L')] + \
             [('sigma', ctypes.c_float), ('hard_forward', ctypes.c_int32), ('x', ctypes.c_void_p), ('code_book', ctypes.c_void_p),
              ('y', ctypes.c_void_p), ('index', ctypes.c_void_p), ('pmf', ctypes.c_void_p), ('ws', ctypes.c_void_p),
              ('ws_bytes', ctypes.c_size_t), ('stream', ctypes.c_void_p)]


class VqQuantizeBwdArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('dtype', 'M', 'D', 'L')] + \
             [('sigma', ctypes.c_float), ('dy', ctypes.c_void_p), ('x', ctypes.c_void_p), ('code_book', ctypes.c_void_p),
              ('dpmf', ctypes.c_void_p), ('dx', ctypes.c_void_p), ('dcode_book', ctypes.c_void_p), ('ws', ctypes.c_void_p),
              ('ws_bytes', ctypes.c_size_t), ('stream', ctypes.c_void_p)]


# the rate term of the vector-quantizer bottleneck (vq_bottleneck.hip)
class VqRateFwdArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('dtype', 'M', 'D', 'L', 'G')] + \
             [('sigma', ctypes.c_float), ('hard', ctypes.c_int32), ('x', ctypes.c_void_p), ('code_book', ctypes.c_void_p),
              ('scale', ctypes.c_float), ('denom', ctypes.c_float), ('hist', ctypes.c_void_p), ('rate', ctypes.c_void_p),
              ('dhist', ctypes.c_void_p), ('ws', ctypes.c_void_p), ('ws_bytes', ctypes.c_size_t), ('stream', ctypes.c_void_p)]


class VqQuantizeBwdGroupedArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('dtype', 'M', 'D', 'L', 'G')] + \
             [('sigma', ctypes.c_float), ('dy', ctypes.c_void_p), ('x', ctypes.c_void_p), ('code_book', ctypes.c_void_p),
              ('dhist', ctypes.c_void_p), ('dx', ctypes.c_void_p), ('dcode_book', ctypes.c_void_p), ('ws', ctypes.c_void_p),
              ('ws_bytes', ctypes.c_size_t), ('stream', ctypes.c_void_p)]


# the code-book fit (vq_fit.hip)
class VqLloydAccumArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('dtype', 'M', 'D', 'L', 'first')] + \
             [(n, ctypes.c_void_p) for n in ('x', 'code_book', 'counts', 'sums', 'sse', 'far_dist', 'far_vec', 'ws')] + \
             [('ws_bytes', ctypes.c_size_t), ('stream', ctypes.c_void_p)]


class VqLloydUpdateArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('D', 'L', 'reseed')] + \
             [(n, ctypes.c_void_p) for n in ('code_book', 'counts', 'sums', 'sse', 'far_dist', 'far_vec', 'report', 'stream')]


# the entropy-constrained assignment (vq_ec.hip)
class VqEcAssignArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('dtype', 'M', 'D', 'L', 'G')] + \
             [(n, ctypes.c_void_p) for n in ('x', 'code_book', 'bias', 'index', 'hist', 'sse', 'ws')] + \
             [('ws_bytes', ctypes.c_size_t), ('stream', ctypes.c_void_p)]


class VqEcLengthsArgs(ctypes.Structure):
  _fields_ = [('G', ctypes.c_int32), ('L', ctypes.c_int32), ('lam', ctypes.c_double), ('hist', ctypes.c_void_p),
              ('bias', ctypes.c_void_p), ('bits', ctypes.c_void_p), ('stream', ctypes.c_void_p)]


# the residual quantizer (vq_residual.hip)
VQ_RES_MAX_STAGES = 8


class VqResFwdArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('dtype', 'M', 'D', 'L', 'S', 'n_stages')] + \
             [(n, ctypes.c_void_p) for n in ('x', 'books', 'y', 'index', 'sse', 'residual', 'ws')] + \
             [('ws_bytes', ctypes.c_size_t), ('stream', ctypes.c_void_p)]


class VqResRowsFwdArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('dtype', 'M', 'D', 'L', 'S', 'n_stages')] + \
             [(n, ctypes.c_void_p) for n in ('x', 'books', 'y', 'index', 'stream')]


class VqResEcAssignArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('dtype', 'M', 'D', 'L', 'S', 'n_stages', 'G')] + \
             [(n, ctypes.c_void_p) for n in ('x', 'books', 'bias', 'y', 'index', 'hist', 'sse', 'ws')] + \
             [('ws_bytes', ctypes.c_size_t), ('stream', ctypes.c_void_p)]


class VqResDecodeArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('dtype', 'M', 'D', 'L', 'S', 'n_stages')] + \
             [(n, ctypes.c_void_p) for n in ('index', 'books', 'y', 'status', 'stream')]


class VqResBwdArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('dtype', 'M', 'D', 'L', 'S', 'n_stages')] + [('sigma', ctypes.c_float)] + \
             [(n, ctypes.c_void_p) for n in ('dy', 'x', 'books', 'index', 'dx', 'dbooks', 'ws')] + \
             [('ws_bytes', ctypes.c_size_t), ('stream', ctypes.c_void_p)]


# the residual quantizer's rate term (vq_res_rate.hip, vq_residual.hip)
class VqResRateFwdArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('dtype', 'M', 'D', 'L', 'S', 'n_stages', 'G')] + \
             [(n, ctypes.c_float) for n in ('sigma', 'scale', 'denom')] + \
             [(n, ctypes.c_void_p) for n in ('x', 'books', 'rate', 'rates', 'hist', 'dhist', 'y', 'index', 'ws')] + \
             [('ws_bytes', ctypes.c_size_t), ('stream', ctypes.c_void_p)]


class VqResBwdGroupedArgs(ctypes.Structure):
  _fields_ = [('bwd', VqResBwdArgs), ('G', ctypes.c_int32), ('dhist', ctypes.c_void_p)]


# a stage depth per cell (vq_residual.hip): the plain struct, G vectors per cell, depth int32 [M / G]
class VqResRowsFwdDepthArgs(ctypes.Structure):
  _fields_ = [('fwd', VqResRowsFwdArgs), ('G', ctypes.c_int32), ('depth', ctypes.c_void_p)]


class VqResDecodeDepthArgs(ctypes.Structure):
  _fields_ = [('dec', VqResDecodeArgs), ('G', ctypes.c_int32), ('depth', ctypes.c_void_p)]


class VqResBwdDepthArgs(ctypes.Structure):
  _fields_ = [('bwd', VqResBwdArgs), ('G', ctypes.c_int32), ('depth', ctypes.c_void_p)]


class VqDepthMapArgs(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in ('N', 'H', 'W', 'step', 'n_classes', 'default_depth')] + \
             [(n, ctypes.c_void_p) for n in ('label', 'table', 'depth', 'stream')]


_P, _I32, _I64, _F, _SZ = (ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float,
                           ctypes.c_size_t)
_CD, _ND = ctypes.POINTER(ConvDesc), ctypes.POINTER(InormDesc)

# name -> (restype, argtypes); every symbol declared in include/jpdse.h
SIGNATURES = {
    'jpdse_version': (_I32, []),
    'jpdse_last_error': (ctypes.c_char_p, []),
    'jpdse_arch_check': (_I32, [_I32]),
    'jpdse_prof_select': (_I32, [_I32, _I32, _I64, _I32]),
    'jpdse_prof_collect': (_I32, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_I64)]),
    'jpdse_prof_collect_class': (_I32, [_I32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_I64)]),
    'jpdse_prof_hbm_select': (_I32, [_I32, _I32]),
    'jpdse_prof_hbm_collect': (_I32, [_I32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_I64)]),
    'jpdse_conv_out_shape': (_I32, [_CD, ctypes.POINTER(_I32), ctypes.POINTER(_I32)]),
    'jpdse_conv_plan_query': (_I32, [_CD, ctypes.POINTER(_I32), _I32]),
    'jpdse_conv_fwd_pack_size': (_SZ, [_CD]),
    'jpdse_conv_dgrad_pack_size': (_SZ, [_CD]),
    'jpdse_conv_pack_entries': (_I32, [_CD, _P, _P, ctypes.POINTER(PackEntry), _I32]),
    'jpdse_conv_pack_run': (_I32, [_P, _I32, _I64, _P]),
    'jpdse_conv_pack_weights': (_I32, [_CD, _P, _P, _P, _P]),
    'jpdse_conv_workspace_size': (_SZ, [_CD]),
    'jpdse_conv_fwd': (_I32, [_CD, _P, _P, _P, _P, _P, _SZ, _P]),
    'jpdse_conv_fwd_pool': (_I32, [_CD, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    'jpdse_conv_dgrad': (_I32, [_CD, _P, _P, _P, _P, _SZ, _P]),
    'jpdse_conv_dgrad_relu': (_I32, [_CD, _P, _P, _P, _P, _P, _SZ, _P]),
    'jpdse_conv_dgrad_fused': (_I32, [_CD, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    'jpdse_conv_dgrad_fused_lrelu': (_I32, [_CD, _P, _P, _P, _F, _P, _P, _P, _SZ, _P]),
    'jpdse_conv_dgrad_batched': (_I32, [_CD, _P, _P, _P, _F, _P, _I32, _I32, _P, _P, _SZ, _P]),
    'jpdse_conv_dgrad_nsum_slots': (_I32, [_CD]),
    'jpdse_conv_dgrad_fused_nsums': (_I32, [_CD, _P, _P, _P, _P, _P, _P, _P, _I32, _F, _P, _P, _SZ, _P]),
    'jpdse_conv_wgrad': (_I32, [_CD, _P, _P, _P, _P, _SZ, _P]),
    'jpdse_convT_fwd': (_I32, [_CD, _P, _P, _P, _P, _SZ, _P]),
    'jpdse_conv_moment_slots': (_I32, [_CD]),
    'jpdse_convT_moment_slots': (_I32, [_CD]),
    'jpdse_conv_fwd_moments': (_I32, [_CD, _P, _P, _P, _P, _P, _SZ, _P]),
    'jpdse_convT_fwd_moments': (_I32, [_CD, _P, _P, _P, _P, _P, _SZ, _P]),
    'jpdse_inorm_fwd_from_moments': (_I32, [_ND, _P, _P, _I32, _P, _P, _P, _P]),
    'jpdse_convT_dgrad': (_I32, [_CD, _P, _P, _P, _P, _SZ, _P]),
    'jpdse_convT_wgrad': (_I32, [_CD, _P, _P, _P, _P, _SZ, _P]),
    'jpdse_inorm_workspace_size': (_SZ, [_ND]),
    'jpdse_inorm_fwd': (_I32, [_ND, _P, _P, _P, _P, _P, _SZ, _P]),
    'jpdse_inorm_bwd': (_I32, [_ND, _P, _P, _P, _P, _P, _SZ, _P]),
    'jpdse_inorm_bwd_from_sums': (_I32, [_ND, _P, _P, _P, _P, _I32, _P, _P, _SZ, _P]),
    'jpdse_avgpool3s2_fwd': (_I32, [_I32, _I32, _I32, _I32, _I32, _P, _P, _P]),
    'jpdse_avgpool3s2_bwd': (_I32, [_I32, _I32, _I32, _I32, _I32, _P, _P, _P]),
    'jpdse_maxpool2_fwd': (_I32, [_I32, _I32, _I32, _I32, _I32, _P, _P, _P]),
    'jpdse_maxpool2_bwd': (_I32, [_I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P]),
    'jpdse_act_bwd': (_I32, [_I32, _I64, _I32, _F, _P, _P, _P, _P]),
    'jpdse_add': (_I32, [_I32, _I64, _P, _P, _P, _P]),
    'jpdse_channel_sum_workspace_size': (_SZ, [_I64, _I32]),
    'jpdse_channel_sum': (_I32, [_I32, _I64, _I32, _P, _P, _P, _SZ, _P]),
    'jpdse_channel_copy': (_I32, [_I32, _I64, _P, _I32, _I32, _P, _I32, _I32, _I32, _P]),
    'jpdse_concat_channels': (_I32, [_I32, _I64, _P, _I32, _P, _I32, _I32, _I32, _P, _P]),
    'jpdse_copy': (_I32, [_I64, _P, _P, _P]),
    'jpdse_zero': (_I32, [_I32, _I64, _P, _P]),
    'jpdse_cast': (_I32, [_I32, _I32, _I64, _P, _P, _P]),
    'jpdse_quant_loss_workspace_size': (_SZ, []),
    'jpdse_quant_loss': (_I32, [_I32, _I32, _I64, _I32, _P, _P, ctypes.POINTER(ctypes.c_double),
                                ctypes.POINTER(ctypes.c_double), _I32, _P, _P, _SZ, _P]),
    'jpdse_nchw_to_nhwc': (_I32, [_I32, _I32, _I32, _I32, _I32, _P, _P, _P]),
    'jpdse_nhwc_to_nchw': (_I32, [_I32, _I32, _I32, _I32, _I32, _P, _P, _P]),
    'jpdse_onehot_edge': (_I32, [_I32, _I32, _I32, _I32, _I32, _P, _P, _P, _I32, _P]),
    'jpdse_input_builder': (_I32, [_I32, _I32, _I32, _I32, _I32, _P, _P, _I32, ctypes.POINTER(_P), ctypes.POINTER(_P), _I32, _I32,
                                   _I32, _I32, _P]),
    'jpdse_input_builder_wide': (_I32, [_I32, _I32, _I32, _I32, _I32, _P, _P, _I32, ctypes.POINTER(_P), ctypes.POINTER(_P), _I32,
                                        _I32, _I32, _I32, _P]),
    'jpdse_insert_channels': (_I32, [_I32, _I64, _P, _I32, _P, _I32, _I32, _I32, _P]),
    'jpdse_loss_workspace_size': (_SZ, [_I64]),
    'jpdse_loss_partial_count': (_I32, [_I64]),
    'jpdse_loss_finalize': (_I32, [_P, _I32, _P]),
    'jpdse_l1_fwd': (_I32, [_I32, _I64, _I64, _P, _P, _P, _P, _SZ, _P]),
    'jpdse_l1_bwd': (_I32, [_I32, _I64, _I64, _P, _P, _P, _F, _P, _P]),
    'jpdse_l1_bwd_relu': (_I32, [_I32, _I64, _I64, _P, _P, _P, _F, _P, _P]),
    'jpdse_l1_fwd_bwd': (_I32, [_I32, _I64, _I64, _P, _P, _P, _F, _I32, _P, _P, _SZ, _P]),
    'jpdse_mse_fwd': (_I32, [_I32, _I64, _I64, _P, _P, _P, _P, _SZ, _P]),
    'jpdse_mse_bwd': (_I32, [_I32, _I64, _I64, _P, _P, _P, _F, _P, _P]),
    'jpdse_mse_const_fwd': (_I32, [_I32, _I64, _I32, _F, _P, _P, _P, _SZ, _P]),
    'jpdse_mse_const_bwd': (_I32, [_I32, _I64, _I32, _F, _P, _P, _F, _P, _P]),
    'jpdse_adam_step': (_I32, [_P, _I32, _I64, _F, _F, _F, _F, _I32, _F, _P]),
    'jpdse_binarize_fwd': (_I32, [_I32, _I32, _I32, _I32, _I32, _P, _P, _I32, ctypes.c_uint64, ctypes.c_uint64, _I64, _P, _P]),
    'jpdse_code_stats_workspace_size': (_SZ, [_I32, _I32, _I32, _I32, _I32]),
    'jpdse_code_stats': (_I32, [_I32, _I32, _I32, _I32, _I32, _P, _P, _P, _SZ, _P]),
    'jpdse_code_export': (_I32, [_I32, _I32, _I32, _I32, _I32, _P, _I32, _P, _P]),
    'jpdse_code_import': (_I32, [_I32, _I32, _I32, _I32, _I32, _P, _I32, _P, _P]),
    'jpdse_code_entropy_capacity': (_SZ, [_I32, _I32, _I32]),
    'jpdse_code_entropy_workspace_size': (_SZ, [_I32, _I32, _I32, _I32]),
    'jpdse_code_entropy_encode': (_I32, [_I32, _I32, _I32, _I32, _I32, _P, _P, _I64, _P, _P, _P, _SZ, _P]),
    'jpdse_code_entropy_decode': (_I32, [_I32, _I32, _I32, _I32, _I32, _P, _I64, ctypes.POINTER(_I32), _P, _P]),
    'jpdse_semantics_capacity': (_SZ, [_I32, _I32, _I32, _I32]),
    'jpdse_semantics_workspace_size': (_SZ, [_I32, _I32, _I32, _I32, _I32]),
    'jpdse_semantics_encode': (_I32, [_I32, _I32, _I32, _I32, _I32, _P, _P, _P, _I64, _P, _P, _P, _SZ, _P]),
    'jpdse_semantics_decode': (_I32, [_I32, _I32, _I32, _I32, _I32, _I32, _P, _I64, _I64, _P, _P, _P, _P, _P]),
    'jpdse_eval_metrics_workspace_size': (_SZ, [_I32, _I32, _I32, _I32]),
    'jpdse_eval_metrics': (_I32, [_I32, _I32, _I32, _I32, _I32, _I32, _P, _P, ctypes.POINTER(ctypes.c_double),
                                  ctypes.POINTER(ctypes.c_double), _P, _P, _SZ, _P]),
    'jpdse_eval_metrics_sem_workspace_size': (_SZ, [_I32, _I32, _I32, _I32, _I32]),
    'jpdse_eval_metrics_sem': (_I32, [ctypes.POINTER(EvalMetricsSemArgs)]),
    'jpdse_msssim_loss_workspace_size': (_SZ, [_I32, _I32, _I32, _I32, _I32]),
    'jpdse_msssim_loss': (_I32, [ctypes.POINTER(MsssimLossArgs)]),
    'jpdse_code_rate_workspace_size': (_SZ, [_I32, _I32, _I32, _I32]),
    'jpdse_code_rate_loss': (_I32, [ctypes.POINTER(CodeRateArgs)]),
    'jpdse_sem_weighted_loss': (_I32, [ctypes.POINTER(SemLossArgs)]),
    'jpdse_code_cost_table': (_I32, [ctypes.POINTER(ctypes.c_uint32)]),
    'jpdse_code_cost_workspace_size': (_SZ, [_I32, _I32, _I32, _I32, _I32]),
    'jpdse_code_cost': (_I32, [ctypes.POINTER(CodeCostArgs)]),
    'jpdse_vq_workspace_size': (_SZ, [_I32, _I32, _I32]),
    'jpdse_vq_soft_fwd': (_I32, [ctypes.POINTER(VqSoftFwdArgs)]),
    'jpdse_vq_hard_fwd': (_I32, [ctypes.POINTER(VqHardFwdArgs)]),
    'jpdse_vq_soft_bwd': (_I32, [ctypes.POINTER(VqSoftBwdArgs)]),
    'jpdse_vq_decode': (_I32, [ctypes.POINTER(VqDecodeArgs)]),
    'jpdse_vq_decode_bwd': (_I32, [ctypes.POINTER(VqDecodeBwdArgs)]),
    'jpdse_vq_argmax': (_I32, [ctypes.POINTER(VqArgmaxArgs)]),
    'jpdse_vq_pmf': (_I32, [ctypes.POINTER(VqPmfArgs)]),
    'jpdse_vq_pmf_bwd': (_I32, [ctypes.POINTER(VqPmfBwdArgs)]),
    'jpdse_vq_lloyd_workspace_size': (_SZ, [_I32, _I32, _I32]),
    'jpdse_vq_lloyd_accum': (_I32, [ctypes.POINTER(VqLloydAccumArgs)]),
    'jpdse_vq_lloyd_update': (_I32, [ctypes.POINTER(VqLloydUpdateArgs)]),
    'jpdse_vq_index_capacity': (_SZ, [_I32, _I32, _I32]),
    'jpdse_vq_index_workspace_size': (_SZ, [_I32, _I32, _I32]),
    'jpdse_vq_index_encode': (_I32, [ctypes.POINTER(VqIndexEncodeArgs)]),
    'jpdse_vq_index_decode': (_I32, [ctypes.POINTER(VqIndexDecodeArgs)]),
    'jpdse_vq_plane_capacity': (_SZ, [_I32, _I32, _I32, _I32, _I32]),
    'jpdse_vq_plane_workspace_size': (_SZ, [_I32, _I32, _I32, _I32, _I32]),
    'jpdse_vq_plane_encode': (_I32, [ctypes.POINTER(VqPlaneEncodeArgs)]),
    'jpdse_vq_plane_decode': (_I32, [ctypes.POINTER(VqPlaneDecodeArgs)]),
    'jpdse_vq_index_cost_workspace_size': (_SZ, [_I32, _I32, _I32, _I32, _I32]),
    'jpdse_vq_index_cost': (_I32, [ctypes.POINTER(VqIndexCostArgs)]),
    'jpdse_vq_plane_cost_workspace_size': (_SZ, [_I32, _I32, _I32, _I32, _I32, _I32]),
    'jpdse_vq_plane_cost': (_I32, [ctypes.POINTER(VqPlaneCostArgs)]),
    'jpdse_vq_quantize_workspace_size': (_SZ, [_I32, _I32, _I32]),
    'jpdse_vq_quantize_fwd': (_I32, [ctypes.POINTER(VqQuantizeFwdArgs)]),
    'jpdse_vq_quantize_bwd': (_I32, [ctypes.POINTER(VqQuantizeBwdArgs)]),
    'jpdse_vq_rate_workspace_size': (_SZ, [_I32, _I32, _I32, _I32]),
    'jpdse_vq_rate_fwd': (_I32, [ctypes.POINTER(VqRateFwdArgs)]),
    'jpdse_vq_ec_workspace_size': (_SZ, [_I32, _I32, _I32, _I32]),
    'jpdse_vq_ec_assign': (_I32, [ctypes.POINTER(VqEcAssignArgs)]),
    'jpdse_vq_ec_lengths': (_I32, [ctypes.POINTER(VqEcLengthsArgs)]),
    'jpdse_vq_quantize_bwd_grouped': (_I32, [ctypes.POINTER(VqQuantizeBwdGroupedArgs)]),
    'jpdse_vq_res_workspace_size': (_SZ, [_I32, _I32, _I32, _I32]),
    'jpdse_vq_res_fwd': (_I32, [ctypes.POINTER(VqResFwdArgs)]),
    'jpdse_vq_res_rows_fwd': (_I32, [ctypes.POINTER(VqResRowsFwdArgs)]),
    'jpdse_vq_res_decode': (_I32, [ctypes.POINTER(VqResDecodeArgs)]),
    'jpdse_vq_res_bwd': (_I32, [ctypes.POINTER(VqResBwdArgs)]),
    'jpdse_vq_res_ec_workspace_size': (_SZ, [_I32, _I32, _I32, _I32, _I32]),
    'jpdse_vq_res_ec_assign': (_I32, [ctypes.POINTER(VqResEcAssignArgs)]),
    'jpdse_vq_res_rate_workspace_size': (_SZ, [_I32, _I32, _I32, _I32, _I32]),
    'jpdse_vq_res_rate_fwd': (_I32, [ctypes.POINTER(VqResRateFwdArgs)]),
    'jpdse_vq_res_bwd_grouped': (_I32, [ctypes.POINTER(VqResBwdGroupedArgs)]),
    'jpdse_vq_res_rows_fwd_depth': (_I32, [ctypes.POINTER(VqResRowsFwdDepthArgs)]),
    'jpdse_vq_res_decode_depth': (_I32, [ctypes.POINTER(VqResDecodeDepthArgs)]),
    'jpdse_vq_res_bwd_depth': (_I32, [ctypes.POINTER(VqResBwdDepthArgs)]),
    'jpdse_vq_depth_map': (_I32, [ctypes.POINTER(VqDepthMapArgs)]),
}

# the developer build (same sources, -DJPDSE_DEV): the shipped ABI plus include/jpdse_dev.h
DEV_LIB_PATH = os.path.join(_HERE, 'libjpdse_hip_dev.so')
DEV_SIGNATURES = {'jpdse_debug_set_fast_path': (_I32, [_I32]),
                  'jpdse_debug_occupy_cus': (_I32, [_I32, _P, _I32, _P]),
                  'jpdse_debug_conv_route': (_I32, [_CD, _I32, ctypes.POINTER(_I32)]),
                  'jpdse_debug_route_name': (ctypes.c_char_p, [_I32, _I32])}

_lib = None
_dev = None
_binding_epoch = [0]     # bumped whenever the bound library or its kernel-selection mode changes (dev_mode enter / exit)


def binding_epoch():
  """Changes whenever answers cached from the library (e.g. a layer's moment-slot count) may have become stale."""
  return _binding_epoch[0]


def _load(path, signatures):
  handle = ctypes.CDLL(path)
  for name, (res, args) in signatures.items():
    fn = getattr(handle, name)   # AttributeError here == ABI/header drift: fail loudly
    fn.restype, fn.argtypes = res, args
  return handle


class dev_mode(object):
  """Developer / test tool: run the enclosed calls on libjpdse_hip_dev.so with kernel-selection mode `mode`
  (include/jpdse_dev.h: e.g. 0 = generic kernels only, 6 = no split-K, 19 = 16x16x32 MFMA halo variant).  The shipped
  library has no such switch; on exit the binding is back on it.  Not re-entrant, single threaded."""

  def __init__(self, mode):
    self.mode = int(mode)

  def __enter__(self):
    global _lib, _dev
    import torch  # noqa: F401
    lib()
    if _dev is None:
      if not os.path.isfile(DEV_LIB_PATH):
        raise JpdseError('libjpdse_hip_dev.so not found at %s -- build it with `make -C jpd-se_amd/csrc`' % DEV_LIB_PATH)
      sig = dict(SIGNATURES)
      sig.update(DEV_SIGNATURES)
      _dev = _load(DEV_LIB_PATH, sig)
    self._saved = _lib
    _lib = _dev
    _binding_epoch[0] += 1
    check(_dev.jpdse_debug_set_fast_path(self.mode), 'jpdse_debug_set_fast_path')
    return _dev

  def __exit__(self, *exc):
    global _lib
    _dev.jpdse_debug_set_fast_path(1)
    _lib = self._saved
    _binding_epoch[0] += 1
    return False


def set_dev_mode(mode):
  """Scripts: switch the binding to the developer build for the rest of the process, in kernel-selection mode `mode`."""
  dev_mode(mode).__enter__()


def lib():
  """The loaded library; raises JpdseError when libjpdse_hip.so has not been built."""
  global _lib
  if _lib is None:
    # torch first: it ships its own libamdhip64; loading ours before it would put a second HIP
    # runtime (the system one) into the process, which then sees no device.
    import torch  # noqa: F401
    if not os.path.isfile(LIB_PATH):
      raise JpdseError(
          'libjpdse_hip.so not found at %s -- build it with `python -c "import __graft_entry__ as g; '
          'g.build()"` or `make -C jpd-se_amd/csrc`.  There is no CPU/torch fallback.' % LIB_PATH)
    _lib = _load(LIB_PATH, SIGNATURES)
  return _lib


def last_error():
  return lib().jpdse_last_error().decode('utf-8', 'replace')


def check(rc, what):
  if rc != 0:
    raise JpdseError('%s failed (%d): %s' % (what, rc, last_error()))


def require_gpu(device=0):
  """Fail loudly unless `device` is a gfx950 GPU visible to this process."""
  import torch
  if not torch.cuda.is_available():
    raise JpdseError('no GPU visible: the JPD-SE HIP path has no CPU fallback')
  check(lib().jpdse_arch_check(int(device)), 'jpdse_arch_check')
