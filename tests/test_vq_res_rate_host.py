"""Host-only checks of the rate term of the residual quantizer: the restated gradient against float64 autograd,
the one-stage identity with tests/vq_rate_ref.py, the library's workspace query and refusals (never-dereferenced pointers), the
`opt` field lambda_vq_stage_rate with its refusals, and the module method's host refusals.  Nothing here launches a kernel."""
import ctypes
import importlib.util
import math
import os

import pytest
import torch

import jpdse_hip
from jpdse_hip import F32
from ctu.models.model_options import resolve_model_options
from oracle.ctu_cpu import model as omodel
import vq_rate_ref
import vq_res_rate_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
  spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'scripts', name + '.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


MAKER = _load('make_model_option_refusals')


def _opt(*dicts, **over):
  kw = dict(MAKER.NET)
  for d in dicts:
    kw.update(d)
  kw.update(over)
  return omodel.default_opt(**kw)


# ---- the mathematics -------------------------------------------------------------------------------------------------------------
def _draw(M, L, D, S, seed):
  g = torch.Generator().manual_seed(seed)
  x = torch.randn(M, D, generator=g, dtype=torch.float64)
  books = torch.rand(S, L, D, generator=g, dtype=torch.float64) * 2 - 1
  dy = torch.randn(M, D, generator=g, dtype=torch.float64)
  return x, books, dy


@pytest.mark.parametrize('case', [(24, 5, 3, 3, 4, 3), (30, 7, 2, 4, 3, 2), (16, 4, 4, 1, 2, 1), (12, 6, 1, 2, 1, 2)], ids=str)
def test_restated_gradient_equals_fp64_autograd(case):
  """dhist by the stated formula and the grouped stage recursion against autograd of surrogate + scale * rate, stage prefixes
  included (books beyond the prefix get zeros)."""
  M, L, D, S, G, n = case
  x, books, dy = _draw(M, L, D, S, 100 + M + L)
  sigma, denom, scale = 1.0 / D, 7.0, 0.75
  rate, rates, hist, index = ref.rate(x, books, sigma, G, denom, n)
  assert tuple(rates.shape) == (n,) and tuple(hist.shape) == (n, G, L) and tuple(index.shape) == (n, M)
  assert torch.allclose(hist.sum(-1), torch.full((n, G), M / G, dtype=torch.float64), rtol=1e-12)
  assert float(rate) == float(sum(rates.tolist()[1:], rates.tolist()[0])) and 0 < float(rate) <= n * M * math.log2(L) / denom
  dhist = ref.dhist_of(hist, M // G, denom, scale)
  dx, dbooks = ref.bwd_grouped(dy, x, books, index, sigma, G, dhist)
  dx_auto, dbooks_auto = ref.grads(dy, x, books, sigma, G, denom, scale, n)
  assert torch.allclose(dx, dx_auto, rtol=1e-9, atol=1e-12)
  assert torch.allclose(dbooks, dbooks_auto[:n], rtol=1e-9, atol=1e-12) and not bool(dbooks_auto[n:].any())
  # the value of the differentiated loss is the hard forward's, and without a dhist the recursion is the plain surrogate's
  want = (books[torch.arange(n).unsqueeze(1), index].sum(0) * dy).sum() + scale * rate
  assert torch.allclose(ref.loss(x, books, sigma, G, denom, dy, scale, n), want, rtol=1e-12)
  import vq_residual_ref
  dx0, dbooks0 = ref.bwd_grouped(dy, x, books, index, sigma, G)
  dx_plain, dbooks_plain = vq_residual_ref.grads(dy, x, books, sigma, n)
  assert torch.allclose(dx0, dx_plain, rtol=1e-9, atol=1e-12) and torch.allclose(dbooks0, dbooks_plain[:n], rtol=1e-9, atol=1e-12)
  assert not torch.allclose(dbooks, dbooks0)


def test_one_stage_is_the_rate_term_of_the_bottleneck():
  x, books, dy = _draw(40, 6, 3, 1, 9)
  sigma, G, denom, scale = 0.5, 4, 11.0, 1.5
  rate, rates, hist, index = ref.rate(x, books, sigma, G, denom)
  rate1, hist1 = vq_rate_ref.rate(x, books[0], sigma, G, denom)
  assert torch.equal(rate, rate1) and torch.equal(rates[0], rate1) and torch.equal(hist[0], hist1)
  dhist = ref.dhist_of(hist, 10, denom, scale)
  assert torch.equal(dhist[0], vq_rate_ref.dhist_of(hist1, 10, denom, scale))
  dx, dbooks = ref.bwd_grouped(dy, x, books, index, sigma, G, dhist)
  dx1, dc1 = vq_rate_ref.quantize_bwd_grouped(dy, x, books[0], sigma, G, dhist[0])
  assert torch.equal(dx, dx1) and torch.equal(dbooks[0], dc1)


# ---- the library -------------------------------------------------------------------------------------------------------------------
def test_workspace_query_is_zero_outside_every_limit():
  q = jpdse_hip.lib().jpdse_vq_res_rate_workspace_size
  assert 0 < q(4112, 8, 64, 16, 4) <= 16 << 20 and 0 < q(1 << 20, 8, 64, 16, 4) <= 16 << 20
  assert 0 < q(1, 1, 2, 1, 1) and 0 < q(1040, 4, 16, 130, 8) and 0 < q(304, 32, 512, 16, 8) <= 16 << 20
  for bad in ((0, 8, 64, 16, 2), (64, 0, 64, 16, 2), (64, 33, 64, 16, 2), (64, 8, 1, 16, 2), (64, 8, 513, 16, 2), (64, 8, 64, 0, 2),
              (64, 8, 64, 5, 2), (64, 8, 64, 16, 0), (64, 8, 64, 16, 9), (1 << 20, 8, 512, 256, 1), (1 << 18, 8, 512, 128, 2),
              (1 << 23, 8, 512, 1, 1), (-4, 8, 64, 2, 2)):
    assert q(*bad) == 0, bad


P = 0x1000      # never dereferenced: every call below is refused first


def _fwd_args(**kw):
  v = dict(dtype=F32, M=64, D=8, L=64, S=4, n_stages=4, G=16, sigma=0.125, scale=1.0, denom=64.0, x=P, books=P, rate=P, rates=P,
           hist=None, dhist=None, y=None, index=None, ws=P, ws_bytes=1 << 30, stream=None)
  v.update(kw)
  return jpdse_hip.VqResRateFwdArgs(**v)


def _bwd_args(G=16, dhist=P, **kw):
  v = dict(dtype=F32, M=64, D=8, L=64, S=4, n_stages=4, sigma=0.125, dy=P, x=P, books=P, index=P, dx=P, dbooks=None, ws=None,
           ws_bytes=0, stream=None)
  v.update(kw)
  return jpdse_hip.VqResBwdGroupedArgs(jpdse_hip.VqResBwdArgs(**v), G, dhist)


FWD_REFUSALS = [
    (dict(dtype=7), 'bad dtype'), (dict(M=0), 'M = 0'), (dict(D=33), 'center_size D = 33'), (dict(L=1), 'n_center L = 1'),
    (dict(M=1 << 23, L=512, G=1), 'M * L'), (dict(S=9), 'S = 9 stages'), (dict(S=0), 'S = 0 stages'),
    (dict(n_stages=0), 'n_stages = 0'), (dict(n_stages=5), 'n_stages = 5'), (dict(G=0), 'G = 0 groups'),
    (dict(G=5), 'G = 5 does not divide M = 64'), (dict(M=1 << 12, L=512, G=256, n_stages=1), 'G * L = 131072'),
    (dict(M=1 << 12, L=512, G=64, n_stages=4), 'n_stages * G * L = 131072'),
    (dict(sigma=0.0), 'sigma is 0'), (dict(sigma=float('nan')), 'sigma is nan'), (dict(sigma=float('inf')), 'sigma is inf'),
    (dict(scale=float('inf')), 'scale is inf'), (dict(scale=float('nan')), 'scale is nan'),
    (dict(denom=0.0), 'denom is 0'), (dict(denom=-1.0), 'denom is -1'), (dict(denom=float('inf')), 'denom is inf'),
    (dict(x=None), 'null pointer (x, books)'), (dict(books=None), 'null pointer (x, books)'),
    (dict(rate=None), 'null pointer (rate, rates)'), (dict(rates=None), 'null pointer (rate, rates)'),
    (dict(y=P), 'y and index come together'), (dict(index=P), 'y and index come together'),
    (dict(ws=None), 'workspace too small'), (dict(ws_bytes=16), 'workspace too small'),
]


@pytest.mark.parametrize('over,field', FWD_REFUSALS, ids=[str(o) for o, _ in FWD_REFUSALS])
def test_rate_forward_refuses_on_the_host_by_field(over, field):
  lib = jpdse_hip.lib()
  assert 'jpdse_vq_res_rate_fwd' in jpdse_hip.SIGNATURES
  assert lib.jpdse_vq_res_rate_fwd(ctypes.byref(_fwd_args(**over))) == -1, field
  assert field in jpdse_hip.last_error() and 'vq_res_rate_fwd' in jpdse_hip.last_error(), (field, jpdse_hip.last_error())


BWD_REFUSALS = [
    (dict(dtype=7), 'bad dtype'), (dict(M=0), 'M = 0'), (dict(D=0), 'center_size D = 0'), (dict(L=513), 'n_center L = 513'),
    (dict(S=9), 'S = 9 stages'), (dict(n_stages=0), 'n_stages = 0'), (dict(n_stages=5), 'n_stages = 5'), (dict(G=0), 'G = 0 groups'),
    (dict(G=3), 'G = 3 does not divide M = 64'), (dict(M=1 << 12, L=512, G=256, n_stages=1), 'G * L = 131072'),
    (dict(M=1 << 12, L=512, G=64, n_stages=4), 'n_stages * G * L = 131072'), (dict(sigma=-1.0), 'sigma is -1'),
    (dict(dy=None), 'null pointer'), (dict(index=None), 'null pointer'), (dict(dbooks=P), 'workspace too small'),
]


@pytest.mark.parametrize('over,field', BWD_REFUSALS, ids=[str(o) for o, _ in BWD_REFUSALS])
def test_grouped_backward_refuses_on_the_host_by_field(over, field):
  lib = jpdse_hip.lib()
  assert 'jpdse_vq_res_bwd_grouped' in jpdse_hip.SIGNATURES
  for dhist in (P, None):                       # the group checks hold with and without a dhist
    assert lib.jpdse_vq_res_bwd_grouped(ctypes.byref(_bwd_args(dhist=dhist, **over))) == -1, field
    assert field in jpdse_hip.last_error() and 'vq_res_bwd_grouped' in jpdse_hip.last_error(), (field, jpdse_hip.last_error())


def test_null_structs_and_the_abi_version():
  lib = jpdse_hip.lib()
  assert lib.jpdse_version() == 2
  assert lib.jpdse_vq_res_rate_fwd(None) == -1 and 'null argument struct' in jpdse_hip.last_error()
  assert lib.jpdse_vq_res_bwd_grouped(None) == -1 and 'null argument struct' in jpdse_hip.last_error()
  # the grouped struct is the plain one plus G and dhist
  assert ctypes.sizeof(jpdse_hip.VqResBwdGroupedArgs) == ctypes.sizeof(jpdse_hip.VqResBwdArgs) + 16
  assert jpdse_hip.VqResBwdGroupedArgs.bwd.offset == 0


# ---- the option --------------------------------------------------------------------------------------------------------------------
def test_lambda_vq_stage_rate_is_accepted_with_stages():
  with MAKER.hidden_device():
    for value, want in ((0.5, 0.5), (2, 2.0), (0, 0.0), (0.0, 0.0), (None, 0.0)):
      rec = resolve_model_options(_opt(MAKER.S2HVQ, vq_stages=3, lambda_vq_stage_rate=value))
      assert rec.lambda_vq_stage_rate == want and isinstance(rec.lambda_vq_stage_rate, float) and rec.lambda_vq_rate == 0.0
    rec = resolve_model_options(_opt(MAKER.S2HVQ, vq_stages=2, vq_train_stages='uniform', lambda_vq_stage_rate=0.25))
    assert rec.lambda_vq_stage_rate == 0.25 and rec.vq_train_stages == 'uniform'
    # at 0 the field goes with everything, one stage and --zero_vis included
    assert resolve_model_options(_opt(MAKER.S2HVQ, lambda_vq_stage_rate=0.0, lambda_vq_rate=0.5)).lambda_vq_rate == 0.5
    assert resolve_model_options(_opt(MAKER.S2HVQ, vq_stages=2, zero_vis=True, lambda_vq_stage_rate=0)).lambda_vq_stage_rate == 0.0
    assert resolve_model_options(_opt(MAKER.CODEC, lambda_vq_stage_rate=0.0)).lambda_vq_stage_rate == 0.0


ONE_STAGE = ('lambda_vq_stage_rate > 0 is the rate term of the residual bottleneck: it needs vq_stages > 1 (the one-stage bottleneck '
             'takes --lambda_vq_rate)')
OPTION_REFUSALS = [
    (dict(vq_stages=2, lambda_vq_stage_rate=-0.5), 'lambda_vq_stage_rate must be a finite number >= 0, got -0.5'),
    (dict(vq_stages=2, lambda_vq_stage_rate=float('inf')), 'lambda_vq_stage_rate must be a finite number >= 0, got inf'),
    (dict(vq_stages=2, lambda_vq_stage_rate=float('nan')), 'lambda_vq_stage_rate must be a finite number >= 0, got nan'),
    (dict(vq_stages=2, lambda_vq_stage_rate='1'), "lambda_vq_stage_rate must be a finite number >= 0, got '1'"),
    (dict(vq_stages=2, lambda_vq_stage_rate=True), 'lambda_vq_stage_rate must be a finite number >= 0, got True'),
    (dict(vq_stages=1, lambda_vq_stage_rate=0.5), ONE_STAGE),
    (dict(lambda_vq_stage_rate=0.5), ONE_STAGE),
    (dict(vq_stages=2, lambda_vq_stage_rate=0.5, zero_vis=True),
     'lambda_vq_stage_rate > 0 needs an encoder that runs: it cannot be combined with --zero_vis'),
]


@pytest.mark.parametrize('over,text', OPTION_REFUSALS, ids=[str(o) for o, _ in OPTION_REFUSALS])
def test_lambda_vq_stage_rate_is_refused_by_name(over, text):
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  with MAKER.hidden_device():
    with pytest.raises(ValueError) as err:
      resolve_model_options(_opt(MAKER.S2HVQ, over))
    assert str(err.value) == text and 'lambda_vq_stage_rate' in text
    with pytest.raises(ValueError) as err:                    # the constructor refuses before any network exists
      Pix2PixHDModel(_opt(MAKER.S2HVQ, over))
    assert str(err.value) == text


def test_the_earlier_refusals_come_first_and_stay():
  with MAKER.hidden_device():
    with pytest.raises(ValueError) as err:
      resolve_model_options(_opt(MAKER.S2HVQ, vq_stages=2, lambda_vq_rate=1, lambda_vq_stage_rate=-1))
    assert str(err.value) == 'vq_stages = 2 cannot be combined with --lambda_vq_rate > 0: the rate term is built for one stage'
    with pytest.raises(ValueError, match="vq_train_stages must be 'all' or 'uniform'"):
      resolve_model_options(_opt(MAKER.S2HVQ, vq_stages=2, vq_train_stages='x', lambda_vq_stage_rate=-1))
    with pytest.raises(ValueError, match='lambda_vq_stage_rate'):         # and the class weights after it
      resolve_model_options(_opt(MAKER.S2HVQ, vq_stages=2, lambda_vq_stage_rate=-1, class_distortion_weights='24'))


def test_an_opt_without_the_field_resolves_as_with_zero():
  with MAKER.hidden_device():
    for base in ({}, MAKER.CODEC, MAKER.S2HVQ, dict(MAKER.S2HVQ, vq_stages=3), dict(MAKER.S2HVQ, vq_stages=2, vq_train_stages='uniform'),
                 dict(MAKER.S2HVQ, lambda_vq_rate=0.5)):
      assert not hasattr(_opt(base), 'lambda_vq_stage_rate')
      plain = resolve_model_options(_opt(base))
      given = resolve_model_options(_opt(base, lambda_vq_stage_rate=0.0))
      assert plain == given and plain.lambda_vq_stage_rate == 0.0
      assert plain._fields[-3:] == ('lambda_vq_stage_rate', 'vq_stages', 'vq_train_stages')


def test_the_stages_codec_takes_the_field_as_its_rate_weight():
  from ctu.models.codec import VQStagesCodec, VQIndexCodec
  assert VQStagesCodec.RATE_OPTION == 'lambda_vq_stage_rate' and VQIndexCodec.RATE_OPTION == 'lambda_vq_rate'
  assert VQStagesCodec(None, F32).rate_denom(3, 32, 64) == 3 * 32 * 64


# ---- the module: refused before any device work ------------------------------------------------------------------------------------
def test_module_rate_refuses_on_the_host():
  from ctu.quantizers import ResidualS2HVQ
  vq = ResidualS2HVQ(torch.zeros(3, 8, 4))
  x = torch.zeros(6, 8)                         # code_len 2: M = 12
  for bad in (0, 4, True, 1.0):
    with pytest.raises(ValueError, match='stages must be an int in 1 .. 3'):
      vq.rate(x, 2, stages=bad)
  for bad in (0, 5, -1):
    with pytest.raises(ValueError, match='groups must divide n \\* code_len'):
      vq.rate(x, 2, groups=bad)
  for bad in (0.0, -2.0, float('inf'), float('nan')):
    with pytest.raises(ValueError, match='denom must be a finite number > 0'):
      vq.rate(x, 2, groups=3, denom=bad)
  with pytest.raises(ValueError, match='code_len must divide'):
    vq.rate(x, 3)
  big = ResidualS2HVQ(torch.zeros(2, 512, 1))
  with pytest.raises(NotImplementedError, match='stages \\* groups \\* n_center = 131072'):
    big.rate(torch.zeros(128, 1), 1, groups=128)
  with pytest.raises(Exception):                # a good call gets as far as the device check
    vq.rate(x, 2, groups=3)
