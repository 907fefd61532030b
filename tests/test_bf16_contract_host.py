"""The bf16 rounding contract (tests/bf16_contract.py) on the CPU: it accepts a correct fp32 implementation with room to spare and
rejects the errors it exists to catch, each of which today's bf16 bounds (hip_util RTOL / ETOL) let through.  torch-CPU only."""
import time

import pytest
import torch

from jpdse_hip import PAD_REFLECT, F32, BF16
import bf16_contract as bc
from bf16_contract import rn_bf16, ulp_bf16, Cand
from hip_util import RTOL, ETOL, rel_err, elem_err
from test_hip_ops import CONV_CASES

CASES = {c[0]: c for c in CONV_CASES}
HEAVY = ['resblock1024', 'tile320_path', 'taps_3x3s2_256', 'thin_ragged', 'd_layer4_1k', 'head_rows_7']


def test_rn_bf16_matches_fp32_rounding_and_avoids_double_rounding():
  g = torch.Generator().manual_seed(5)
  x = torch.randn(200000, generator=g) * torch.exp(torch.randn(200000, generator=g) * 8)
  x = torch.cat([x, torch.tensor([0.0, -0.0, 1.0, -3.0, 2.0 ** -130, -2.0 ** -128, 1e30])])
  # on fp32 inputs the result is torch's fp32 -> bf16 round-to-nearest-even
  assert torch.equal(rn_bf16(x.double()), x.to(torch.bfloat16).double())
  # exact midpoints round to even, both ways
  assert rn_bf16(torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8)])).tolist() == [1.0, 1.0 + 2 ** -6, -1.0]
  # just above a midpoint by less than fp32 resolves: fp64 -> fp32 -> bf16 lands on the midpoint and rounds to even (down)
  v = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)
  assert v.float().to(torch.bfloat16).double().item() == 1.0
  assert rn_bf16(v).item() == 1.0 + 2.0 ** -7


def test_ulp_bf16():
  v = torch.tensor([1.0, 1.5, -2.0, 0.75, 0.0, 2.0 ** -126, 2.0 ** -140, 3e5], dtype=torch.float64)
  assert ulp_bf16(v).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -133, 2.0 ** -133, 2.0 ** -133, 2.0 ** 11]


def test_frame_model_is_the_reflect_data_gradient():
  """Without its rounding, the folded-frame form of the candidates is the exact data gradient of the reflect-padded conv."""
  g = torch.Generator().manual_seed(3)
  dy = torch.randn(2, 5, 9, 11, generator=g, dtype=torch.float64)
  w = torch.randn(5, 4, 3, 3, generator=g, dtype=torch.float64)
  ref = bc.dgrad64(dy, w, (2, 4, 9, 11), 1, 1, PAD_REFLECT)
  assert (bc.frame_dgrad64(dy, w, round_frame=False) - ref).abs().max().item() < 1e-12


def _fp32_impl(case, seed):
  """A correct fp32 implementation (torch-CPU, its own summation order) next to the case's fp64 candidates."""
  name, N, H, W, C, K, k, st, pad, mode, act = case
  x, w, b, gy = bc.conv_case_inputs(case, seed)
  z32 = bc.conv64(x, w, st, pad, mode) + b.view(1, -1, 1, 1)
  y32 = bc.act64(z32, act)
  y64, Sy, ny = bc.fwd_reference(x, w, b, st, pad, mode, act)
  dz = bc.dz_operand(gy, rn_bf16(y32.double()), act).float()
  dx32 = bc.dgrad64(dz, w, x.shape, st, pad, mode)
  dx64, cands, Sdx, ndx = bc.dgrad_reference(dz.double(), w.double(), x.shape, st, pad, mode)
  return dict(y=rn_bf16(y32.double()), y64=y64, Sy=Sy, ny=ny, dx=rn_bf16(dx32.double()), dx64=dx64, cands=cands,
              Sdx=Sdx, ndx=ndx, x=x, w=w, dz=dz)


@pytest.mark.parametrize('name', HEAVY)
def test_correct_fp32_implementation_passes(name):
  t0 = time.process_time()
  r = _fp32_impl(CASES[name], 0)
  _, sy = bc.assert_bf16_contract(r['y'], [Cand(r['y64'])], r['Sy'], r['ny'], name + ' fwd (torch-CPU fp32)')
  _, sd = bc.assert_bf16_contract(r['dx'], r['cands'], r['Sdx'], r['ndx'], name + ' dgrad (torch-CPU fp32)')
  print('%s: share not correctly rounded: fwd %.4f %%, dgrad %.4f %% (cap %.1f %%; CPU %.1f s)'
        % (name, 100 * sy, 100 * sd, 100 * bc.CAP, time.process_time() - t0))
  assert sy <= bc.CAP / 10 and sd <= bc.CAP / 10, 'the inputs of %s leave a correct implementation too close to the cap' % name


def test_correct_fp32_weight_gradient_passes():
  name, N, H, W, C, K, k, st, pad, mode, act = CASES['tile320_path']
  assert N * H * W == 33024
  x, w, b, gy = bc.conv_case_inputs(CASES['tile320_path'], 0)
  dw32 = bc.wgrad64(x, gy, w.shape, st, pad, mode)
  dw64 = bc.wgrad64(x.double(), gy.double(), w.shape, st, pad, mode)
  bc.assert_fp32_vs_fp64(dw32, dw64, name + ' wgrad (torch-CPU fp32)')
  bc.assert_fp32_vs_fp64(gy.sum(dim=(0, 2, 3)), gy.double().sum(dim=(0, 2, 3)), name + ' bias grad (torch-CPU fp32)')
  print('%s wgrad: max-norm %.2e, element-wise %.2e (bounds %.0e / %.0e)'
        % (name, rel_err(dw32, dw64), elem_err(dw32, dw64), RTOL[F32], ETOL[F32]))


def _old_bf16_bounds_pass(got, ref):
  e, ee = rel_err(got, ref), elem_err(got, ref)
  return e <= RTOL[BF16] and ee <= ETOL[BF16], e, ee


def _mutant_verdict(label, got, ref, check_new):
  """The mutant must pass today's bf16 comparison and fail the new criterion."""
  old_ok, e, ee = _old_bf16_bounds_pass(got, ref)
  try:
    check_new()
    new_msg = None
  except AssertionError as ex:
    new_msg = str(ex)
  print('%s: old bf16 bounds %s (max-norm %.2e, element-wise %.2e); new criterion %s'
        % (label, 'pass' if old_ok else 'FAIL', e, ee, 'fails: ' + new_msg if new_msg else 'PASSES'))
  assert old_ok, label + ': the mutant should pass the old bounds (the gap this criterion closes)'
  assert new_msg is not None, label + ': the new criterion missed the mutant'


MUTANT_CASE = 'resblock_tail'


def _fwd_parts(name):
  case = CASES[name]
  _, N, H, W, C, K, k, st, pad, mode, act = case
  x, w, b, gy = bc.conv_case_inputs(case, 0)
  y64, S, n = bc.fwd_reference(x, w, b, st, pad, mode, act)
  return case, x, w, b, y64, S, n


def _truncate_bf16(t):
  b = t.float().contiguous().view(torch.int32)
  return (b & ~0xffff).view(torch.float32).double()


def test_mutant_truncation():
  case, x, w, b, y64, S, n = _fwd_parts(MUTANT_CASE)
  _, N, H, W, C, K, k, st, pad, mode, act = case
  got = _truncate_bf16(bc.act64(bc.conv64(x, w, st, pad, mode) + b.view(1, -1, 1, 1), act))
  _mutant_verdict('truncation instead of RNE', got, y64, lambda: bc.assert_bf16_contract(got, [Cand(y64)], S, n, 'mutant'))


def test_mutant_two_rounded_halves_of_the_k_reduction():
  case, x, w, b, y64, S, n = _fwd_parts(MUTANT_CASE)
  _, N, H, W, C, K, k, st, pad, mode, act = case
  h = C // 2
  p0 = rn_bf16(bc.conv64(x[:, :h].double(), w[:, :h].double(), st, pad, mode))
  p1 = rn_bf16(bc.conv64(x[:, h:].double(), w[:, h:].double(), st, pad, mode))
  got = rn_bf16(bc.act64(p0 + p1 + b.double().view(1, -1, 1, 1), act))
  _mutant_verdict('K reduction in two bf16-rounded halves', got, y64,
                  lambda: bc.assert_bf16_contract(got, [Cand(y64)], S, n, 'mutant'))


def test_mutant_one_tap_off_by_1e_3():
  case, x, w, b, y64, S, n = _fwd_parts(MUTANT_CASE)
  _, N, H, W, C, K, k, st, pad, mode, act = case
  wm = w.double().clone()
  wm[:, :, 1, 1] *= 1.0 + 1e-3
  got = rn_bf16(bc.act64(bc.conv64(x.double(), wm, st, pad, mode) + b.double().view(1, -1, 1, 1), act))
  _mutant_verdict('one filter tap scaled by 1 + 1e-3', got, y64, lambda: bc.assert_bf16_contract(got, [Cand(y64)], S, n, 'mutant'))


def test_mutant_weight_gradient_split_rounded_to_bf16():
  case = CASES[MUTANT_CASE]
  _, N, H, W, C, K, k, st, pad, mode, act = case
  x, w, b, gy = bc.conv_case_inputs(case, 0)
  h = N // 2 + 1        # two splits of the pixel reduction along the batch; the first one's fp32 partial rounded to bf16
  p0 = bc.wgrad64(x[:h], gy[:h], w.shape, st, pad, mode)
  p1 = bc.wgrad64(x[h:], gy[h:], w.shape, st, pad, mode)
  got = (rn_bf16(p0.double()).float() + p1).double()
  ref = bc.wgrad64(x.double(), gy.double(), w.shape, st, pad, mode)
  _mutant_verdict('weight gradient with one split partial rounded to bf16', got, ref,
                  lambda: bc.assert_fp32_vs_fp64(got, ref, 'mutant'))
