"""GPU tests of the entropy-constrained residual code through the model and the trainer: get_stage_code_ec,
get_coded_stages_ec, get_stage_ec_report, get_stage_usage, get_stage_rates and get_stage_curve(rate_lambda=).  The small
trainer of test_hip_vq_res_bottleneck.py -- ngf 8, nef 8, two down-samplings, 64 x 128 images, batch 2, 16 channels in vectors
of 8, 16 centres -- at three stages, fp32 and bf16."""
import pytest
import torch

from ctu.utils import vqstages
from oracle.ctu_cpu import model as omodel
import test_hip_vq_res_bottleneck as base
import vq_res_ec_ref as ref

pytestmark = pytest.mark.gpu
N, H, W, C, D, L, S = base.N, base.H, base.W, base.C, base.D, base.L, base.S
G, CODE_LEN = C // D, base.CODE_LEN
LAM = 0.002                # at the scale of the books (0.05): a few bits of length against squared distances of about 1e-2
DTYPES = base.DTYPES


def _pair(dtype):
  tr, xd, _ = base._pair(dtype)
  return tr, xd, {'label': xd['label'], 'instance': xd['instance']}


def _usage_of(code):
  """int64 [S', G, L] of a code [N, S', indices]: index i of an image belongs to channel group i % G."""
  g = (torch.arange(code.shape[2], device=code.device) % G).view(1, -1).expand(code.shape[0], -1).reshape(-1)
  return torch.stack([torch.bincount(g * L + code[:, s].reshape(-1), minlength=G * L).view(G, L) for s in range(code.shape[1])])


@pytest.mark.parametrize('dtype', DTYPES)
def test_zero_lambda_is_the_plain_code(dtype):
  tr, xd, _ = _pair(dtype)
  plain = tr.get_vq_code(xd)
  code = tr.get_stage_code_ec(xd, 0.0)
  assert code.dtype == torch.int64 and code.is_cuda and tuple(code.shape) == (N, S, CODE_LEN) and torch.equal(code, plain)
  assert torch.equal(tr.get_stage_code_ec(xd, LAM, n_iter=0), plain)
  assert tr.get_coded_stages_ec(xd, 0.0) == tr.get_coded(xd)


@pytest.mark.parametrize('dtype', DTYPES)
def test_ec_code_files_decode_and_prefixes(dtype):
  tr, xd, receiver = _pair(dtype)
  code = tr.get_stage_code_ec(xd, LAM)
  assert tuple(code.shape) == (N, S, CODE_LEN) and not torch.equal(code, tr.get_vq_code(xd))
  img = tr.decode(code, receiver)
  blobs = tr.get_coded_stages_ec(xd, LAM)
  assert len(blobs) == N and all(isinstance(b, bytes) and vqstages.parse_stages(b)[:4] == (S, 1, CODE_LEN, L) for b in blobs)
  assert torch.equal(tr.decode_coded(blobs, receiver), img)
  for n in (1, 2):                                     # the prefix property through the model, the files and the receiver
    code_n = tr.get_stage_code_ec(xd, LAM, stages=n)
    assert torch.equal(code_n, code[:, :n])
    cut = [vqstages.truncate_stages(b, n) for b in blobs]
    assert tr.get_coded_stages_ec(xd, LAM, stages=n) == cut
    assert torch.equal(tr.decode_coded(cut, receiver), tr.decode(code[:, :n].contiguous(), receiver))
  reports = tr.get_stage_ec_report(xd, LAM)
  assert len(reports) == N
  for i, rep in enumerate(reports):                    # per image: the last round's bits are the entropy of that image's code
    assert all(len(rep[k]) == 3 for k in ('distortion', 'bits', 'cost')) and all(len(r) == S for r in rep['bits'] + rep['distortion'])
    want = ref.entropy_bits(_usage_of(code[i:i + 1]).cpu()).tolist()
    assert rep['bits'][-1] == pytest.approx(want, rel=1e-12)
  assert [r['bits'] for r in tr.get_stage_ec_report(xd, LAM, stages=2)] == [[row[:2] for row in r['bits']] for r in reports]


@pytest.mark.parametrize('dtype', DTYPES)
def test_stage_usage_and_rates(dtype):
  tr, xd, _ = _pair(dtype)
  code = tr.get_vq_code(xd)
  usage = tr.get_stage_usage(xd)
  assert usage.dtype == torch.int64 and usage.is_cuda and tuple(usage.shape) == (S, G, L)
  assert torch.equal(usage.sum(2), torch.full((S, G), N * CODE_LEN // G, dtype=torch.int64, device=usage.device))
  assert torch.equal(usage, _usage_of(code))
  rates = tr.get_stage_rates(xd)
  want = (ref.entropy_bits(usage.cpu()) / (N * H * W)).tolist()
  assert isinstance(rates, list) and len(rates) == S and all(isinstance(r, float) for r in rates)
  assert rates == pytest.approx(want, rel=1e-12) and all(r > 0 for r in rates)


@pytest.mark.parametrize('dtype', DTYPES)
def test_stage_curve_of_the_ec_code(dtype):
  """On 192 x 256 images, as test_stage_curve: MS-SSIM's five scales need a shorter side of 176."""
  tr, _, _ = _pair(dtype)
  Hc, Wc = 192, 256
  xd = omodel.synthetic_batch(N, Hc, Wc, seed=5)
  code = tr.get_vq_code(xd)                            # the parent's rows, rebuilt from the calls the parent had
  blobs = tr.get_coded(xd)
  parent = []
  for n in range(1, S + 1):
    m = tr.get_eval_metrics_decoded(code[:, :n].contiguous(), xd)
    bpp = sum(8.0 * len(vqstages.truncate_stages(b, n)) / (Hc * Wc) for b in blobs) / N
    parent.append(dict(stages=n, bpp=bpp, l1=m['l1'], mse=m['mse'], psnr=m['psnr'], ms_ssim=m['ms_ssim']))
  assert tr.get_stage_curve(xd) == parent == tr.get_stage_curve(xd, rate_lambda=0.0, n_iter=2)
  rows = tr.get_stage_curve(xd, rate_lambda=LAM)
  ec = tr.get_coded_stages_ec(xd, LAM)
  assert [r['stages'] for r in rows] == [1, 2, 3] and all(sorted(r) == sorted(parent[0]) for r in rows)
  for r in rows:
    assert r['bpp'] == sum(8.0 * len(vqstages.truncate_stages(b, r['stages'])) / (Hc * Wc) for b in ec) / N
  assert rows != parent
