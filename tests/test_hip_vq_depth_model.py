"""GPU tests of opt.vq_class_stages on the model and the trainer at the suite's small s2hvq model (nef 8, 64 x 32,
batch 2, vq_stages 3): the depth map the trainer derives, the -1 pattern of the code, the .jpdm streams and their cuts, the receiver
against get_img bit for bit, a stream against another image's labels, one train step whose books' gradient is the depth backward,
'*:3' against the field absent, the 'uniform' prefix, and the calls the field refuses."""
import numpy as np
import pytest
import torch

from jpdse_hip import ops
from jpdse_hip.layers import StageDepth
from ctu.utils import vqdepth, vqstages
from oracle.ctu_cpu import model as omodel
import vq_depth_ref as ref
from test_hip_vq_encoder import N, H, W, C, D, L, DOWN, DTYPES

pytestmark = pytest.mark.gpu
S, G, STEP, SIGMA = 3, C // D, 1 << DOWN, 10.0
SPEC = '1:3,2:2,*:1'
_shared = {}


def _trainer(dtype, seed=1234, **over):
  from ctu.trainers import get_trainer
  kw = dict(gpu_ids=[0], print_losses=False, compute_dtype=dtype, ngf=8, ndf=8, n_blocks_global=1, n_downsample_global=2,
            no_feat_encoding=False, no_encoder_binarization=False, feat_num=3, nef=8, n_downsample_E=DOWN,
            encoder_binarizer_out_channels=C, encoder_quantizer='s2hvq', vq_n_center=L, vq_center_size=D, vq_sigma=SIGMA,
            no_vgg_loss=True, no_gan_feat_loss=True, no_g_gan_loss=True, no_d_gan_loss=True, skip_unused_losses=True, vq_stages=S)
  kw.update(over)
  opt = omodel.default_opt(**kw)
  torch.manual_seed(seed)
  tr = get_trainer(opt)(opt, 'train')
  with torch.no_grad():      # books at the scale of the bottleneck's features, so that more than one centre is in use
    tr.model.netE._vq.vq._code_books.mul_(0.05)
  return tr


def _batch(seed=3, shift=0):
  """The suite's synthetic batch with a label map of three regions: class 1 (depth 3), class 2 (depth 2), class 5 and one pixel
  outside the table (depth 1).  `shift` moves the borders: another image's labels, other per-stage counts."""
  xd = omodel.synthetic_batch(N, H, W, seed=seed)
  lab = torch.full((N, 1, H, W), 5.0)
  lab[:, :, :24 + shift, :] = 1.0
  lab[:, :, 24 + shift:40, :14] = 2.0                          # a border inside a cell: the maximum rule decides
  lab[1, 0, H - 1, W - 1] = 77.0
  xd['label'] = lab
  return xd


def _table():
  n = omodel.default_opt().num_labels
  t = np.ones(n + 1, dtype=np.int64)
  t[1], t[2] = 3, 2
  return t


def _pair(dtype):
  if dtype not in _shared:
    tr = _trainer(dtype, vq_class_stages=SPEC)
    xd = _batch()
    tr.eval()
    _shared[dtype] = (tr, xd, tr.get_img(xd).clone())
  return _shared[dtype]


@pytest.mark.parametrize('dtype', DTYPES)
def test_depth_code_streams_and_receiver(dtype):
  tr, xd, img = _pair(dtype)
  depth = tr.get_stage_depth(xd)
  n_classes = len(tr.model.codec.class_stages[0])
  want = ref.depth_map(xd['label'].numpy(), _table()[:n_classes], 1, STEP)
  assert depth.dtype == torch.int64 and tuple(depth.shape) == (N, H // STEP, W // STEP)
  assert np.array_equal(depth.cpu().numpy(), want) and sorted(set(want.reshape(-1).tolist())) == [1, 2, 3]
  code = tr.get_vq_code(xd)
  assert tuple(code.shape) == (N, S, want[0].size * G)
  per_index = torch.from_numpy(want).view(N, 1, -1).repeat_interleave(G, dim=2).to(code.device)
  past = torch.arange(S, device=code.device).view(1, S, 1) >= per_index
  assert torch.equal(code == -1, past) and bool(((code >= 0) & (code < L))[~past].all())
  blobs = tr.get_coded(xd)
  for j, b in enumerate(blobs):
    assert b[:4] == b'JPDM'
    counts = vqdepth.parse_depth_stages(b, depth=want[j])[4]
    assert sum(counts) * G == G * int(want[j].sum()) and counts == vqdepth.stage_counts(want[j], S)
    with pytest.raises(ValueError, match='not a coded stage file'):
      vqstages.parse_stages(b)
  assert torch.equal(tr.decode(code, xd), img)
  assert torch.equal(tr.decode_coded(blobs, xd), img)
  receiver = {'label': xd['label'], 'instance': xd['instance']}
  assert torch.equal(tr.decode_coded(blobs, receiver), img)
  coded, raw = tr.get_coded_rate(xd)
  assert coded == sum(8.0 * len(b) for b in blobs) / (N * H * W) and raw > 0
  report = tr.get_depth_report(xd)
  for j, row in enumerate(report):
    assert row['cells'] == [int((want[j] == v).sum()) for v in (1, 2, 3)] and row['total_bytes'] == len(blobs[j])
    assert row['indices'] == [G * c for c in vqdepth.stage_counts(want[j], S)] and row['bpp'] == 8.0 * len(blobs[j]) / (H * W)
    assert sum(row['bytes']) + 24 + 8 * S == len(blobs[j])


@pytest.mark.parametrize('dtype', DTYPES)
def test_a_cut_stream_is_the_model_at_the_clamped_depth(dtype):
  tr, xd, img = _pair(dtype)
  code, blobs = tr.get_vq_code(xd), tr.get_coded(xd)
  vq = tr.model.netE._vq
  for keep in (1, 2):
    cut = [vqdepth.truncate_depth_stages(b, keep) for b in blobs]
    a = tr.decode_coded(cut, xd)
    assert torch.equal(a, tr.decode(code[:, :keep].contiguous(), xd))
    assert torch.equal(tr.get_vq_code(xd, stages=keep), code[:, :keep])
    # the model run with min(depth, keep): the eval forward at that stage count under the same map.  get_img has no public
    # stage argument (an eval forward always takes every stage), so the layer's fwd is forced to `keep` for this one call: the
    # check is of the receiver (the cut stream, the code prefix) against the ENCODER's own forward at that depth
    inner = vq.fwd
    vq.fwd = lambda x, stages=None: inner(x, keep)
    try:
      want = tr.get_img(xd)
    finally:
      del vq.fwd
    assert torch.equal(a, want) and not torch.equal(a, img)


@pytest.mark.parametrize('dtype', DTYPES)
def test_another_images_labels_are_refused_on_the_host(dtype):
  tr, xd, _ = _pair(dtype)
  blobs = tr.get_coded(xd)
  other = _batch(shift=8)
  calls = []
  inner = tr.model.netE.decode_vq_code
  tr.model.netE.decode_vq_code = lambda *a, **k: calls.append(1) or inner(*a, **k)
  try:
    with pytest.raises(ValueError, match='count table: stage 1 codes .* the depth map implies'):
      tr.decode_coded(blobs, {'label': other['label'], 'instance': other['instance']})
  finally:
    del tr.model.netE.decode_vq_code
  assert not calls


def _spied_step(tr, xd):
  vq = tr.model.netE._vq
  seen = []
  inner = vq.bwd

  def spy(ctx, dy, need_dx=True, need_dw=True):
    seen.append((ctx.items[1].t.clone(), ctx.items[2].clone(), ctx.items[3] if len(ctx.items) > 3 else None, dy.t.clone(),
                 vq.vq._code_books.detach().clone()))
    return inner(ctx, dy, need_dx, need_dw)

  vq.bwd = spy
  try:
    tr.step(xd)
  finally:
    del vq.bwd
  torch.cuda.synchronize()
  assert len(seen) == 1
  return seen[0]


@pytest.mark.parametrize('dtype', DTYPES)
def test_one_train_step_is_the_depth_backward(dtype):
  tr = _trainer(dtype, vq_class_stages=SPEC)
  xd = _batch()
  h, index, extra, dy, books = _spied_step(tr, xd)
  assert isinstance(extra, StageDepth) and tr.model.netE._vq.depth is None, 'the map travels with the context and is unset after the call'
  n_classes = len(tr.model.codec.class_stages[0])
  want = ref.depth_map(xd['label'].numpy(), _table()[:n_classes], 1, STEP).reshape(-1)
  assert np.array_equal(extra.depth.cpu().numpy(), want)
  for k, v in tr.last_losses.items():
    assert v == v and abs(v) != float('inf'), (k, v)
  want_y, want_index = ops.vq_res_rows_fwd(h.view(-1, D), books, S, depth=extra.depth, groups=G)
  assert torch.equal(index, want_index) and bool((index == -1).any())
  _, dc = ops.vq_res_bwd(dy.view(-1, D), h.view(-1, D), books, index, SIGMA, want_dx=False, groups=G, depth=extra.depth)
  grad = tr.model.netE._vq.vq._code_books.grad
  assert torch.equal(grad, dc) and float(grad.abs().max()) > 0


@pytest.mark.parametrize('dtype', DTYPES)
def test_star_at_full_depth_is_the_field_absent(dtype):
  xd = _batch()
  out = []
  for over in (dict(vq_class_stages='*:3'), {}):
    tr = _trainer(dtype, **over)
    h, index, extra, dy, books = _spied_step(tr, xd)
    vq = tr.model.netE._vq
    tr.eval()
    out.append((dict(tr.last_losses), vq.vq._code_books.grad.clone(), vq.conv.weight.grad.clone(), h, index, dy, tr.get_img(xd),
                [len(b) for b in tr.get_coded(xd)], extra))
  a, b = out
  assert isinstance(a[8], StageDepth) and b[8] is None
  assert a[0] == b[0] and all(torch.equal(a[i], b[i]) for i in range(1, 7))
  # payload sizes aside from the container header: .jpdm carries one more table of S counts than .jpdr
  assert a[7] == [n + 4 * S for n in b[7]]


@pytest.mark.parametrize('dtype', DTYPES)
def test_uniform_schedule_takes_the_smaller_of_depth_and_draw(dtype):
  tr = _trainer(dtype, vq_train_stages='uniform', vq_class_stages=SPEC)
  xd = _batch()
  vq = tr.model.netE._vq
  draw = lambda t: 1 + int(torch.randint(S, (1,), generator=torch.Generator().manual_seed(tr.model.codec_seed * 1000003 + t)))
  for n in (1, 2):
    t = next(t for t in range(100) if draw(t) == n)
    tr.model.codec_draw = t
    h, index, extra, dy, books = _spied_step(tr, xd)
    assert vq.train_stages == n and tuple(index.shape)[0] == n
    _, want_index = ops.vq_res_rows_fwd(h.view(-1, D), books, n, depth=extra.depth.clamp(max=n), groups=G)
    assert torch.equal(index, want_index)
    grad = vq.vq._code_books.grad
    assert grad.ne(0).any(dim=2).any(dim=1).cpu().tolist() == [s < n for s in range(S)], (t, n)


def test_the_field_refuses_what_has_no_depth_form():
  tr, xd, _ = _pair('fp32')
  for call in (lambda: tr.get_stage_code_ec(xd, 0.1), lambda: tr.get_coded_stages_ec(xd, 0.1), lambda: tr.get_stage_usage(xd),
               lambda: tr.get_stage_rates(xd), lambda: tr.get_stage_curve(xd, rate_lambda=0.1)):
    with pytest.raises(ValueError, match='not available with opt.vq_class_stages'):
      call()
  with pytest.raises(ValueError, match='rate_lambda > 0'):
    tr.get_vq_code(xd, rate_lambda=0.1)
  for over, text in ((dict(vq_class_stages='1:4'), 'outside 1 .. vq_stages = 3'), (dict(vq_class_stages='1;2'), 'malformed entry'),
                     (dict(vq_class_stages='*:1', vq_stages=1), 'it needs'), (dict(vq_class_stages='*:1', lambda_vq_stage_rate=0.5), 'lambda_vq_stage_rate > 0'),
                     (dict(vq_class_stages='*:1', zero_sem=True), '--zero_sem')):
    with pytest.raises(ValueError) as err:
      _trainer('fp32', **over)
    assert text in str(err.value) and 'vq_class_stages' in str(err.value)
  plain = _trainer('fp32')
  for call in (plain.get_stage_depth, plain.get_depth_report):
    with pytest.raises(ValueError, match='needs opt.vq_class_stages'):
      call(xd)


@pytest.mark.parametrize('dtype', DTYPES)
def test_eval_calls_run_under_the_map(dtype):
  tr, xd, img = _pair(dtype)
  loss = float(tr.get_eval_loss(xd))
  assert loss == loss and abs(loss) != float('inf')
  full = _trainer(dtype)                                       # the same weights without the field: another image
  full.eval()
  assert not torch.equal(full.get_img(xd), img)
  # the metrics and the stage curve need MS-SSIM's 176 pixels: one 192 x 192 image through the same model
  big = omodel.synthetic_batch(1, 192, 192, seed=5)
  lab = torch.full((1, 1, 192, 192), 5.0)
  lab[:, :, :64, :] = 1.0
  lab[:, :, 64:128, :90] = 2.0
  big['label'] = lab
  m = tr.get_eval_metrics(big, per_class=True)
  assert m['l1'] == m['l1'] and 'per_class' in m
  blobs = tr.get_coded(big)
  curve = tr.get_stage_curve(big)
  assert [r['stages'] for r in curve] == [1, 2, 3] and curve[0]['bpp'] < curve[1]['bpp'] < curve[2]['bpp']
  for keep in (1, 2, 3):
    assert curve[keep - 1]['bpp'] == 8.0 * len(vqdepth.truncate_depth_stages(blobs[0], keep)) / (192 * 192)
  assert abs(curve[2]['l1'] - m['l1']) <= 1e-9 * max(1.0, abs(m['l1']))
