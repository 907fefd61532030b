"""The invariant the panel cache exists for (jpdse_hip/panels.py; its rule is pinned on the CPU by tests/test_panels_host.py):
whatever moved a conv filter's fp32 master -- the fused optimizer step, with or without the batched re-pack behind it, a loaded
state dict, an update behind torch's version counter announced by bump_weights_epoch() -- the panels the next kernel reads are
bit for bit what a fresh pack of that master gives.  Weights only: no activation kernel runs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import jpdse_hip
from jpdse_hip import ops, layers, F32, BF16, ACT_NONE, PAD_ZERO
from jpdse_hip.layers import HipConv2d, PackBatcher, Ctx
from jpdse_hip.optim import FusedAdam
from hip_util import DEV

LAYERS = {      # the layers of tests/test_panels_host.py (there: why the two 64 -> 64 ones)
    'cast': lambda: HipConv2d(64, 16, 3, 1, 1, dtype=BF16, device=DEV),
    'cast_T': lambda: HipConv2d(128, 64, 3, 2, 1, apply_bias=False, transposed=True, dtype=BF16, device=DEV),
    'packed_bf16': lambda: HipConv2d(39, 64, 3, 1, 1, dtype=BF16, device=DEV),
    'alias': lambda: HipConv2d(16, 8, 3, 1, 1, dtype=F32, device=DEV),
    'packed_f32': lambda: HipConv2d(39, 64, 3, 1, 1, dtype=F32, device=DEV),
    'cast_64': lambda: HipConv2d(64, 64, 3, 1, 1, dtype=BF16, device=DEV),
    'alias_64': lambda: HipConv2d(64, 64, 3, 1, 1, dtype=F32, device=DEV),
    'sliced': lambda: HipConv2d(39, 64, 4, 2, 2, PAD_ZERO, act=ACT_NONE, dtype=BF16, device=DEV),     # PatchGAN layer 0
}
ALIAS = ('alias', 'alias_64')
COVERED = ('cast_T', 'cast_64', 'alias_64')
SLICE = (36, 39)


@pytest.fixture(scope='module', autouse=True)
def _gpu():
  jpdse_hip.require_gpu(0)


def as_bytes(t):
  return t.contiguous().view(torch.uint8).reshape(-1)


def test_panels_follow_the_master(monkeypatch):
  """PackBatcher.run() covers 3 of the 8 layers -- cast_T, cast_64 and alias_64, as it did before panels.py existed: 'cast' and
  'alias' are below the 64 x 64 padded channels at which jpdse_conv_pack_entries has rows, the others have both panels to
  build."""
  real_pack, real_into = ops.conv_pack, ops.conv_pack_into
  launches = []
  monkeypatch.setattr(ops, 'conv_pack', lambda *a: launches.append('pack') or real_pack(*a))
  monkeypatch.setattr(ops, 'conv_pack_into', lambda *a: launches.append('into') or real_into(*a))
  slice_pack = []
  monkeypatch.setattr(ops, 'conv_dgrad', lambda d, dz, pack, **kw: slice_pack.append(pack))     # bwd_input_slice's last call
  torch.manual_seed(7)
  net = torch.nn.ModuleDict({name: make() for name, make in LAYERS.items()})
  opt = FusedAdam(net.parameters(), lr=2e-4)
  batcher = PackBatcher(net)
  x, dy = ops.Act.empty(1, 8, 8, 39, BF16, DEV), ops.Act.empty(1, 5, 5, 64, BF16, DEV)
  d_slice = ops.conv_desc(BF16, 1, 8, 8, SLICE[1] - SLICE[0], 64, 4, 4, 2, 2, PAD_ZERO, ACT_NONE, 0.2)

  def check_all(what, quiet=()):
    """Every layer's panels against a fresh pack of its master; `quiet`: the layers whose packs() must launch nothing."""
    for name, m in net.items():
      del launches[:]
      fwd, dgrad = m.packs()
      assert (launches == []) == (name in quiet), (what, name, launches)
      w = m.weight.detach()
      want_fwd, want_dgrad = real_pack(m._desc(1, 64, 64), w, DEV)
      if name in ALIAS:
        assert fwd.data_ptr() == w.data_ptr(), (what, name)
        fwd = w.permute(0, 2, 3, 1)                  # KRSC, the order of the memory the kernels read
      assert torch.equal(as_bytes(fwd), want_fwd), (what, name, 'forward panel')
      assert torch.equal(dgrad, want_dgrad), (what, name, 'data-gradient panel')
      del launches[:]
      m.packs()
      assert launches == [], (what, name, 'second packs()')
    m = net['sliced']
    m.bwd_input_slice(Ctx(x, None), dy, SLICE[0], SLICE[1])
    ws = m.weight.detach()[:, SLICE[0]:SLICE[1]].contiguous(memory_format=torch.channels_last)
    assert torch.equal(slice_pack[-1], real_pack(d_slice, ws, DEV)[1]), (what, 'slice panel')

  def step():
    for p in net.parameters():
      p.grad.copy_(torch.randn(p.shape, device=DEV))
    before = [p.detach().clone() for p in net.parameters()]
    opt.step()
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, net.parameters()))

  for m in net.values():
    m.ensure_grads()
  check_all('first use')
  first_slice = slice_pack[-1]
  assert batcher.run() == 0                           # nothing moved
  step()
  assert batcher.run() == len(COVERED)
  check_all('step + PackBatcher.run', quiet=COVERED)
  step()
  check_all('step alone')
  state = {k: v + 0.01 * torch.randn(v.shape, device=DEV) for k, v in net.state_dict().items()}
  net.load_state_dict(state)
  assert batcher.run() == 0                           # weights replaced: the lazy path
  check_all('load_state_dict')
  for m in net.values():
    m.weight.data.mul_(1.5)                           # behind torch's version counter ...
  layers.bump_weights_epoch()                         # ... hence announced
  check_all('bump_weights_epoch')
  assert slice_pack[-1] is first_slice                # same channel range throughout: the slice panels were re-packed in place
