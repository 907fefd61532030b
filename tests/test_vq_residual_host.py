"""Host-only checks of the residual vector quantizer: what ctu.quantizers.ResidualS2HVQ refuses without a
device, the C entry points' refusals before any launch, and the .jpdr container of ctu.utils.vqstages -- header round trip, cutting
after a stage, and every hostile field -- on blobs built on the CPU from mode-0 (packed-index) stage blobs.  Nothing here launches
a kernel."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import jpdse_hip
from jpdse_hip import F32
from ctu.quantizers import ResidualS2HVQ, S2HVQ
from ctu.utils import vqstages, vqstream


# ---- the module ---------------------------------------------------------------------------------------------------------------
def test_constructor_refusals():
  with pytest.raises(ValueError, match='stages, n_center, center_size'):
    ResidualS2HVQ(torch.zeros(4, 2))
  with pytest.raises(NotImplementedError, match='0 stages'):
    ResidualS2HVQ(torch.zeros(0, 4, 2))
  with pytest.raises(NotImplementedError, match='9 stages'):
    ResidualS2HVQ(torch.zeros(9, 4, 2))
  with pytest.raises(NotImplementedError, match='n_center 513'):
    ResidualS2HVQ(torch.zeros(2, 513, 2))
  with pytest.raises(NotImplementedError, match='n_center 1'):
    ResidualS2HVQ(torch.zeros(2, 1, 2))
  with pytest.raises(NotImplementedError, match='center_size 33'):
    ResidualS2HVQ(torch.zeros(2, 4, 33))
  with pytest.raises(NotImplementedError, match='float32'):
    ResidualS2HVQ(torch.zeros(2, 4, 2, dtype=torch.float64))
  rvq = ResidualS2HVQ(torch.zeros(8, 512, 32), sigma=3.0)
  assert rvq.n_stages == 8 and rvq.center_size == 32 and rvq.sigma == 3.0
  assert [n for n, _ in rvq.named_parameters()] == ['_code_books'] and rvq.code_books is rvq._code_books
  rvq.sigma = 5.0
  assert rvq.sigma == 5.0
  with pytest.raises(AssertionError):
    rvq.sigma = 0.0


def test_argument_checks_are_s2hvqs_and_need_no_device():
  rvq, one = ResidualS2HVQ(torch.zeros(3, 4, 2)), S2HVQ(torch.zeros(4, 2))
  for x, code_len in ((torch.zeros(5, 3), 4), (torch.zeros(5, 6), 4), (torch.zeros(5, 6), 2)):
    with pytest.raises(ValueError) as mine:
      rvq.quantize(x, code_len)
    with pytest.raises(ValueError) as theirs:
      one.quantize(x, code_len)
    assert str(mine.value) == str(theirs.value)
  with pytest.raises(NotImplementedError, match='float32 and bfloat16'):
    rvq.encode(torch.zeros(5, 4, dtype=torch.float64), 2)
  for bad in (0, 4, 1.0, True):
    with pytest.raises(ValueError, match='stages must be an int in 1 .. 3'):
      rvq.quantize(torch.zeros(5, 4), 2, stages=bad)
  with pytest.raises(ValueError, match='int64 tensor'):
    rvq.decode(torch.zeros(4, 5, 2, dtype=torch.int64))              # more stages than books
  with pytest.raises(ValueError, match='int64 tensor'):
    rvq.decode(torch.zeros(2, 5, 2, dtype=torch.int32))
  with pytest.raises(ValueError, match='n_iter'):
    rvq.fit(torch.zeros(5, 4), 2, n_iter=-1)
  with pytest.raises(ValueError, match='init'):
    rvq.fit(torch.zeros(5, 4), 2, init='kmeans++')
  with pytest.raises(ValueError, match='distinct vectors'):
    rvq.fit(torch.zeros(1, 4), 2)


def test_soft_forward_is_refused_beyond_one_stage_before_any_device_work():
  rvq = ResidualS2HVQ(torch.zeros(2, 4, 2))
  with pytest.raises(NotImplementedError, match='soft forward'):
    rvq.quantize(torch.zeros(5, 4), 2, hard_forward=False)           # CPU tensors: a device call would have raised JpdseError


# ---- the C entry points: refused on the host --------------------------------------------------------------------------------
def _refused(call, args, field):
  assert call(ctypes.byref(args)) == -1, field
  assert field in jpdse_hip.last_error(), (field, jpdse_hip.last_error())


def test_entry_points_refuse_bad_shapes_before_a_launch():
  L = jpdse_hip.lib()
  P = 0x1000                                                         # never dereferenced: every call below is refused first
  def fwd(**kw):
    v = dict(dtype=F32, M=10, D=8, L=64, S=4, n_stages=4, x=P, books=P, y=P, index=P, sse=None, residual=None, ws=None,
             ws_bytes=0, stream=None)
    v.update(kw)
    return jpdse_hip.VqResFwdArgs(**v)
  _refused(L.jpdse_vq_res_fwd, fwd(S=0), 'S = 0 stages')
  _refused(L.jpdse_vq_res_fwd, fwd(S=9, n_stages=9), 'S = 9 stages')
  _refused(L.jpdse_vq_res_fwd, fwd(n_stages=5), 'n_stages = 5')
  _refused(L.jpdse_vq_res_fwd, fwd(n_stages=-1), 'n_stages = -1')
  _refused(L.jpdse_vq_res_fwd, fwd(D=33), 'center_size D = 33')
  _refused(L.jpdse_vq_res_fwd, fwd(L=513), 'n_center L = 513')
  _refused(L.jpdse_vq_res_fwd, fwd(M=0), 'M = 0')
  _refused(L.jpdse_vq_res_fwd, fwd(M=1 << 26, L=64), 'M * L')
  _refused(L.jpdse_vq_res_fwd, fwd(dtype=7), 'bad dtype')
  _refused(L.jpdse_vq_res_fwd, fwd(x=None), 'null pointer')
  _refused(L.jpdse_vq_res_fwd, fwd(sse=P), 'workspace too small')
  def bwd(**kw):
    v = dict(dtype=F32, M=10, D=8, L=64, S=4, n_stages=4, sigma=1.0, dy=P, x=P, books=P, index=P, dx=P, dbooks=None, ws=None,
             ws_bytes=0, stream=None)
    v.update(kw)
    return jpdse_hip.VqResBwdArgs(**v)
  _refused(L.jpdse_vq_res_bwd, bwd(n_stages=0), 'n_stages = 0')
  _refused(L.jpdse_vq_res_bwd, bwd(sigma=0.0), 'sigma')
  _refused(L.jpdse_vq_res_bwd, bwd(sigma=float('nan')), 'sigma')
  _refused(L.jpdse_vq_res_bwd, bwd(index=None), 'null pointer')
  _refused(L.jpdse_vq_res_bwd, bwd(dbooks=P), 'workspace too small')
  dec = jpdse_hip.VqResDecodeArgs(dtype=F32, M=10, D=8, L=64, S=4, n_stages=0, index=P, books=P, y=P, status=P, stream=None)
  _refused(L.jpdse_vq_res_decode, dec, 'n_stages = 0')
  dec.n_stages, dec.status = 2, None
  _refused(L.jpdse_vq_res_decode, dec, 'null pointer')
  # the workspace query: 0 outside the limits, the larger of the forward's fp64 partials and the backward's fp32 partials inside
  assert L.jpdse_vq_res_workspace_size(10, 8, 64, 0) == 0 and L.jpdse_vq_res_workspace_size(10, 8, 64, 9) == 0
  assert L.jpdse_vq_res_workspace_size(10, 33, 64, 2) == 0
  assert L.jpdse_vq_res_workspace_size(10, 8, 64, 2) == 1 * 2 * 64 * 8 * 4           # one block of the backward
  big = L.jpdse_vq_res_workspace_size(1 << 20, 32, 512, 8)
  assert 0 < big <= 256 << 20                                                       # the cap on the partials


# ---- the .jpdr container -------------------------------------------------------------------------------------------------------
N, CODE_LEN, NC = 5, 3, 11


def _stage_blob(seed, n=N, code_len=CODE_LEN, L=NC):
  """A mode-0 .jpdv blob and its indices: a 4-byte table + empty streams is never smaller than the packed form here."""
  idx = np.random.RandomState(seed).randint(0, L, size=n * code_len)
  blob = vqstream.build_blob((n, code_len), L, 1, struct.pack('<I', 60) + bytes(60), idx)
  assert vqstream.parse_blob(blob)[4] == vqstream.MODE_PACKED
  return blob, idx


def _container(S=3):
  made = [_stage_blob(100 + s) for s in range(S)]
  return vqstages.build_stages([b for b, _ in made], N, CODE_LEN, NC), made


def test_container_round_trips_and_cuts_byte_for_byte():
  blob, made = _container(3)
  assert blob[:4] == b'JPDR' and vqstages.coded_bits(blob) == 8 * len(blob)
  S, n, code_len, L, blobs = vqstages.parse_stages(blob)
  assert (S, n, code_len, L) == (3, N, CODE_LEN, NC) and blobs == [b for b, _ in made]
  code = vqstages.read_stages(blob, 'cpu')                            # packed stages need no device call
  assert code.dtype == torch.int64 and tuple(code.shape) == (3, N, CODE_LEN)
  assert np.array_equal(code.numpy().reshape(3, -1), np.stack([i for _, i in made]))
  for k in (1, 2, 3):
    cut = vqstages.truncate_stages(blob, k)
    Sk, nk, ck, Lk, bk = vqstages.parse_stages(cut)
    assert (Sk, nk, ck, Lk) == (k, N, CODE_LEN, NC) and bk == [b for b, _ in made[:k]]
    assert cut == vqstages.build_stages([b for b, _ in made[:k]], N, CODE_LEN, NC)
    assert torch.equal(vqstages.read_stages(cut, 'cpu'), code[:k]) and torch.equal(vqstages.read_stages(blob, 'cpu', stages=k), code[:k])
    assert vqstages.coded_bits(blob, stages=k) == 8 * len(cut)
  assert vqstages.truncate_stages(blob, 3) == blob
  # reading a prefix does not look at the later blobs: garbage there goes unnoticed, in the prefix it does not
  at = len(blob) - len(made[2][0])
  spoiled = blob[:at] + b'XXXX' + blob[at + 4:]
  assert torch.equal(vqstages.read_stages(spoiled, 'cpu', stages=2), code[:2])
  with pytest.raises(ValueError, match='stage 2'):
    vqstages.read_stages(spoiled, 'cpu')


def _patched(blob, offset, value):
  return blob[:offset] + struct.pack('<I', value) + blob[offset + 4:]


def test_container_refuses_hostile_fields_by_name():
  blob, made = _container(3)
  first = vqstages.HEADER_BYTES + 4 * 3                               # where the first stage blob starts
  cases = [
      (b'JPDV' + blob[4:], 'not a coded stage file'),
      (_patched(blob, 4, 2), 'format version 2'),
      (_patched(blob, 8, 0), 'S = 0 stages'),
      (_patched(blob, 8, 9), 'S = 9 stages'),
      (_patched(blob, 12, 0), 'empty code shape'),
      (_patched(blob, 20, 513), 'n_center L = 513'),
      (blob[:10], 'shorter than the 24-byte header'),
      (blob[:vqstages.HEADER_BYTES + 5], 'length table'),
      (_patched(blob, vqstages.HEADER_BYTES, 3), 'length table: stage 0'),
      (_patched(blob, vqstages.HEADER_BYTES + 4, len(made[1][0]) + 1), 'truncated'),
      (blob[:-1], 'truncated'),
      (blob + b'\0', 'beyond'),
      (_patched(blob, 12, N + 1), 'stage 0: its n = 5'),               # the outer n against the inner blobs'
      (_patched(blob, 16, CODE_LEN + 1), 'stage 0: its code_len = 3'),
      (_patched(blob, 20, NC + 1), 'stage 0: its n_center = 11'),
      (_patched(blob, first + 8, N + 1), 'stage 0'),                   # an inner header that disagrees with its own body
      (_patched(blob, first, 0), 'stage 0: not a coded index file'),
  ]
  for hostile, field in cases:
    with pytest.raises(ValueError, match=field):
      vqstages.read_stages(hostile, 'cpu')
    with pytest.raises(ValueError, match=field):
      vqstages.truncate_stages(hostile, 1)
  for bad in (0, 4):
    with pytest.raises(ValueError, match='stages'):
      vqstages.truncate_stages(blob, bad)
  with pytest.raises(ValueError, match='bytes'):
    vqstages.parse_stages('not bytes')
  with pytest.raises(ValueError, match='S = 0 stages'):
    vqstages.build_stages([], N, CODE_LEN, NC)
  with pytest.raises(ValueError, match='int64'):
    vqstages.write_stages(None, torch.zeros(2, 3, dtype=torch.int64), NC)
  # a second stage of another shape: named as stage 1
  other, _ = _stage_blob(7, n=N + 1)
  mixed = vqstages.build_stages([made[0][0], other], N, CODE_LEN, NC)
  with pytest.raises(ValueError, match='stage 1: its n = 6, the container says 5'):
    vqstages.read_stages(mixed, 'cpu')
  assert torch.equal(vqstages.read_stages(mixed, 'cpu', stages=1), vqstages.read_stages(blob, 'cpu', stages=1))
