"""Residual (multi-stage) soft-to-hard vector quantizer on the jpdse_vq_res_* kernels (an extension: the
reference has one stage).

S code books C_1 .. C_S of L centres each.  Stage s quantizes what the stages before left over:

    r_1 = x;  k_s = argmin_k |r_s - C_s[k]|^2;  r_{s+1} = r_s - C_s[k_s];  y^(n) = C_1[k_1] + .. + C_n[k_n]

so S stages of L centres address L^S reproduction points for S times the score loop of one, and a stored code (k_1 .. k_S) can be
cut after any stage: the first n stages reproduce y^(n) (ctu.utils.vqstages).  The gradient is the soft form's at every stage (the
straight-through rule of S2HVQ.quantize), whatever the forward was.  There is no CPU path.  Limits: 1 <= S <= 8, and S2HVQ's for
center_size, n_center and n * code_len * n_center.
"""
import torch
import torch.nn as nn

from jpdse_hip import ops
from .s2h_vq import S2HVQ, MAX_CENTER_SIZE, MAX_N_CENTER, _on_gpu, _rows_limit, _ec_lambda, _ec_iterations

__all__ = ['ResidualS2HVQ']

MAX_STAGES = ops.VQ_RES_MAX_STAGES


class _ResidualQuantize(torch.autograd.Function):
  """(y, index) of ops.vq_res_rows_fwd (vq_res_fwd's bits) over the first `stages` books; backward:
  ops.vq_res_bwd from the saved x, books and indices.  The books beyond `stages` get a zero gradient."""

  @staticmethod
  def forward(ctx, x, books, sigma, stages, depth=None, groups=1):
    x, books = x.contiguous(), books.contiguous()
    y, index = ops.vq_res_rows_fwd(x, books, stages, depth=depth, groups=groups)
    ctx.save_for_backward(x, books, index)
    ctx.sigma, ctx.depth, ctx.groups = sigma, depth, groups
    ctx.mark_non_differentiable(index)
    return y, index

  @staticmethod
  def backward(ctx, dy, _dindex):
    x, books, index = ctx.saved_tensors
    if ctx.depth is None:
      dx, dc = ops.vq_res_bwd(dy.contiguous(), x, books, index, ctx.sigma, want_dx=ctx.needs_input_grad[0],
                              want_dc=ctx.needs_input_grad[1])
    else:                                        # the per-row recursion of DESIGN.md 4.27
      dx, dc = ops.vq_res_bwd(dy.contiguous(), x, books, index, ctx.sigma, want_dx=ctx.needs_input_grad[0],
                              want_dc=ctx.needs_input_grad[1], groups=ctx.groups, depth=ctx.depth)
    return dx, dc, None, None, None, None


class _ResidualRate(torch.autograd.Function):
  """rate fp32 [1] of ops.vq_res_rate_fwd over the first `stages` books; backward: ops.vq_res_bwd(groups, dhist)
  with dy = 0 on the indices of ops.vq_res_rows_fwd, dhist scaled by the incoming gradient.  The books beyond `stages` get a zero
  gradient."""

  @staticmethod
  def forward(ctx, x, books, sigma, groups, denom, stages):
    x, books = x.contiguous(), books.contiguous()
    rate, _, _, dhist, _, index = ops.vq_res_rate_fwd(x, books, sigma, groups, denom, 1.0, n_stages=stages, want_code=True)
    ctx.save_for_backward(x, books, index, dhist)
    ctx.sigma, ctx.groups = sigma, groups
    return rate

  @staticmethod
  def backward(ctx, drate):
    x, books, index, dhist = ctx.saved_tensors
    # The softmax backward sees dp only through dp - <p, dp>: a constant added to a row of dhist changes nothing.  With dy = 0 the
    # rows ARE dp, and on near-uniform histograms they are a large common value plus a small variation that carries the whole
    # gradient; fp32 would lose it under the common value, so the row means are taken out first.
    dhist = dhist - dhist.mean(dim=-1, keepdim=True)
    dx, dc = ops.vq_res_bwd(torch.zeros_like(x), x, books, index, ctx.sigma, want_dx=ctx.needs_input_grad[0],
                            want_dc=ctx.needs_input_grad[1], groups=ctx.groups,
                            dhist=(dhist * drate.to(torch.float32).reshape(())).contiguous())
    return dx, dc, None, None, None, None


class ResidualS2HVQ(nn.Module):
  """code_books: float32 tensor [S, n_center, center_size], learnable (parameter `_code_books`); sigma > 0: the hardness of the
  soft assignment whose gradient training uses."""

  def __init__(self, code_books, sigma=10., **kwargs):
    super(ResidualS2HVQ, self).__init__()
    assert sigma > 0, "sigma must be greater than 0, got {}".format(sigma)
    if code_books.dim() != 3:
      raise ValueError('code_books must have shape (stages, n_center, center_size), got {}'.format(tuple(code_books.shape)))
    stages, n_center, center_size = (int(v) for v in code_books.shape)
    if not 1 <= stages <= MAX_STAGES:
      raise NotImplementedError('ResidualS2HVQ: %d stages, the kernels take 1 .. %d' % (stages, MAX_STAGES))
    if not 1 <= center_size <= MAX_CENTER_SIZE:
      raise NotImplementedError('ResidualS2HVQ: center_size %d, the kernels take 1 .. %d' % (center_size, MAX_CENTER_SIZE))
    if not 2 <= n_center <= MAX_N_CENTER:
      raise NotImplementedError('ResidualS2HVQ: n_center %d, the kernels take 2 .. %d' % (n_center, MAX_N_CENTER))
    if code_books.dtype != torch.float32:
      raise NotImplementedError('ResidualS2HVQ: %s code books, the kernels keep them in float32' % (code_books.dtype,))
    self._center_size = center_size
    self._code_books = nn.Parameter(code_books)
    self._sigma = sigma

  @property
  def center_size(self):
    return self._center_size

  @property
  def code_books(self):
    return self._code_books

  @property
  def n_stages(self):
    return int(self._code_books.size(0))

  @property
  def sigma(self):
    return self._sigma

  @sigma.setter
  def sigma(self, new_sigma):
    assert new_sigma > 0, "sigma must be greater than 0, got {}".format(new_sigma)
    self._sigma = new_sigma

  @property
  def code_book(self):
    """The first stage's book: what S2HVQ's argument checks measure x against (every stage has its shape)."""
    return self._code_books[0]

  _vector_checks = S2HVQ._vector_checks        # the code_len checks are S2HVQ's, word for word

  def _stages(self, stages):
    n = self.n_stages if stages is None else stages
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= self.n_stages:
      raise ValueError('stages must be an int in 1 .. {}, got {!r}'.format(self.n_stages, stages))
    return n

  def _vectors(self, x, code_len):
    self._vector_checks(x, code_len)
    _on_gpu(x, 'x')
    _on_gpu(self._code_books, 'the code books')
    return x.contiguous().view(x.size(0) * code_len, self._center_size)

  def _depth(self, depth, groups, M):
    """(depth int32 [M / groups] contiguous or None, groups) of a depth= / groups= pair, checked on the host."""
    if depth is None:
      if groups != 1:
        raise ValueError('groups is the number of vectors of a depth cell: it comes with depth=, got groups = {!r} alone'.format(groups))
      return None, 1
    if isinstance(groups, bool) or not isinstance(groups, int) or groups < 1 or M % groups != 0:
      raise ValueError('groups must be an int that divides n * code_len = {}, got {!r}'.format(M, groups))
    if not torch.is_tensor(depth) or depth.dtype not in (torch.int32, torch.int64) or depth.numel() != M // groups:
      raise ValueError('depth must be an int32 or int64 tensor of n * code_len / groups = {} cells, got {}'.format(
          M // groups, (depth.dtype, tuple(depth.shape)) if torch.is_tensor(depth) else type(depth).__name__))
    return depth.reshape(-1).to(torch.int32).contiguous(), groups      # a map on the CPU fails ops' device check with x's

  def quantize(self, x, code_len, stages=None, hard_forward=True, depth=None, groups=1):
    """x [n, d], code_len dividing d with d // code_len == center_size -> (y [n, d] in x's dtype, code int64 [S', n, code_len]) of
    the first `stages` (default: all) stages, in one kernel.  Training mode: differentiable in x and the books, the gradient
    the soft form's at every stage; books beyond `stages` get a zero gradient.  Eval mode: nothing saved.  The soft forward
    exists for one stage only (there it is S2HVQ.quantize's): with more it raises NotImplementedError before any device work.
    depth / groups: depth an int tensor of n * code_len / groups cells, values 1 .. S (clamped); vector m of the
    [n * code_len, center_size] matrix lies in cell m // groups and takes its first min(stages, depth) stages; code is -1 past a
    vector's depth and the gradient is the per-row recursion's.  Hard forward only."""
    n_st = self._stages(stages)
    depth, groups = self._depth(depth, groups, x.size(0) * code_len if torch.is_tensor(x) and x.dim() == 2 else 0)
    if depth is not None and not hard_forward:
      raise NotImplementedError('ResidualS2HVQ.quantize: a depth map goes with the hard forward only')
    if not hard_forward and self.n_stages > 1:
      raise NotImplementedError('ResidualS2HVQ.quantize: the soft forward is built for one stage, this module has %d' % self.n_stages)
    xm = self._vectors(x, code_len)
    n = x.size(0)
    if not hard_forward:
      y, code, _ = S2HVQ.quantize(self, x, code_len, hard_forward=False)
      return y, code.unsqueeze(0)
    if self.training and torch.is_grad_enabled():
      y, index = _ResidualQuantize.apply(xm, self._code_books, float(self._sigma), n_st, depth, groups)
    else:
      y, index = ops.vq_res_rows_fwd(xm.detach(), self._code_books.detach().contiguous(), n_st, depth=depth, groups=groups)
    return y.view(n, code_len * self._center_size), index.to(torch.int64).view(n_st, n, code_len)

  def rate(self, x, code_len, groups=1, denom=None, stages=None):
    """The rate term of the first `stages` (default: all) stages on per-group histograms: x [n, d] as in
    quantize; vector m of the [n * code_len, center_size] matrix belongs to group m % groups (groups must divide n * code_len).
    Returns the 0-dim float32 sum over the stages s of -sum_g sum_k hist[s][g][k] log2(hist[s][g][k] / (M / groups)) / denom, hist[s]
    the per-group sums of the soft assignment of the residual r_s that the hard forward hands to stage s; denom defaults to M =
    n * code_len: bits per vector.  Differentiable in x and the books when gradients are enabled: p_s is evaluated at the hard
    residual and differentiates through the soft chain of quantize's surrogate; books beyond `stages` get a zero gradient.  [M,
    n_center] is never stored.  With one stage it is S2HVQ.rate's value."""
    n_st = self._stages(stages)
    self._vector_checks(x, code_len)
    M, groups, L = x.size(0) * code_len, int(groups), int(self._code_books.size(1))
    if groups < 1 or M % groups != 0:
      raise ValueError('groups must divide n * code_len, got {} and {}'.format(groups, M))
    if n_st * groups * L > 65536:
      raise NotImplementedError('ResidualS2HVQ.rate: stages * groups * n_center = %d, the kernels take at most 65536' % (n_st * groups * L))
    denom = float(M if denom is None else denom)
    if not (denom > 0 and denom != float('inf')):
      raise ValueError('denom must be a finite number > 0, got {}'.format(denom))
    xm = self._vectors(x, code_len)      # every refusal above needs no device
    if torch.is_grad_enabled() and (xm.requires_grad or self._code_books.requires_grad):
      return _ResidualRate.apply(xm, self._code_books, float(self._sigma), groups, denom, n_st).reshape(())
    value = ops.vq_res_rate_fwd(xm.detach(), self._code_books.detach().contiguous(), float(self._sigma), groups, denom,
                                n_stages=n_st, want_grad=False)[0]
    return value.reshape(())

  def encode(self, x, code_len, stages=None, depth=None, groups=1):
    """The int64 code [S', n, code_len] of x [n, d]; with depth / groups (see quantize) -1 past a vector's depth.  Nothing is
    differentiable."""
    n_st = self._stages(stages)
    depth, groups = self._depth(depth, groups, x.size(0) * code_len if torch.is_tensor(x) and x.dim() == 2 else 0)
    with torch.no_grad():
      xm = self._vectors(x, code_len).detach()
      _, index = ops.vq_res_rows_fwd(xm, self._code_books.detach().contiguous(), n_st, depth=depth, groups=groups)
    return index.to(torch.int64).view(n_st, x.size(0), code_len)

  def _ec_groups(self, who, x, code_len, groups, n_st):
    """groups as an int after S2HVQ.encode_ec's checks, and the table limit n * groups * n_center <= 65536 of DESIGN.md 4.25."""
    M, groups, L = x.size(0) * code_len, int(groups), int(self._code_books.size(1))
    if groups < 1 or M % groups != 0:
      raise ValueError('groups must divide n * code_len, got {} and {}'.format(groups, M))
    if n_st * groups * L > 65536:
      raise NotImplementedError('ResidualS2HVQ.%s: stages * groups * n_center = %d, the kernels take at most 65536'
                                % (who, n_st * groups * L))
    return groups

  def encode_ec(self, x, code_len, lam, groups=1, n_iter=2, stages=None):
    """Entropy-constrained encoding of the first `stages` (default: all) stages: S2HVQ.encode_ec's rounds with
    every stage assigned in one kernel (ops.vq_res_ec_assign).  Stage s of vector m takes the centre that minimises |r_s - C_s[k]|^2
    + lam * len[s][g][k], g = m % groups, len[s][g][k] = log2(n_g / hist[s][g][k]) the code length of centre k under the histogram
    of group g's own stage-s code, and hands r_s minus that centre to stage s + 1.  Round 0 assigns with no bias (the plain code,
    encode(x, code_len, stages)); round t = 1 .. n_iter takes the lengths of every (stage, group) plane from the histograms of
    round t - 1 (ops.vq_ec_lengths) and assigns all stages again.  The decoder is untouched: the result is an ordinary code, and
    its first n' stages are encode_ec(.., stages=n')'s.
    Returns (code int64 [stages, n, code_len], report): report['distortion'][t][s] the summed squared error after stage s of round
    t, report['bits'][t][s] the ideal length of stage s's code under its own per-group histograms, report['cost'][t] =
    distortion[t][-1] + lam * sum(bits[t]); n_iter + 1 rows each, read back once, at the end.  Only stage 1 has ECVQ's guarantee
    (its own cost does not rise over the rounds, up to the fp32 rounding of the scores): a later stage sees another residual every
    round, and nothing monotone holds for it or for the total.  lam == 0 or n_iter == 0: the plain code, index for index.  Runs
    under no_grad: nothing is differentiable."""
    lam = _ec_lambda(lam)
    n_iter = _ec_iterations(n_iter)
    n_st = self._stages(stages)
    self._vector_checks(x, code_len)
    groups = self._ec_groups('encode_ec', x, code_len, groups, n_st)
    L = int(self._code_books.size(1))
    with torch.no_grad():
      xm = self._vectors(x, code_len).detach()
      books = self._code_books.detach().contiguous()
      _, index, hist, sse = ops.vq_res_ec_assign(xm, books, None, groups, n_st, want_y=False)
      dist, bits = [sse.sum(1)], []
      for _ in range(n_iter):
        bias, b = ops.vq_ec_lengths(hist.view(n_st * groups, L), lam)
        bits.append(b.view(n_st, groups).sum(1))
        _, index, hist, sse = ops.vq_res_ec_assign(xm, books, bias.view(n_st, groups, L), groups, n_st, want_y=False)
        dist.append(sse.sum(1))
      bits.append(ops.vq_ec_lengths(hist.view(n_st * groups, L), lam)[1].view(n_st, groups).sum(1))
      back = torch.stack(dist + bits).cpu().tolist()
    dist = [[float(v) for v in row] for row in back[:n_iter + 1]]
    bits = [[float(v) for v in row] for row in back[n_iter + 1:]]
    report = dict(distortion=dist, bits=bits, cost=[d[-1] + lam * sum(b) for d, b in zip(dist, bits)])
    return index.to(torch.int64).view(n_st, x.size(0), code_len), report

  def usage(self, x, code_len, groups=1, stages=None):
    """int64 [stages, groups, n_center] on the device: how often the plain code of x (encode) uses every centre of every stage, per
    group m % groups -- one round of ops.vq_res_ec_assign without a bias.  A zero column is a dead centre of that stage."""
    n_st = self._stages(stages)
    self._vector_checks(x, code_len)
    groups = self._ec_groups('usage', x, code_len, groups, n_st)
    with torch.no_grad():
      xm = self._vectors(x, code_len).detach()
      _, _, hist, _ = ops.vq_res_ec_assign(xm, self._code_books.detach().contiguous(), None, groups, n_st, want_y=False)
    return hist.to(torch.int64)

  def decode(self, code, stages=None, depth=None, groups=1):
    """code int64 [S', n, code_len] -> float32 [n, code_len * center_size]: the sum of the centres of the first `stages` (default:
    all S') stages, bit for bit quantize's y.  ValueError for an index outside [0, n_center) (this synchronises).
    depth / groups (see quantize): vector m sums its first min(stages, depth) centres; what the code holds past a vector's depth
    is neither read nor checked."""
    if not torch.is_tensor(code) or code.dim() != 3 or code.dtype != torch.int64 or not 1 <= code.size(0) <= self.n_stages:
      raise ValueError('code must be an int64 tensor (stages <= {}, n, code_len), got {}'.format(
          self.n_stages, (code.dtype, tuple(code.shape)) if torch.is_tensor(code) else type(code).__name__))
    n_st = code.size(0) if stages is None else stages
    if isinstance(n_st, bool) or not isinstance(n_st, int) or not 1 <= n_st <= code.size(0):
      raise ValueError('stages must be an int in 1 .. {}, got {!r}'.format(code.size(0), stages))
    L = self._code_books.size(1)
    _rows_limit(code.size(1) * code.size(2), L)
    depth, groups = self._depth(depth, groups, code.size(1) * code.size(2))      # host refusals first, then the device's
    _on_gpu(code, 'code')
    _on_gpu(self._code_books, 'the code books')
    index = code[:n_st].reshape(n_st, -1)
    bad = (index < 0) | (index >= L)
    if depth is not None:                        # only inside the depth (the clamp is the device's); beyond it nothing is read
      bad = bad & (torch.arange(n_st, device=code.device).view(n_st, 1) < depth.clamp(1, self.n_stages).repeat_interleave(groups))
      index = index.clamp(-1, L)                 # so that the cast below cannot fold a far value into range
    if bool(bad.any()):                          # before the cast to int32 could fold a far value into range
      raise ValueError('ResidualS2HVQ.decode: an index outside [0, {})'.format(L))
    index = index.to(torch.int32).contiguous()
    y, _ = ops.vq_res_decode(index, self._code_books.detach().contiguous(), n_st, depth=depth, groups=groups)
    return y.view(code.size(1), code.size(2) * self._center_size)

  def distortion(self, x, code_len):
    """float64 [S] on the device: the mean squared error per vector, sum |x - y^(s)|^2 / (n * code_len), after every stage s --
    the measure S2HVQ.fit reports for one."""
    with torch.no_grad():
      xm = self._vectors(x, code_len).detach()
      _, _, sse, _ = ops.vq_res_fwd(xm, self._code_books.detach().contiguous(), want_sse=True)
    return sse / float(xm.size(0))

  def fit(self, x, code_len, n_iter=10, init='sample', seed=0, reseed=True):
    """Fit the books stage by stage: stage s is S2HVQ.fit's Lloyd loop (ops.vq_lloyd_accum / vq_lloyd_update, the
    same sampling rule for init='sample') on the residual r_s that the fitted stages before it leave, taken from ops.vq_res_fwd(...,
    n_stages=s - 1, want_residual=True).  x: one tensor [n, d].  Runs under no_grad and writes `_code_books` IN PLACE: same
    storage, requires_grad and .grad untouched.  Deterministic.  Returns a list of S dicts, S2HVQ.fit's report of every stage
    (its `distortion` measured on r_s), and in each `final`: the mean squared distance after that stage under the fitted books
    (what distortion(x, code_len) returns); statistics are read back once per stage."""
    if isinstance(n_iter, bool) or not isinstance(n_iter, int) or n_iter < 0:
      raise ValueError('n_iter must be an int >= 0, got {!r}'.format(n_iter))
    if init not in ('sample', 'current'):
      raise ValueError("init must be 'sample' or 'current', got {!r}".format(init))
    if not torch.is_tensor(x) or x.dim() != 2 or x.size(0) < 1:
      raise ValueError('x must be a tensor [n, d] with n >= 1, got {}'.format(tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
    self._vector_checks(x, code_len)
    S, L, D = self.n_stages, int(self._code_books.size(1)), self._center_size
    if init == 'sample' and x.size(0) * code_len < L:
      raise ValueError("init='sample' draws n_center = {} distinct vectors from x, which has {}".format(L, x.size(0) * code_len))
    reports = []
    with torch.no_grad():
      xm = self._vectors(x, code_len).detach()
      books = self._code_books.data
      if not books.is_contiguous() or xm.device != books.device:
        raise ValueError('ResidualS2HVQ.fit: the code books must be contiguous and on the device of x')
      M = xm.size(0)
      state = ops.vq_lloyd_state(L, D, books.device)
      for s in range(S):
        res = ops.vq_res_fwd(xm, books, n_stages=s, want_residual=True)[3]
        book = books[s]                                        # a view: the updates land in the parameter's storage
        if init == 'sample':
          pick = torch.randperm(M, generator=torch.Generator().manual_seed(int(seed) + s))[:L]
          book.copy_(res.index_select(0, pick.to(book.device)))
        distortion, updates = [], []
        for it in range(n_iter + 1):
          ops.vq_lloyd_accum(res, book, state, first=True)
          distortion.append(state['sse'].sum() / float(M))
          if it < n_iter:
            updates.append(ops.vq_lloyd_update(book, state, reseed=bool(reseed)))
        counts = state['counts'].clone()
        distortion = torch.stack(distortion).cpu().tolist()
        updates = torch.stack(updates).cpu().tolist() if updates else []
        reports.append(dict(distortion=[float(v) for v in distortion], dead=[int(r[0]) for r in updates],
                            reseeded=[int(r[1]) for r in updates], counts=counts))
      final = self.distortion(x, code_len).cpu().tolist()
    for s, rep in enumerate(reports):
      rep['final'] = float(final[s])
    return reports
