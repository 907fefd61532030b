"""Soft-to-hard vector quantizer (reference ctu/quantizers/s2h_vq.py) on the jpdse_vq_* kernels.

`S2HVQ` keeps the reference's interface -- parameter `_code_book`, properties `center_size` / `code_book` / `sigma`, methods
`encode` / `decode`, static `get_pmf` / `get_cross_entropy` -- so a reference training loop runs unchanged:

    code_raw = vq.encode(x, code_len)                       # soft assignment, differentiable in x and the code book
    pmf = S2HVQ.get_pmf(code_raw)
    loss = S2HVQ.get_cross_entropy(pmf, pmf) + ((vq.decode(code_raw) - x) ** 2).mean()
    loss.backward()

Every [.., n_center] matrix is float32, as in the reference, where the float32 code book promotes the scores; the hard one-hot
takes x's dtype.  There is no CPU path: tensors live on the GPU.  Limits (the kernels'): center_size <= 32, 2 <= n_center
<= 512, n * code_len * n_center < 2^31; anything beyond raises NotImplementedError.
"""
import torch
import torch.nn as nn

import jpdse_hip
from jpdse_hip import ops

__all__ = ['S2HVQ', 'S2HVQV2']

MAX_CENTER_SIZE = ops.VQ_MAX_D
MAX_N_CENTER = ops.VQ_MAX_L


def _on_gpu(t, what):
  if not t.is_cuda:
    raise jpdse_hip.JpdseError('S2HVQ: %s is on %s: the JPD-SE HIP path has no CPU fallback' % (what, t.device))


def _rows_limit(rows, n_center):
  if rows * n_center >= 2 ** 31:
    raise NotImplementedError('S2HVQ: n * code_len * n_center = %d, the kernels index below 2^31' % (rows * n_center))


def _ec_lambda(lam):
  """The rate multiplier of the entropy-constrained calls as a float: ValueError unless it is a finite number >= 0."""
  try:
    value = float(lam)
  except (TypeError, ValueError):
    raise ValueError('lam must be a finite number >= 0, got {!r}'.format(lam))
  if not (0.0 <= value < float('inf')):
    raise ValueError('lam must be a finite number >= 0, got {!r}'.format(lam))
  return value


def _ec_iterations(n_iter):
  if isinstance(n_iter, bool) or not isinstance(n_iter, int) or n_iter < 0:
    raise ValueError('n_iter must be an int >= 0, got {!r}'.format(n_iter))
  return n_iter


class _SoftAssign(torch.autograd.Function):
  """p = softmax_k(-sigma |x_m - c_k|^2) (ops.vq_soft_fwd); backward from the stored p (ops.vq_soft_bwd)."""

  @staticmethod
  def forward(ctx, x, code_book, sigma):
    x, code_book = x.contiguous(), code_book.contiguous()
    p = ops.vq_soft_fwd(x, code_book, sigma)
    ctx.save_for_backward(x, code_book, p)
    ctx.sigma = sigma
    return p

  @staticmethod
  def backward(ctx, dp):
    x, code_book, p = ctx.saved_tensors
    dx, dc = ops.vq_soft_bwd(dp.contiguous(), p, x, code_book, ctx.sigma, want_dx=ctx.needs_input_grad[0],
                             want_dc=ctx.needs_input_grad[1])
    return dx, dc, None


class _Gather(torch.autograd.Function):
  """y[m] = code_book[index[m]] (ops.vq_decode); the code book's gradient is the transposed gather (ops.vq_decode_bwd)."""

  @staticmethod
  def forward(ctx, code_book, index, status):
    code_book = code_book.contiguous()
    y, _ = ops.vq_decode(index, code_book, torch.float32, status)
    ctx.save_for_backward(index)
    ctx.n_center = code_book.shape[0]
    return y

  @staticmethod
  def backward(ctx, dy):
    index, = ctx.saved_tensors
    dc, _ = ops.vq_decode_bwd(index, dy.contiguous(), ctx.n_center)
    return dc, None, None


class _Pmf(torch.autograd.Function):
  """pmf[k] = mean over the rows of scores[.., k] (ops.vq_pmf / ops.vq_pmf_bwd)."""

  @staticmethod
  def forward(ctx, scores):
    s = scores.contiguous().view(-1, scores.shape[-1])
    ctx.shape = tuple(scores.shape)
    return ops.vq_pmf(s)

  @staticmethod
  def backward(ctx, dpmf):
    rows = 1
    for v in ctx.shape[:-1]:
      rows *= v
    return ops.vq_pmf_bwd(dpmf.contiguous(), rows).view(ctx.shape)


class _Quantize(torch.autograd.Function):
  """(y, index, pmf) of ops.vq_quantize_fwd; backward: ops.vq_quantize_bwd, the gradient of the soft form whatever the forward
  was (straight-through), p recomputed from the saved x.  A gradient arriving on pmf becomes dpmf."""

  @staticmethod
  def forward(ctx, x, code_book, sigma, hard_forward, want_pmf):
    x, code_book = x.contiguous(), code_book.contiguous()
    y, index, pmf = ops.vq_quantize_fwd(x, code_book, sigma, hard_forward, want_pmf)
    ctx.save_for_backward(x, code_book)
    ctx.sigma, ctx.want_pmf = sigma, want_pmf
    ctx.mark_non_differentiable(index)
    if not want_pmf:
      pmf = x.new_zeros(0, dtype=torch.float32)           # a placeholder output: autograd wants tensors
      ctx.mark_non_differentiable(pmf)
    return y, index, pmf

  @staticmethod
  def backward(ctx, dy, _dindex, dpmf):
    x, code_book = ctx.saved_tensors
    dpmf = dpmf.contiguous() if (ctx.want_pmf and dpmf is not None) else None
    dx, dc = ops.vq_quantize_bwd(dy.contiguous(), x, code_book, ctx.sigma, dpmf, want_dx=ctx.needs_input_grad[0],
                                 want_dc=ctx.needs_input_grad[1])
    return dx, dc, None, None, None


class _Rate(torch.autograd.Function):
  """rate fp32 [1] of ops.vq_rate_fwd; backward: ops.vq_quantize_bwd(groups, dhist) with dy = 0, dhist scaled
  by the incoming gradient."""

  @staticmethod
  def forward(ctx, x, code_book, sigma, groups, denom, hard):
    x, code_book = x.contiguous(), code_book.contiguous()
    rate, _, dhist = ops.vq_rate_fwd(x, code_book, sigma, groups, denom, 1.0, hard=hard)
    ctx.save_for_backward(x, code_book, dhist)
    ctx.sigma, ctx.groups = sigma, groups
    return rate

  @staticmethod
  def backward(ctx, drate):
    x, code_book, dhist = ctx.saved_tensors
    dx, dc = ops.vq_quantize_bwd(torch.zeros_like(x), x, code_book, ctx.sigma, want_dx=ctx.needs_input_grad[0],
                                 want_dc=ctx.needs_input_grad[1], groups=ctx.groups,
                                 dhist=(dhist * drate.to(torch.float32).reshape(())).contiguous())
    return dx, dc, None, None, None, None


class S2HVQ(nn.Module):
  """code_book: tensor [n_center, center_size], learnable (parameter `_code_book`); sigma > 0: the hardness of the soft
  assignment used in training."""

  def __init__(self, code_book, sigma=10., **kwargs):
    super(S2HVQ, self).__init__()
    assert sigma > 0, "sigma must be greater than 0, got {}".format(sigma)
    if code_book.dim() != 2:
      raise ValueError('code_book must have shape (n_center, center_size), got {}'.format(tuple(code_book.shape)))
    n_center, center_size = int(code_book.size(0)), int(code_book.size(1))
    if not 1 <= center_size <= MAX_CENTER_SIZE:
      raise NotImplementedError('S2HVQ: center_size %d, the kernels take 1 .. %d' % (center_size, MAX_CENTER_SIZE))
    if not 2 <= n_center <= MAX_N_CENTER:
      raise NotImplementedError('S2HVQ: n_center %d, the kernels take 2 .. %d' % (n_center, MAX_N_CENTER))
    if code_book.dtype != torch.float32:
      raise NotImplementedError('S2HVQ: a %s code book, the kernels keep it in float32' % (code_book.dtype,))
    self._center_size = center_size
    self._code_book = nn.Parameter(code_book)
    self._sigma = sigma

  @property
  def center_size(self):
    return self._center_size

  @property
  def code_book(self):
    return self._code_book

  @property
  def sigma(self):
    return self._sigma

  @sigma.setter
  def sigma(self, new_sigma):
    assert new_sigma > 0, "sigma must be greater than 0, got {}".format(new_sigma)
    self._sigma = new_sigma

  def _vectors(self, x, code_len):
    """[n, d] -> the contiguous [n * code_len, center_size] matrix of vectors, after every check that needs no device."""
    self._vector_checks(x, code_len)
    _on_gpu(x, 'x')
    _on_gpu(self.code_book, 'the code book')
    return x.contiguous().view(x.size(0) * code_len, self._center_size)

  def _vector_checks(self, x, code_len):
    """The checks of _vectors that need no device."""
    if x.size(1) < code_len:
      raise ValueError("x.size(1) must be greater than or equal to code_len, got "
                       "{} and {}, respectively".format(x.size(1), code_len))
    if x.size(1) % code_len != 0:
      raise ValueError("code_len must divide x.size(1), got {} and {}, respectively".format(code_len, x.size(1)))
    if x.size(1) // code_len != self.code_book.size(1):
      raise ValueError("Illegal code_len. x.size(1) // code_len must equal "
                       "code_book.size(0), got {}, {}, and {}, respectively.".format(x.size(1), code_len, self.code_book.size(1)))
    if x.dtype not in (torch.float32, torch.bfloat16):
      raise NotImplementedError('S2HVQ: x is %s, the kernels take float32 and bfloat16' % (x.dtype,))
    _rows_limit(x.size(0) * code_len, self.code_book.size(0))

  def encode(self, x, code_len, train=True, raw=True):
    """x [n, d], code_len dividing d with d // code_len == center_size.  raw: the scores over the centres, [n, code_len,
    n_center] -- the soft assignment (train, float32, differentiable) or the one-hot of the nearest centre (x's dtype);
    not raw: the index of the highest score, int64 [n, code_len]."""
    xm = self._vectors(x, code_len)
    n, L = x.size(0), self.code_book.size(0)
    if train:
      p = _SoftAssign.apply(xm, self.code_book, float(self._sigma))
      if raw:
        return p.view(n, code_len, L)
      return ops.vq_argmax(p.detach()).to(torch.int64).view(n, code_len)
    index, onehot = ops.vq_hard_fwd(xm.detach(), self.code_book.detach().contiguous(), want_onehot=raw)
    if raw:
      return onehot.view(n, code_len, L).to(x.dtype)
    return index.to(torch.int64).view(n, code_len)

  def quantize(self, x, code_len, hard_forward=True, want_pmf=False):
    """The quantizer as a bottleneck: x [n, d] -> (y [n, d] in x's dtype, code int64 [n, code_len], pmf float32
    [n_center] or None) in one kernel, the [n * code_len, n_center] assignment never stored.  y is the nearest centre of every
    vector (hard_forward) or the soft assignment's mix of the centres; pmf the column means of the soft assignment.
    Training mode: differentiable in x and the code book, and the gradient is the soft form's whatever hard_forward is (the
    straight-through rule); a gradient on pmf is taken too.  Eval mode: always the hard forward, nothing saved.  Argument checks
    are encode's."""
    xm = self._vectors(x, code_len)
    n = x.size(0)
    if self.training and torch.is_grad_enabled():
      y, index, pmf = _Quantize.apply(xm, self.code_book, float(self._sigma), bool(hard_forward), bool(want_pmf))
    else:
      y, index, pmf = ops.vq_quantize_fwd(xm.detach(), self.code_book.detach().contiguous(), float(self._sigma),
                                          bool(hard_forward) or not self.training, bool(want_pmf))
    return y.view(n, code_len * self._center_size), index.to(torch.int64).view(n, code_len), (pmf if want_pmf else None)

  def rate(self, x, code_len, groups=1, denom=None, hard=False):
    """The rate term on per-group histograms: x [n, d] as in quantize; vector m of the [n * code_len,
    center_size] matrix belongs to group m % groups (groups must divide n * code_len).  Returns the 0-dim float32
    -sum_g sum_k hist[g][k] log2(hist[g][k] / (M / groups)) / denom with hist the per-group sums of the soft assignment (hard:
    of the one-hot of the nearest centre); denom defaults to M = n * code_len: bits per index.  Differentiable in x and the code
    book when gradients are enabled (the gradient is the soft form's, also with hard); [M, n_center] is never stored.  With
    groups = 1, rate * denom / M is get_cross_entropy(pmf, pmf) of pmf = get_pmf(encode(x, code_len))."""
    xm = self._vectors(x, code_len)
    M, groups = xm.size(0), int(groups)
    if groups < 1 or M % groups != 0:
      raise ValueError('groups must divide n * code_len, got {} and {}'.format(groups, M))
    if groups * self.code_book.size(0) > 65536:
      raise NotImplementedError('S2HVQ.rate: groups * n_center = %d, the kernels take at most 65536' % (groups * self.code_book.size(0)))
    denom = float(M if denom is None else denom)
    if not (denom > 0 and denom != float('inf')):
      raise ValueError('denom must be a finite number > 0, got {}'.format(denom))
    if torch.is_grad_enabled() and (xm.requires_grad or self.code_book.requires_grad):
      return _Rate.apply(xm, self.code_book, float(self._sigma), groups, denom, bool(hard)).reshape(())
    value, _, _ = ops.vq_rate_fwd(xm.detach(), self.code_book.detach().contiguous(), float(self._sigma), groups, denom,
                                  hard=bool(hard), want_grad=False)
    return value.reshape(())

  def encode_ec(self, x, code_len, lam, groups=1, n_iter=2):
    """Entropy-constrained encoding (Chou, Lookabaugh, Gray): x [n, d] as in encode; vector m of the [n *
    code_len, center_size] matrix belongs to group m % groups (groups must divide n * code_len).  Every vector takes the centre
    that minimises |x - c_k|^2 + lam * len[g][k], len[g][k] = log2(n_g / hist[g][k]) the code length of centre k under the
    histogram of group g's own code.  Iteration 0 assigns with no bias (the plain code, encode(train=False, raw=False));
    iteration t = 1 .. n_iter takes the lengths from the histogram of iteration t - 1 (ops.vq_ec_lengths) and assigns again
    (ops.vq_ec_assign).  The decoder is untouched: the result is an ordinary code.
    Returns (code int64 [n, code_len], report): report['distortion'][t] the summed squared distance of iteration t,
    report['bits'][t] the ideal length of its code under its own per-group histograms, report['cost'][t] = distortion[t] +
    lam * bits[t]; n_iter + 1 Python floats each, read back once, at the end.  cost is non-increasing up to the fp32 rounding
    of the scores.  lam == 0 or n_iter == 0: the plain code, index for index.
    A centre that the plain code of a group never uses has length +inf there and stays unused in that group in every later
    iteration, so the set of centres in use can only shrink.  Runs under no_grad: nothing is differentiable."""
    lam = _ec_lambda(lam)
    n_iter = _ec_iterations(n_iter)
    self._vector_checks(x, code_len)
    M, groups, L = x.size(0) * code_len, int(groups), self.code_book.size(0)
    if groups < 1 or M % groups != 0:
      raise ValueError('groups must divide n * code_len, got {} and {}'.format(groups, M))
    if groups * L > 65536:
      raise NotImplementedError('S2HVQ.encode_ec: groups * n_center = %d, the kernels take at most 65536' % (groups * L))
    with torch.no_grad():
      xm = self._vectors(x, code_len).detach()
      book = self.code_book.detach().contiguous()
      index, hist, sse = ops.vq_ec_assign(xm, book, None, groups)
      dist, bits = [sse.sum()], []
      for _ in range(n_iter):
        bias, b = ops.vq_ec_lengths(hist, lam)
        bits.append(b.sum())
        index, hist, sse = ops.vq_ec_assign(xm, book, bias, groups)
        dist.append(sse.sum())
      bits.append(ops.vq_ec_lengths(hist, lam)[1].sum())
      back = torch.stack(dist + bits).cpu().tolist()
    dist, bits = [float(v) for v in back[:n_iter + 1]], [float(v) for v in back[n_iter + 1:]]
    report = dict(distortion=dist, bits=bits, cost=[d + lam * b for d, b in zip(dist, bits)])
    return index.to(torch.int64).view(x.size(0), code_len), report

  def fit(self, x, code_len, n_iter=10, init='sample', seed=0, reseed=True):
    """Fit the code book to data by Lloyd (k-means) iterations on the device.  x: a tensor [n, d] or a list of
    such tensors (batches), each checked as encode checks it; every iteration accumulates all of them under the current book
    (ops.vq_lloyd_accum: one fused pass per tensor) and then moves every centre to the mean of its members
    (ops.vq_lloyd_update).  reseed: a centre without members takes the farthest member of the centre with the largest summed
    distance (one donor per dead centre, donors need two members); without it such a centre stays where it is.
    init: 'current' starts from the book as it is; 'sample' first sets it to n_center distinct vectors of the first tensor, rows
    torch.randperm(M, generator=<CPU generator seeded with `seed`>)[:n_center] of its [M, center_size] matrix (ValueError when
    M < n_center).  Deterministic: the same arguments give the same bits, on every device and rank.
    Runs under no_grad and writes `_code_book` IN PLACE: same storage (the fused Adam and the gradient buckets keep their
    pointer), requires_grad and .grad untouched.  After the last update one more pass measures the fitted book.  Returns a dict:
    `distortion`, n_iter + 1 Python floats, the mean squared distance of a vector to its nearest centre -- entry t under the
    book before update t, the last under the fitted book; `dead` and `reseeded`, n_iter ints each: the centres without members
    at update t and how many of them were reseeded; `counts`, int64 [n_center] on the device: the members under the fitted
    book.  The statistics are read back once, at the end."""
    if isinstance(n_iter, bool) or not isinstance(n_iter, int) or n_iter < 0:
      raise ValueError('n_iter must be an int >= 0, got {!r}'.format(n_iter))
    if init not in ('sample', 'current'):
      raise ValueError("init must be 'sample' or 'current', got {!r}".format(init))
    xs = list(x) if isinstance(x, (list, tuple)) else [x]
    if len(xs) == 0:
      raise ValueError('x must be a tensor [n, d] or a non-empty list of such tensors')
    for t in xs:
      if not torch.is_tensor(t) or t.dim() != 2 or t.size(0) < 1:
        raise ValueError('x must be a tensor [n, d] with n >= 1 or a list of such tensors, got {}'.format(
            tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
      self._vector_checks(t, code_len)
    L, D = int(self.code_book.size(0)), self._center_size
    if init == 'sample' and xs[0].size(0) * code_len < L:
      raise ValueError("init='sample' draws n_center = {} distinct vectors from the first tensor, which has {}".format(
          L, xs[0].size(0) * code_len))
    with torch.no_grad():
      mats = [self._vectors(t, code_len).detach() for t in xs]
      book = self._code_book.data
      if not book.is_contiguous() or any(m.device != book.device for m in mats):
        raise ValueError('S2HVQ.fit: the code book must be contiguous and on the device of x')
      if init == 'sample':
        pick = torch.randperm(mats[0].size(0), generator=torch.Generator().manual_seed(int(seed)))[:L]
        book.copy_(mats[0].index_select(0, pick.to(book.device)).to(torch.float32))
      total = float(sum(m.size(0) for m in mats))
      state = ops.vq_lloyd_state(L, D, book.device)
      distortion, reports = [], []
      for it in range(n_iter + 1):
        for i, m in enumerate(mats):
          ops.vq_lloyd_accum(m, book, state, first=(i == 0))
        distortion.append(state['sse'].sum() / total)
        if it < n_iter:
          reports.append(ops.vq_lloyd_update(book, state, reseed=bool(reseed)))
      counts = state['counts'].clone()
      distortion = torch.stack(distortion).cpu().tolist()
      reports = torch.stack(reports).cpu().tolist() if reports else []
    return dict(distortion=[float(v) for v in distortion], dead=[int(r[0]) for r in reports],
                reseeded=[int(r[1]) for r in reports], counts=counts)

  def decode(self, code_raw):
    """code_raw [n, code_len, n_center] (e.g. encode(..., raw=True)) -> [n, code_len * center_size]: the centre with the highest
    score of every position (always the hard decoding, as the reference).  Differentiable in the code book."""
    L = self.code_book.size(0)
    if code_raw.dim() != 3 or code_raw.size(2) != L:
      raise ValueError('code_raw must have shape (n, code_len, {}), got {}'.format(L, tuple(code_raw.shape)))
    _rows_limit(code_raw.size(0) * code_raw.size(1), L)
    _on_gpu(code_raw, 'code_raw')
    _on_gpu(self.code_book, 'the code book')
    s = code_raw.detach().contiguous().view(-1, L)
    index = ops.vq_argmax(s if s.dtype == torch.float32 else s.float())
    status = torch.zeros(1, dtype=torch.int32, device=index.device)
    y = _Gather.apply(self.code_book, index, status)
    if not self.training and int(status.item()) != 0:      # eval paths synchronise anyway
      raise ValueError('S2HVQ.decode: an index outside [0, {})'.format(L))
    return y.view(code_raw.size(0), code_raw.size(1) * self._center_size)

  @staticmethod
  def get_pmf(scores):
    """scores [n, code_len, n_center] -> the histogram over the centres, [n_center]: the batch estimate of the code's pmf."""
    if not 2 <= scores.size(-1) <= MAX_N_CENTER:
      raise NotImplementedError('S2HVQ.get_pmf: n_center %d, the kernels take 2 .. %d' % (scores.size(-1), MAX_N_CENTER))
    _rows_limit(scores.numel() // scores.size(-1), scores.size(-1))
    _on_gpu(scores, 'scores')
    return _Pmf.apply(scores if scores.dtype == torch.float32 else scores.float())

  @staticmethod
  def get_cross_entropy(pmf1, pmf2):
    """H(pmf1, pmf2) = -sum_k pmf1[k] log2 pmf2[k] over the centres with pmf2[k] > 0.  n_center numbers: plain torch."""
    assert torch.all(pmf1 >= 0), "pmf1 have < 0 or nan element(s)"
    assert torch.all(pmf2 >= 0), "pmf2 have < 0 or nan element(s)"
    one = torch.tensor(1., device=pmf1.device)
    assert torch.allclose(pmf1.sum(), one), "pmf1 is not normalized"
    assert torch.allclose(pmf2.sum(), one.to(pmf2.device)), "pmf2 is not normalized"
    keep = pmf2 > 0
    return (-pmf1[keep] * torch.log2(pmf2[keep])).sum()


class S2HVQV2(S2HVQ):
  """The reference's variant with an MLP score: it needs Linear layers, which this project does not have."""

  def __init__(self, **kwargs):
    raise NotImplementedError('S2HVQV2 scores with an MLP (three Linear layers): not available on the HIP path')
