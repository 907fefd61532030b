"""Float64 torch-CPU restatement of the code-book fit (include/jpdse.h, "code-book fit"), written from the
definitions: the state of one accumulate pass for a given assignment, the update rule with its donor ranking, and a whole Lloyd
run.  x: [M, D] float64, c: [L, D] float64.  A state is a dict counts int64 [L], sums float64 [L, D], sse float64 [L], far_dist
float64 [L] (-1 without members), far_vec float64 [L, D] (zeros without members), far_m int64 [L] (-1 without members)."""
import torch

import vq_util


def assign(x, c):
  """(index int64 [M], distance float64 [M]): the nearest centre, the lowest index on a tie, and its distance."""
  d = vq_util.scores(x, c)
  index = vq_util.hard_index(x, c)
  return index, d[torch.arange(x.shape[0]), index]


def accumulate(x, index, dist, L, state=None, m_offset=0):
  """The state after one pass over x with the given assignment; `state`: the running state to add to (a later pass replaces a
  centre's farthest member only on a strictly greater distance)."""
  M, D = x.shape
  if state is None:
    state = dict(counts=torch.zeros(L, dtype=torch.int64), sums=torch.zeros(L, D, dtype=torch.float64),
                 sse=torch.zeros(L, dtype=torch.float64), far_dist=torch.full((L,), -1.0, dtype=torch.float64),
                 far_vec=torch.zeros(L, D, dtype=torch.float64), far_m=torch.full((L,), -1, dtype=torch.int64))
  else:
    state = {k: v.clone() for k, v in state.items()}
  for k in range(L):
    members = torch.nonzero(index == k).view(-1)
    if members.numel() == 0:
      continue
    state['counts'][k] += members.numel()
    state['sums'][k] += x[members].sum(dim=0)
    state['sse'][k] += dist[members].sum()
    dk = dist[members]
    first = members[torch.nonzero(dk == dk.max()).view(-1)[0]]      # the lowest m of the largest distance
    if float(dk.max()) > float(state['far_dist'][k]):
      state['far_dist'][k] = dk.max()
      state['far_vec'][k] = x[first]
      state['far_m'][k] = int(first) + m_offset
  return state


def donors(state):
  """The donor centres in rank order: n >= 2 and far_dist > 0, by sse descending, the lower k first on equal sse."""
  L = state['counts'].numel()
  ks = [k for k in range(L) if int(state['counts'][k]) >= 2 and float(state['far_dist'][k]) > 0]
  return sorted(ks, key=lambda k: (-float(state['sse'][k]), k))


def update(c, state, reseed=True):
  """(next code book float64 [L, D], (dead, reseeded), {dead k: donor k})."""
  out = c.clone()
  L = c.shape[0]
  dead = [k for k in range(L) if int(state['counts'][k]) == 0]
  rank = donors(state)
  took = {}
  for k in range(L):
    n = int(state['counts'][k])
    if n > 0:
      out[k] = state['sums'][k] / float(n)
  if reseed:
    for i, k in enumerate(dead):
      if i < len(rank):
        out[k] = state['far_vec'][rank[i]]
        took[k] = rank[i]
  return out, (len(dead), len(took)), took


def lloyd(xs, c, n_iter, reseed=True, round32=True):
  """A whole run over the list of matrices xs from the book c: (fitted book, distortion [n_iter + 1], dead [n_iter], reseeded
  [n_iter], counts of the fitted book).  round32: the book is rounded to float32 after every update, as the device stores it."""
  c = c.clone()
  total = sum(x.shape[0] for x in xs)
  distortion, dead, reseeded = [], [], []
  L = c.shape[0]
  for it in range(n_iter + 1):
    state = None
    for x in xs:
      index, dist = assign(x, c)
      state = accumulate(x, index, dist, L, state)
    distortion.append(float(state['sse'].sum()) / total)
    if it < n_iter:
      c, (nd, nr), _ = update(c, state, reseed)
      if round32:
        c = c.float().double()
      dead.append(nd)
      reseeded.append(nr)
  return c, distortion, dead, reseeded, state['counts']
