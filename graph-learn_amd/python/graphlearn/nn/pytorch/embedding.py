"""Trainable embedding tables that live in HBM and are updated in place on the rows a batch touched: the torch surface
of glx_rows_coalesce and glx_embedding_update (include/glx.h).

The role of the reference's EmbeddingColumn (graphlearn/python/nn/tf/data/feature_column.py:128-157) -- one per
categorical attribute (feature_handler.py:162) -- and of the target / context id embeddings of DeepWalk / node2vec
(examples/tf/node2vec/node2vec.py:49-50):

    target, context = SparseEmbedding(V, 128), SparseEmbedding(V, 128)
    opt = SparseAdam([target, context], lr=0.01)
    nodes, local = glx.unique([walks, negs])                           # the distinct ids of the batch
    zt, zc = target(nodes, distinct=True), context(nodes, distinct=True)
    loss = ...pair_dot(zt, l_src, zc, l_dst)...
    loss.backward()                                                    # no [V, 128] gradient anywhere
    opt.step()                                                         # touches nodes.numel() rows of each table

A table's weight is a buffer, not a Parameter: dense optimizers never see it, state_dict() carries it, and backward
produces no [num_rows, dim] tensor -- it only notes (ids, gradient of the looked-up rows) on the module.  step() sums
the noted gradients per distinct row (in ascending position, in a fixed order: the same bits on every run, no float
atomic) and applies SGD / Adagrad / Adam to those rows with one kernel.  No step reads anything back on the host.

Limits: float32 tables and states; dense row indices (id v is row v); one GPU; no graph capture; no weight decay;
Adam's step count is one number per table, as in torch.optim.SparseAdam.  With distinct=True the ids of that forward
must be distinct (glx.unique's output, CompactBatch.nodes): when it is the table's only forward of the step its gradient
goes to the update as it is -- a repeated id there would be a lost update.  (That path keeps a -0.0 gradient element as
it is where the coalesce, which adds every term to +0.0, makes it +0.0: with a -0.0 in the gradient the two paths can
differ in the sign of a zero.)
"""
import math

import torch

from graphlearn.nn.pytorch.segment import _glx, _no_double_backward

__all__ = ["SparseEmbedding", "SparseSGD", "SparseAdagrad", "SparseAdam"]

_INT32_MAX = 2 ** 31 - 1


class _Lookup(torch.autograd.Function):

  @staticmethod
  def forward(ctx, anchor, module, ids, distinct, seq):
    glx = _glx()
    w = module.weight
    out = glx.Features(w, view=True, device=w.device.index or 0).lookup(ids, 0.0)
    ctx.module, ctx.distinct, ctx.seq = module, distinct, seq
    ctx.save_for_backward(ids)
    return out

  @staticmethod
  def backward(ctx, grad):
    _no_double_backward("SparseEmbedding")
    (ids,) = ctx.saved_tensors
    grad = grad.to(torch.float32).contiguous()
    ctx.module._pending.append((ctx.seq, ids, grad, ctx.distinct))
    return None, None, None, None, None


class SparseEmbedding(torch.nn.Module):
  """A [num_rows, dim] float32 table on `device`, normal(0, init_std or dim ** -0.5) from a generator seeded with
  `seed`.  forward(ids) looks rows up; backward notes their gradient for a Sparse* optimizer of this module."""

  def __init__(self, num_rows, dim, device="cuda", init_std=None, seed=0):
    super().__init__()
    num_rows, dim = int(num_rows), int(dim)
    if num_rows < 0 or num_rows >= _INT32_MAX:
      raise ValueError("SparseEmbedding: num_rows must be in [0, 2^31 - 1), not {}".format(num_rows))
    if dim < 1 or dim > _INT32_MAX:
      raise ValueError("SparseEmbedding: dim must be in [1, 2^31 - 1], not {}".format(dim))
    self.num_rows, self.dim = num_rows, dim
    device = torch.device(device)
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    std = float(init_std) if init_std is not None else dim ** -0.5
    weight = torch.empty((num_rows, dim), dtype=torch.float32, device=device)
    weight.normal_(0.0, std, generator=gen)
    self.register_buffer("weight", weight)
    # what makes the output part of the autograd graph although the weight is not: an empty leaf that gets no gradient
    self._anchor = torch.zeros(0, requires_grad=True)
    self._pending = []  # (forward sequence number, ids [n], grad [n, dim], distinct), in the order backward ran
    self._seq = 0

  def forward(self, ids, distinct=False):
    """[*ids.shape, dim]: row ids[...] of the table; an id outside [0, num_rows) reads zeros and is never updated.
    distinct=True promises that the ids are distinct (see the module's docstring)."""
    who = "SparseEmbedding"
    w = self.weight
    if not isinstance(ids, torch.Tensor):
      raise ValueError("{}: ids must be a torch tensor".format(who))
    if ids.dtype != torch.int64:
      raise ValueError("{}: ids must be int64, not {}".format(who, ids.dtype))
    if not w.is_cuda:
      raise ValueError("{}: the table lives on {}; lookups run on a CUDA device only".format(who, w.device))
    if ids.device != w.device:
      raise ValueError("{}: ids live on {}, the table on {}".format(who, ids.device, w.device))
    shape = tuple(ids.shape)
    flat = ids.reshape(-1).contiguous()
    if flat.numel() * self.dim > _INT32_MAX:
      raise ValueError("{}: n * dim exceeds int32".format(who))
    self._seq += 1
    if torch.is_grad_enabled():
      out = _Lookup.apply(self._anchor, self, flat, bool(distinct), self._seq)
    else:
      glx = _glx()
      out = glx.Features(w, view=True, device=w.device.index or 0).lookup(flat, 0.0)
    return out.reshape(shape + (self.dim,))


class _SparseOptimizer(object):
  """What the three optimizers share: the pending gradients of each table, in forward order, coalesced and applied."""
  _ALGO = None
  _NUM_STATES = 0

  def __init__(self, embeddings, lr):
    if isinstance(embeddings, SparseEmbedding):
      embeddings = [embeddings]
    self.embeddings = list(embeddings)
    for e in self.embeddings:
      if not isinstance(e, SparseEmbedding):
        raise ValueError("{}: expected SparseEmbedding modules, got {}".format(type(self).__name__, type(e).__name__))
    if not lr >= 0.0:
      raise ValueError("{}: lr must be >= 0, not {}".format(type(self).__name__, lr))
    self.lr = float(lr)
    self.state = [{"step": 0, "state1": None, "state2": None} for _ in self.embeddings]

  # -- the pieces a subclass fills in
  def _new_state(self, weight, which):
    return torch.zeros_like(weight)

  def _scalars(self, t):
    raise NotImplementedError

  @staticmethod
  def _collect(emb):
    """(ids [n], grad [n, dim], direct) of a table's pending entries, concatenated in FORWARD order (backward runs in
    whatever order the graph dictates); direct: one entry, marked distinct -- its gradient is already one row per id."""
    entries = sorted(emb._pending, key=lambda e: e[0])
    if len(entries) == 1:
      _, ids, grad, distinct = entries[0]
      return ids, grad, bool(distinct)
    return torch.cat([e[1] for e in entries]), torch.cat([e[2] for e in entries]), False

  def step(self):
    glx = None
    for emb, st in zip(self.embeddings, self.state):
      if not emb._pending:
        continue
      glx = glx or _glx()
      ids, grad, direct = self._collect(emb)
      emb._pending = []
      if ids.numel() == 0:
        continue
      if not direct:
        ids, grad, _ = glx.rows_coalesce(ids, grad, emb.num_rows)  # the count stays on the device
      w = emb.weight
      for which in range(self._NUM_STATES):
        key = "state%d" % (which + 1)
        if st[key] is None:
          st[key] = self._new_state(w, which)
      st["step"] += 1
      alpha, eps, beta1, c1, beta2, c2 = self._scalars(st["step"])
      glx.embedding_update(self._ALGO, w, ids, grad, state1=st["state1"], state2=st["state2"], alpha=alpha, eps=eps,
                           beta1=beta1, c1=c1, beta2=beta2, c2=c2)

  def zero_grad(self):
    for emb in self.embeddings:
      emb._pending = []

  def state_dict(self):
    return {"lr": self.lr, "state": [dict(st) for st in self.state]}

  def load_state_dict(self, sd):
    if len(sd["state"]) != len(self.embeddings):
      raise ValueError("{}: the state dict has {} tables, the optimizer {}".format(
          type(self).__name__, len(sd["state"]), len(self.embeddings)))
    self.lr = float(sd["lr"])
    for emb, st, src in zip(self.embeddings, self.state, sd["state"]):
      st["step"] = int(src["step"])
      for key in ("state1", "state2"):
        t = src[key]
        st[key] = None if t is None else t.detach().to(device=emb.weight.device, dtype=torch.float32).clone()


class SparseSGD(_SparseOptimizer):
  """w -= lr * g on the touched rows (torch.optim.SGD without momentum or weight decay)."""
  _ALGO, _NUM_STATES = 0, 0

  def __init__(self, embeddings, lr):
    super().__init__(embeddings, lr)

  def _scalars(self, t):
    return self.lr, 0.0, 0.0, 0.0, 0.0, 0.0


class SparseAdagrad(_SparseOptimizer):
  """s += g * g; w -= lr * g / (sqrt(s) + eps) on the touched rows (torch.optim.Adagrad, lr_decay = weight_decay = 0)."""
  _ALGO, _NUM_STATES = 1, 1

  def __init__(self, embeddings, lr, eps=1e-10, initial_accumulator_value=0.0):
    super().__init__(embeddings, lr)
    self.eps, self.initial_accumulator_value = float(eps), float(initial_accumulator_value)

  def _new_state(self, weight, which):
    return torch.full_like(weight, self.initial_accumulator_value)

  def _scalars(self, t):
    return self.lr, self.eps, 0.0, 0.0, 0.0, 0.0


class SparseAdam(_SparseOptimizer):
  """torch.optim.SparseAdam on the coalesced gradient: the moments of the touched rows only, one step count per table;
  the bias corrections are folded into the step size in double (alpha = lr * sqrt(1 - beta2^t) / (1 - beta1^t))."""
  _ALGO, _NUM_STATES = 2, 2

  def __init__(self, embeddings, lr, betas=(0.9, 0.999), eps=1e-8):
    super().__init__(embeddings, lr)
    self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)

  def _scalars(self, t):
    b1, b2 = self.betas
    alpha = self.lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    return alpha, self.eps, b1, 1.0 - b1, b2, 1.0 - b2
