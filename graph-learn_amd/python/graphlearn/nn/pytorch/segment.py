"""Differentiable segment reductions and row gathers over a device-resident matrix: the torch surface of
glx_aggregate / glx_aggregate_arg / glx_aggregate_backward (include/glx.h).

The role of tf.math.unsorted_segment_sum / unsorted_segment_mean under the reference's layers
(graphlearn/python/nn/tf/layers/sage_conv.py:69-73, gcn_conv.py:73), for matrices that are computed on the way --
`z = relu(enc(batch.x_nodes))`, one row per distinct node of a CompactBatch -- and therefore need a gradient:

    h1 = segment_aggregate(z, batch.local[2], num_segments=batch.local[1].numel(), op="mean")
    s1 = gather_rows(z, batch.local[1].reshape(-1))

Neither materialises the [n, D] gather `z[index]`, and neither backward uses a float atomic: every element of x.grad
adds its terms in ascending request position, so two runs of one batch give the same bits (torch's `z[index]` goes
backward through index_add_ with float atomics, in whatever order they land).
"""
import torch

__all__ = ["segment_aggregate", "gather_rows"]

_OPS = {"sum": 0, "mean": 1, "max": 2, "min": 3, "prod": 4}


def _glx():
  import graphlearn.graph  # noqa: F401  (puts the engine's ctypes harness on sys.path)
  import glx
  return glx


def _check_inputs(x, index, who):
  if not isinstance(x, torch.Tensor) or not isinstance(index, torch.Tensor):
    raise ValueError("{}: x and index must be torch tensors".format(who))
  if x.dtype != torch.float32:
    raise ValueError("{}: x must be float32, not {} (half tables have no backward)".format(who, x.dtype))
  if not x.is_cuda or x.dim() != 2 or not x.is_contiguous():
    raise ValueError("{}: x must be a contiguous [N, D] CUDA tensor".format(who))
  if x.shape[1] < 1:
    raise ValueError("{}: x must have at least one column".format(who))
  if index.dtype != torch.int64:
    raise ValueError("{}: index must be int64, not {}".format(who, index.dtype))
  if index.device != x.device:
    raise ValueError("{}: index lives on {}, x on {}".format(who, index.device, x.device))
  if index.requires_grad:
    raise ValueError("{}: index carries no gradient".format(who))


def _no_double_backward(who):
  # the engine runs a backward with grad mode on only when it was asked to build a graph of it (create_graph=True)
  if torch.is_grad_enabled():
    raise ValueError("{}: double backward is not supported".format(who))


class _SegmentAggregate(torch.autograd.Function):

  @staticmethod
  def forward(ctx, x, index, segment_ids, num_segments, op, default_attr):
    glx = _glx()
    feats = glx.Features(x.detach(), view=True, device=x.device.index or 0)
    arg = None
    if op in (glx.MAX, glx.MIN):
      emb, cnt, arg = feats.aggregate_arg(op, index, segment_ids, num_segments, default_attr)
    else:
      emb, cnt = feats.aggregate(op, index, segment_ids, num_segments, default_attr)
    ctx.op, ctx.num_rows = op, int(x.shape[0])
    # the implied layout needs no counts: its segments are arithmetic
    ctx.implied = segment_ids is None
    ctx.has_arg = arg is not None
    ctx.save_for_backward(*([index, cnt] + ([arg] if arg is not None else [])))
    return emb

  @staticmethod
  def backward(ctx, grad):
    _no_double_backward("segment_aggregate")
    saved = ctx.saved_tensors
    index, cnt = saved[0], saved[1]
    arg = saved[2] if ctx.has_arg else None
    grad = grad.to(torch.float32).contiguous()
    gx = _glx().aggregate_backward(ctx.op, index, None if ctx.implied else cnt, grad, ctx.num_rows, arg=arg)
    return gx, None, None, None, None, None


def segment_aggregate(x, index, num_segments, op="mean", segment_ids=None, default_attr=0.0):
  """[num_segments, D]: segment s reduces the rows x[index[p]] of its positions p with `op` ("sum", "mean", "max",
  "min"; "prod" only for an x that needs no gradient), exactly as glx.Features(x, view=True).aggregate does -- the
  engine's tuned reduce, left to right, bit-identical on every run.

  x            [N, D] contiguous float32 CUDA tensor; may require grad
  index        int64 CUDA tensor of any shape (flattened): rows of x; a value outside [0, N) reads a row of
               `default_attr` and receives no gradient
  segment_ids  None: num_segments equal segments of index.numel() / num_segments consecutive positions (a dense
               sampler response); or an int32 tensor like index, consumed with the reference's cursor rule
               (non-decreasing ids in [0, num_segments); everything behind the first violation is ignored)
  Empty segments are `default_attr` and pass no gradient on.  Anything else raises ValueError.
  """
  _check_inputs(x, index, "segment_aggregate")
  if op not in _OPS:
    raise ValueError("segment_aggregate: op must be one of {}, not {!r}".format(sorted(_OPS), op))
  num_segments = int(num_segments)
  if num_segments < 0:
    raise ValueError("segment_aggregate: num_segments must be >= 0")
  index = index.reshape(-1).contiguous()
  if segment_ids is not None:
    if not isinstance(segment_ids, torch.Tensor) or segment_ids.dtype != torch.int32 or segment_ids.device != x.device:
      raise ValueError("segment_aggregate: segment_ids must be an int32 tensor on x's device")
    segment_ids = segment_ids.reshape(-1).contiguous()
    if segment_ids.numel() != index.numel():
      raise ValueError("segment_aggregate: segment_ids must have one entry per index")
  elif num_segments == 0 or index.numel() % num_segments != 0:
    raise ValueError("segment_aggregate: without segment_ids, index.numel() must be a multiple of num_segments")
  if num_segments * int(x.shape[1]) > 2 ** 31 - 1:
    raise ValueError("segment_aggregate: num_segments * D exceeds int32")
  if op == "prod":
    if x.requires_grad and torch.is_grad_enabled():
      raise ValueError("segment_aggregate: op='prod' has no backward (its gradient divides by the element)")
    glx = _glx()
    feats = glx.Features(x.detach(), view=True, device=x.device.index or 0)
    return feats.aggregate(glx.PROD, index, segment_ids, num_segments, float(default_attr))[0]
  return _SegmentAggregate.apply(x, index, segment_ids, num_segments, _OPS[op], float(default_attr))


class _GatherRows(torch.autograd.Function):

  @staticmethod
  def forward(ctx, x, index, default_attr):
    glx = _glx()
    out = glx.Features(x.detach(), view=True, device=x.device.index or 0).lookup(index, default_attr)
    ctx.num_rows = int(x.shape[0])
    ctx.save_for_backward(index)
    return out

  @staticmethod
  def backward(ctx, grad):
    _no_double_backward("gather_rows")
    (index,) = ctx.saved_tensors
    glx = _glx()
    grad = grad.to(torch.float32).contiguous()
    # one position per segment: the Sum backward of the implied layout
    return glx.aggregate_backward(glx.SUM, index, None, grad, ctx.num_rows), None, None


def gather_rows(x, index, default_attr=0.0):
  """x[index] as [*index.shape, D] -- the engine's lookup going forward, the deterministic Sum backward (one position
  per segment) going back: the replacement for `z[local[h]]` whose backward is index_add_ with float atomics.  A value
  of index outside [0, N) reads a row of `default_attr` and receives no gradient."""
  _check_inputs(x, index, "gather_rows")
  shape = tuple(index.shape)
  out = _GatherRows.apply(x, index.reshape(-1).contiguous(), float(default_attr))
  return out.reshape(shape + (int(x.shape[1]),))
