"""Differentiable segment reductions, row gathers and pair scores over a device-resident matrix: the torch surface of
glx_aggregate / glx_aggregate_arg / glx_aggregate_backward, of glx_aggregate_weighted and its two gradients, of
glx_segment_softmax and its gradient, of glx_gat_attention and its gradients, of glx_dot_attention and its gradients
and of glx_pair_dot and its gradient (include/glx.h).

The role of tf.math.unsorted_segment_sum / unsorted_segment_mean under the reference's layers
(graphlearn/python/nn/tf/layers/sage_conv.py:69-73, gcn_conv.py:73), for matrices that are computed on the way --
`z = relu(enc(batch.x_nodes))`, one row per distinct node of a CompactBatch -- and therefore need a gradient:

    h1 = segment_aggregate(z, batch.local[2], num_segments=batch.local[1].numel(), op="mean")
    s1 = gather_rows(z, batch.local[1].reshape(-1))

Neither materialises the [n, D] gather `z[index]`, and neither backward uses a float atomic: every element of x.grad
adds its terms in ascending request position, so two runs of one batch give the same bits (torch's `z[index]` goes
backward through index_add_ with float atomics, in whatever order they land).

weighted_segment_aggregate is the reduce under a GCN layer (every neighbour row scaled by an edge coefficient,
gcn_conv.py:52-73) and a GAT layer (a learned coefficient per neighbour and head, gat_conv.py:96-110):

    alpha = torch.softmax(e.view(S, k, H), dim=1)                      # dense sampler response: plain torch
    h = weighted_segment_aggregate(z, batch.local[2], alpha.view(S * k, H), num_segments=S, op="sum")

with a gradient for z and for alpha, neither through a float atomic.  The ragged form -- a FullSampler hop, or any
request with counts (unsorted_segment_softmax under the reference's gat_conv.py:101-112) -- is

    alpha = segment_softmax(e, S, counts=deg)                          # e [n, H]: one row of logits per position
    h = weighted_segment_aggregate(z, nbr_local, alpha, S, counts=deg)

where segment_softmax normalises each head over each segment's own positions, again without an atomic in either
direction.

gat_attention is the whole attention step of a GAT layer in one launch per direction (gat_conv.py:96-104): the logit
leaky_relu(s[segment] + t[index]), its softmax over each segment and dropout on the coefficients,

    alpha = gat_attention(src_e[seed_local], dst_e, nbr_local, S, counts=deg, dropout=0.4, seed=seed, call=step)

with a dropout mask that is a function of (seed, call, position, head) alone: two runs give the same bits.

dot_attention is the whole of a transformer-style layer's attention (TransformerConv in the reference's
examples/pytorch/tgn/train_and_eval.py:38-50): the scaled dot product of every seed's query with its neighbours' keys,
the softmax over each segment, dropout, and the weighted sum of the neighbours' values, with an edge term added to key
and value,

    h = dot_attention(q[seed_local], k, v, nbr_local, S, counts=deg, edge=e, heads=2, dropout=0.1, seed=seed, call=step)

one launch going forward, and neither `k[index] + e` nor `v[index] + e` is ever materialised.

pair_dot is the scoring step of the reference's unsupervised models (examples/tf/sage/train.py:56-57,
python/nn/tf/loss.py:58): the dot product of the two endpoint embeddings of an edge, and of a source with each of its
K sampled negatives,

    pos = pair_dot(z, l_src, z, l_dst)                                 # [B]
    neg = pair_dot(z, l_src, z, l_neg.view(B, K))                      # [B, K]

without the two [n, D] gathers of `(z[src].unsqueeze(1) * z[neg]).sum(-1)` and without their index_add_ backwards.

Hub rows.  By default one lane group adds all the terms of a row, in ascending position; a row that thousands of
positions name -- the hubs an EdgeWeight sampler keeps drawing -- makes the whole backward wait for that one walk.
segment_aggregate, gather_rows and weighted_segment_aggregate take chunked_grad=True to sum x.grad in the CHUNKED order
instead (glx_aggregate_backward_chunked, glx_aggregate_weighted_backward_x_chunked): chunks of 256 of a row's positions
are summed apart, each from +0.0 in ascending position, and the partial sums are added in chunk order.  As
deterministic as the default, the default's bits for every row named at most 256 times, other bits beyond; forward
outputs do not depend on the flag.  dot_attention takes chunked=True, which covers BOTH directions: a hub SEGMENT (more
than 256 positions) has its softmax computed by one workgroup and its out / grad_q summed chunk by chunk, and k.grad /
v.grad are summed in the chunked order above (glx_dot_attention_chunked, glx_dot_attention_backward_chunked).  pair_dot
and gat_attention have no such flag: pair_dot's gradients and gat_attention's gradient of t stay unsplit.

bfloat16.  Under torch.autocast("cuda", dtype=torch.bfloat16) `z = relu(enc(x))` is bfloat16, and segment_aggregate,
gather_rows, weighted_segment_aggregate and pair_dot take it as it is -- inside autocast or outside, they go by the
dtype they are handed.  Every row is upcast exactly as it is loaded and everything else is the float32 arithmetic in the
float32 order: the outputs are float32 and torch.equal the call on `z.float()`.  `z.grad` is bfloat16, written by the
backward kernel itself: the float32 gradient, summed in float32, rounded ONCE per element to nearest even (within 2^-9
relative of it; a NaN is 0xFFFF) -- no float32 [N, D] gradient is allocated.  When one bfloat16 tensor feeds two ops
torch adds their two bfloat16 gradients in bfloat16: one more rounding, torch's.  weights, logits and incoming gradients
stay float32; float16 (its gradients need loss scaling), float64 and float8 raise, and so do bfloat16 inputs to
segment_softmax, gat_attention and dot_attention.
"""
import torch

__all__ = ["segment_aggregate", "gather_rows", "weighted_segment_aggregate", "segment_softmax", "gat_attention",
           "dot_attention", "pair_dot"]

_OPS = {"sum": 0, "mean": 1, "max": 2, "min": 3, "prod": 4}


def _glx():
  import graphlearn.graph  # noqa: F401  (puts the engine's ctypes harness on sys.path)
  import glx
  return glx


def _check_inputs(x, index, who):
  if not isinstance(x, torch.Tensor) or not isinstance(index, torch.Tensor):
    raise ValueError("{}: x and index must be torch tensors".format(who))
  if x.dtype not in (torch.float32, torch.bfloat16):
    raise ValueError("{}: x must be float32 or bfloat16, not {} (bfloat16 is the half type whose gradient has a "
                     "contract: float16 gradients need loss scaling, float8 tables have no backward)".format(
                         who, x.dtype))
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


def _dtype_name(x):
  return str(x.dtype).replace("torch.", "")


def _no_double_backward(who):
  # the engine runs a backward with grad mode on only when it was asked to build a graph of it (create_graph=True)
  if torch.is_grad_enabled():
    raise ValueError("{}: double backward is not supported".format(who))


class _SegmentAggregate(torch.autograd.Function):

  @staticmethod
  def forward(ctx, x, index, segment_ids, num_segments, op, default_attr, chunked_grad):
    glx = _glx()
    ctx.chunked = chunked_grad  # selects the backward entry point only
    feats = glx.Features(x.detach(), view=True, device=x.device.index or 0)
    arg = None
    if op in (glx.MAX, glx.MIN):
      emb, cnt, arg = feats.aggregate_arg(op, index, segment_ids, num_segments, default_attr)
    else:
      emb, cnt = feats.aggregate(op, index, segment_ids, num_segments, default_attr)
    ctx.op, ctx.num_rows, ctx.x_dtype = op, int(x.shape[0]), _dtype_name(x)
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
    # x.grad in x's own dtype straight from the kernel: no float32 [N, D] gradient exists for a bfloat16 x
    gx = _glx().aggregate_backward(ctx.op, index, None if ctx.implied else cnt, grad, ctx.num_rows, arg=arg,
                                   out_dtype=ctx.x_dtype, chunked=ctx.chunked)
    return gx, None, None, None, None, None, None


def segment_aggregate(x, index, num_segments, op="mean", segment_ids=None, default_attr=0.0, chunked_grad=False):
  """[num_segments, D]: segment s reduces the rows x[index[p]] of its positions p with `op` ("sum", "mean", "max",
  "min"; "prod" only for an x that needs no gradient), exactly as glx.Features(x, view=True).aggregate does -- the
  engine's tuned reduce, left to right, bit-identical on every run.

  x            [N, D] contiguous float32 or bfloat16 CUDA tensor; may require grad.  The result is float32 either way
               (bfloat16: that of x.float(), bit for bit); x.grad has x's dtype (bfloat16: the float32 gradient rounded
               once per element)
  index        int64 CUDA tensor of any shape (flattened): rows of x; a value outside [0, N) reads a row of
               `default_attr` and receives no gradient
  segment_ids  None: num_segments equal segments of index.numel() / num_segments consecutive positions (a dense
               sampler response); or an int32 tensor like index, consumed with the reference's cursor rule
               (non-decreasing ids in [0, num_segments); everything behind the first violation is ignored)
  chunked_grad False: x.grad adds its terms in ascending request position.  True: the CHUNKED order
               (glx_aggregate_backward_chunked) -- a row's positions are cut into chunks of 256, each chunk summed from
               +0.0 by its own lane group, the partial sums added in chunk order: as deterministic, other bits for a
               row referenced more than 256 times, the same bits otherwise.  For batches with hub rows.  The forward
               does not depend on it
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
  return _SegmentAggregate.apply(x, index, segment_ids, num_segments, _OPS[op], float(default_attr),
                                 bool(chunked_grad))


class _GatherRows(torch.autograd.Function):

  @staticmethod
  def forward(ctx, x, index, default_attr, chunked_grad):
    glx = _glx()
    out = glx.Features(x.detach(), view=True, device=x.device.index or 0).lookup(index, default_attr)
    ctx.num_rows, ctx.x_dtype, ctx.chunked = int(x.shape[0]), _dtype_name(x), chunked_grad
    ctx.save_for_backward(index)
    return out

  @staticmethod
  def backward(ctx, grad):
    _no_double_backward("gather_rows")
    (index,) = ctx.saved_tensors
    glx = _glx()
    grad = grad.to(torch.float32).contiguous()
    # one position per segment: the Sum backward of the implied layout
    gx = glx.aggregate_backward(glx.SUM, index, None, grad, ctx.num_rows, out_dtype=ctx.x_dtype, chunked=ctx.chunked)
    return gx, None, None, None


def gather_rows(x, index, default_attr=0.0, chunked_grad=False):
  """x[index] as [*index.shape, D] -- the engine's lookup going forward, the deterministic Sum backward (one position
  per segment) going back: the replacement for `z[local[h]]` whose backward is index_add_ with float atomics.  A value
  of index outside [0, N) reads a row of `default_attr` and receives no gradient.  x is float32 or bfloat16; the rows
  come back as float32 (a bfloat16 x: upcast exactly), x.grad has x's dtype.  chunked_grad=True sums x.grad in
  segment_aggregate's chunked order (a row gathered more than 256 times: partial sums of 256 positions each, added in
  order -- the bits of glx.rows_coalesce); the rows that come back do not depend on it."""
  _check_inputs(x, index, "gather_rows")
  shape = tuple(index.shape)
  out = _GatherRows.apply(x, index.reshape(-1).contiguous(), float(default_attr), bool(chunked_grad))
  return out.reshape(shape + (int(x.shape[1]),))


class _WeightedSegmentAggregate(torch.autograd.Function):

  @staticmethod
  def forward(ctx, x, index, weights, counts, num_segments, op, default_attr, chunked_grad):
    glx = _glx()
    xd, wd = x.detach(), weights.detach()
    emb = glx.aggregate_weighted(op, xd, index, wd, num_segments, cnt=counts, default_attr=default_attr)
    ctx.op, ctx.default_attr, ctx.has_counts = op, default_attr, counts is not None
    ctx.chunked = chunked_grad  # selects the row gradient's entry point only
    ctx.save_for_backward(*([xd, index, wd] + ([counts] if counts is not None else [])))
    return emb

  @staticmethod
  def backward(ctx, grad):
    _no_double_backward("weighted_segment_aggregate")
    glx = _glx()
    saved = ctx.saved_tensors
    x, index, w = saved[0], saved[1], saved[2]
    counts = saved[3] if ctx.has_counts else None
    grad = grad.to(torch.float32).contiguous()
    gx = gw = None
    if ctx.needs_input_grad[0]:
      gx = glx.aggregate_weighted_backward_x(ctx.op, index, w, counts, grad, int(x.shape[0]), out_dtype=_dtype_name(x),
                                             chunked=ctx.chunked)
    if ctx.needs_input_grad[2]:
      gw = glx.aggregate_weighted_backward_w(ctx.op, x, index, int(w.shape[1]), counts, grad, ctx.default_attr)
    return gx, None, gw, None, None, None, None, None


def weighted_segment_aggregate(x, index, weights, num_segments, op="sum", counts=None, default_attr=0.0,
                               chunked_grad=False):
  """[num_segments, D]: segment s is the weighted "sum" or "mean" of the rows x[index[p]] of its positions p, each row
  scaled per head by weights[p] before it is added -- fadd(acc, fmul(w, x)) left to right, bit-identical on every run.

  x        [N, D] contiguous float32 or bfloat16 CUDA tensor; may require grad.  The result and the weights' gradient
           are float32 either way (bfloat16: those of x.float(), bit for bit); x.grad has x's dtype (bfloat16: the
           float32 gradient rounded once per element)
  index    int64 CUDA tensor of any shape (flattened, n positions): rows of x; a value outside [0, N) reads a row of
           `default_attr` and passes no gradient to x (its weight still gets one)
  weights  [n] or [n, H] float32 (never bfloat16) on x's device, H dividing D: column c of a row is scaled by head c // (D // H); may
           require grad.  The gradient has the shape of `weights`; each element is a dot product over its head's
           columns with a fixed summation tree (the same bits on every run, no atomics)
  counts   None: num_segments equal segments of n / num_segments consecutive positions (a dense sampler response); or
           an int32 [num_segments] tensor: segment s is the next counts[s] positions, positions from counts.sum() on are
           ignored and get a zero weight gradient
  chunked_grad  True: x.grad sums its terms in segment_aggregate's chunked order
           (glx_aggregate_weighted_backward_x_chunked); the result and the weights' gradient do not depend on it
  Empty segments are `default_attr` and pass no gradient on.  Anything else raises ValueError.
  """
  who = "weighted_segment_aggregate"
  _check_inputs(x, index, who)
  if op not in ("sum", "mean"):
    raise ValueError("{}: op must be 'sum' or 'mean', not {!r} (max / min / prod take no weights)".format(who, op))
  num_segments = int(num_segments)
  if num_segments < 0:
    raise ValueError("{}: num_segments must be >= 0".format(who))
  index = index.reshape(-1).contiguous()
  n, D = index.numel(), int(x.shape[1])
  if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32:
    raise ValueError("{}: weights must be a float32 tensor".format(who))
  if weights.device != x.device:
    raise ValueError("{}: weights live on {}, x on {}".format(who, weights.device, x.device))
  if weights.dim() not in (1, 2) or weights.shape[0] != n:
    raise ValueError("{}: weights must be [n] or [n, H] with one row per index ({}), not {}".format(
        who, n, tuple(weights.shape)))
  heads = 1 if weights.dim() == 1 else int(weights.shape[1])
  if heads < 1 or D % heads != 0:
    raise ValueError("{}: the number of heads ({}) must divide D ({})".format(who, heads, D))
  if counts is not None:
    if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or counts.device != x.device:
      raise ValueError("{}: counts must be an int32 tensor on x's device".format(who))
    if counts.dim() != 1 or counts.numel() != num_segments:
      raise ValueError("{}: counts must have one entry per segment".format(who))
    counts = counts.contiguous()
  elif num_segments == 0 or n % num_segments != 0:
    raise ValueError("{}: without counts, index.numel() must be a multiple of num_segments".format(who))
  if num_segments * D > 2 ** 31 - 1 or n * heads > 2 ** 31 - 1:
    raise ValueError("{}: num_segments * D or n * H exceeds int32".format(who))
  out = _WeightedSegmentAggregate.apply(x, index, weights.reshape(n, heads).contiguous(), counts, num_segments,
                                        _OPS[op], float(default_attr), bool(chunked_grad))
  return out


class _SegmentSoftmax(torch.autograd.Function):

  @staticmethod
  def forward(ctx, e, counts, num_segments):
    alpha = _glx().segment_softmax(e.detach(), num_segments, cnt=counts)
    ctx.num_segments, ctx.has_counts = num_segments, counts is not None
    ctx.save_for_backward(*([alpha] + ([counts] if counts is not None else [])))
    return alpha

  @staticmethod
  def backward(ctx, grad):
    _no_double_backward("segment_softmax")
    if not ctx.needs_input_grad[0]:
      return None, None, None
    saved = ctx.saved_tensors
    alpha = saved[0]
    counts = saved[1] if ctx.has_counts else None
    grad = grad.to(torch.float32).contiguous()
    return _glx().segment_softmax_backward(alpha, grad, counts, ctx.num_segments), None, None


def segment_softmax(e, num_segments, counts=None):
  """A tensor of e's shape: the softmax of the logits over each segment's positions, independently per head --
  exp(e - max) / sum exp(e - max) with the accurate exp and no epsilon, bit-identical on every run.

  e        [n] or [n, H] contiguous float32 CUDA tensor: one row of logits per position; may require grad
  counts   None: num_segments equal segments of n / num_segments consecutive positions (a dense sampler response); or
           an int32 [num_segments] tensor (what Graph.sample_full returns as degrees): segment s is the next counts[s]
           positions; positions from counts.sum() on are ignored: they are 0 and get a zero gradient
  A -inf logit among finite ones is exactly 0 (a mask); a NaN or +inf logit, or a segment of -inf only, makes that
  head's column of the segment NaN, as torch.softmax does.  Anything else raises ValueError.
  """
  who = "segment_softmax"
  if not isinstance(e, torch.Tensor):
    raise ValueError("{}: e must be a torch tensor".format(who))
  if e.dtype != torch.float32:
    raise ValueError("{}: e must be float32, not {} (half logits are not supported)".format(who, e.dtype))
  if not e.is_cuda or e.dim() not in (1, 2) or not e.is_contiguous():
    raise ValueError("{}: e must be a contiguous [n] or [n, H] CUDA tensor".format(who))
  n = int(e.shape[0])
  heads = 1 if e.dim() == 1 else int(e.shape[1])
  if heads < 1:
    raise ValueError("{}: e must have at least one head".format(who))
  num_segments = int(num_segments)
  if num_segments < 0:
    raise ValueError("{}: num_segments must be >= 0".format(who))
  if counts is not None:
    if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or counts.device != e.device:
      raise ValueError("{}: counts must be an int32 tensor on e's device".format(who))
    if counts.dim() != 1 or counts.numel() != num_segments:
      raise ValueError("{}: counts must have one entry per segment".format(who))
    counts = counts.contiguous()
  elif num_segments == 0 or n % num_segments != 0:
    raise ValueError("{}: without counts, e.shape[0] must be a multiple of num_segments".format(who))
  if n * heads > 2 ** 31 - 1:
    raise ValueError("{}: n * H exceeds int32".format(who))
  return _SegmentSoftmax.apply(e, counts, num_segments)


class _GatAttention(torch.autograd.Function):

  @staticmethod
  def forward(ctx, s, t, index, counts, slope, drop_p, seed, call, default_attr):
    sd, td = s.detach(), t.detach()
    alpha, soft = _glx().gat_attention(sd, td, index, cnt=counts, negative_slope=slope, default_attr=default_attr,
                                       drop_p=drop_p, seed=seed, call=call, want_soft=drop_p != 0.0)
    ctx.cfg = (slope, default_attr, drop_p, seed, call)
    ctx.has_counts = counts is not None
    ctx.save_for_backward(*([alpha if soft is None else soft, sd, td, index] + ([counts] if counts is not None else [])))
    return alpha

  @staticmethod
  def backward(ctx, grad):
    _no_double_backward("gat_attention")
    want_s, want_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    if not (want_s or want_t):
      return (None,) * 9
    saved = ctx.saved_tensors
    soft, s, t, index = saved[:4]
    counts = saved[4] if ctx.has_counts else None
    slope, default_attr, drop_p, seed, call = ctx.cfg
    grad = grad.to(torch.float32).contiguous()
    _, gs, gt = _glx().gat_attention_backward(soft, grad, s, t, index, cnt=counts, negative_slope=slope,
                                              default_attr=default_attr, drop_p=drop_p, seed=seed, call=call,
                                              want_s=want_s, want_t=want_t)
    return (gs, gt) + (None,) * 7


def gat_attention(s, t, index, num_segments, counts=None, negative_slope=0.2, dropout=0.0, seed=0, call=0,
                  default_attr=0.0):
  """[n, H] attention coefficients of a GAT layer: for position p of segment sg and head h the logit
  leaky_relu(s[sg, h] + t[index[p], h], negative_slope), its softmax over the segment's positions (segment_softmax's
  definition and exact rules) and dropout on the result -- one kernel going forward, one going back, no atomics,
  bit-identical on every run.

  s        [S, H] or [S] contiguous float32 CUDA tensor, S == num_segments: the segment's half of the logit (a GAT
           layer's attn_src of each seed); may require grad
  t        [M, H] or [M] like s: the neighbour's half, one row per node; may require grad
  index    int64 CUDA tensor of any shape (flattened, n positions): rows of t.  A value outside [0, M) reads
           `default_attr` and passes no gradient to t; default_attr=float("-inf") is the mask for padded neighbours
           (index -1): such a position gets exactly 0
  counts   None: num_segments equal segments of n / num_segments positions; or an int32 [num_segments] tensor: segment
           sg is the next counts[sg] positions, positions from counts.sum() on are 0
  dropout  p in [0, 1): element (p, h) is kept, and scaled by 1 / (1 - p), iff word (p H + h) % 4 of Philox4x32-10
           block (p H + h) // 4 under (seed, call) is >= floor(p 2^32) -- the engine's contract generator; the
           backward recomputes the mask.  Use a new `call` for every step.
  Only the gradients that are needed are computed.  Anything else raises ValueError.
  """
  who = "gat_attention"
  for name, x in (("s", s), ("t", t)):
    if not isinstance(x, torch.Tensor):
      raise ValueError("{}: {} must be a torch tensor".format(who, name))
    if x.dtype != torch.float32:
      raise ValueError("{}: {} must be float32, not {}".format(who, name, x.dtype))
    if not x.is_cuda or x.dim() not in (1, 2) or not x.is_contiguous():
      raise ValueError("{}: {} must be a contiguous [N] or [N, H] CUDA tensor".format(who, name))
  if not isinstance(index, torch.Tensor) or index.dtype != torch.int64:
    raise ValueError("{}: index must be an int64 tensor".format(who))
  if t.device != s.device or index.device != s.device:
    raise ValueError("{}: s, t and index must live on one device".format(who))
  heads = 1 if s.dim() == 1 else int(s.shape[1])
  if heads < 1 or (1 if t.dim() == 1 else int(t.shape[1])) != heads:
    raise ValueError("{}: s and t must have the same number (>= 1) of heads".format(who))
  num_segments = int(num_segments)
  if num_segments < 0 or int(s.shape[0]) != num_segments:
    raise ValueError("{}: s must have one row per segment ({}), not {}".format(who, num_segments, int(s.shape[0])))
  index = index.reshape(-1).contiguous()
  n = index.numel()
  if counts is not None:
    if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or counts.device != s.device:
      raise ValueError("{}: counts must be an int32 tensor on s's device".format(who))
    if counts.dim() != 1 or counts.numel() != num_segments:
      raise ValueError("{}: counts must have one entry per segment".format(who))
    counts = counts.contiguous()
  elif num_segments == 0 or n % num_segments != 0:
    raise ValueError("{}: without counts, index.numel() must be a multiple of num_segments".format(who))
  if n * heads > 2 ** 31 - 1 or num_segments * heads > 2 ** 31 - 1:
    raise ValueError("{}: n * H or num_segments * H exceeds int32".format(who))
  negative_slope, dropout = float(negative_slope), float(dropout)
  if not (negative_slope >= 0.0 and negative_slope != float("inf")):
    raise ValueError("{}: negative_slope must be finite and >= 0".format(who))
  if not 0.0 <= dropout < 1.0:
    raise ValueError("{}: dropout must lie in [0, 1)".format(who))
  seed, call = int(seed), int(call)
  if not (0 <= seed < 2 ** 64 and 0 <= call < 2 ** 64):
    raise ValueError("{}: seed and call must fit 64 unsigned bits".format(who))
  return _GatAttention.apply(s.reshape(num_segments, heads), t.reshape(int(t.shape[0]), heads), index, counts,
                             negative_slope, dropout, seed, call, float(default_attr))


class _DotAttention(torch.autograd.Function):

  @staticmethod
  def forward(ctx, q, k, v, edge, index, counts, heads, scale, drop_p, seed, call, default_attr, chunked):
    qd, kd, vd = q.detach(), k.detach(), v.detach()
    ed = None if edge is None else edge.detach()
    out, soft, _ = _glx().dot_attention(qd, kd, vd, index, cnt=counts, edge=ed, heads=heads, scale=scale,
                                        default_attr=default_attr, drop_p=drop_p, seed=seed, call=call, chunked=chunked)
    ctx.cfg = (heads, scale, default_attr, drop_p, seed, call)
    ctx.chunked = chunked  # selects the entry point of both directions
    ctx.has_edge, ctx.has_counts = ed is not None, counts is not None
    ctx.save_for_backward(*([soft, qd, kd, vd, index] + ([ed] if ed is not None else []) +
                            ([counts] if counts is not None else [])))
    return out

  @staticmethod
  def backward(ctx, grad):
    _no_double_backward("dot_attention")
    want_q, want_k, want_v, want_e = ctx.needs_input_grad[:4]
    if not (want_q or want_k or want_v or want_e):
      return (None,) * 13
    saved = list(ctx.saved_tensors)
    soft, q, k, v, index = saved[:5]
    edge = saved[5] if ctx.has_edge else None
    counts = saved[-1] if ctx.has_counts else None
    heads, scale, default_attr, drop_p, seed, call = ctx.cfg
    grad = grad.to(torch.float32).contiguous()
    _, gq, gk, gv, ge = _glx().dot_attention_backward(soft, grad, q, k, v, index, cnt=counts, edge=edge, heads=heads,
                                                      scale=scale, default_attr=default_attr, drop_p=drop_p, seed=seed,
                                                      call=call, want_q=want_q, want_k=want_k, want_v=want_v,
                                                      want_edge=want_e, chunked=ctx.chunked)
    return (gq, gk, gv, ge) + (None,) * 9


def dot_attention(q, k, v, index, num_segments, counts=None, edge=None, heads=1, scale=None, dropout=0.0, seed=0, call=0,
                  default_attr=0.0, chunked=False):
  """[S, D]: scaled dot-product attention of every segment over its positions.  For position p of segment sg and head
  h (columns [h C, (h + 1) C), C = D / heads): the logit scale * (q[sg] . (k[index[p]] + edge[p])) over the head's
  columns, its softmax over the segment's positions (segment_softmax's definition and exact rules), gat_attention's
  dropout on the coefficients, and out[sg] = the sum over p, in ascending order, of alpha[p, h] * (v[index[p]] + edge[p])
  -- one kernel going forward, no atomics in either direction, bit-identical on every run.

  q        [S, D] contiguous float32 CUDA tensor, S == num_segments: one query per segment; may require grad
  k, v     [M, D] like q: the key and the value of every node; may require grad, and may be one tensor (autograd then
           adds the two gradients: one more float32 add per element)
  index    int64 CUDA tensor of any shape (flattened, n positions): rows of k and v.  A value outside [0, M) reads a
           row of `default_attr` in both and passes no gradient to them
  counts   None: num_segments equal segments of n / num_segments positions; or an int32 [num_segments] tensor: segment
           sg is the next counts[sg] positions, positions from counts.sum() on are ignored.  There is no mask for padded
           neighbours beyond counts
  edge     None, or [n, D] like q: the edge term of every position, added to its key and to its value; may require grad
  scale    None: 1 / sqrt(C), rounded to float32; or a finite float
  dropout  p in [0, 1), with gat_attention's mask under (seed, call).  Use a new `call` for every step.
  chunked  True: the CHUNKED order in both directions, for batches with hub segments (glx_dot_attention_chunked,
           glx_dot_attention_backward_chunked).  A segment of more than 256 positions is normalised by one workgroup and
           its sums (out, q.grad) add chunks of 256 positions apart, each from +0.0 in ascending position, then the
           partial sums in chunk order; k.grad and v.grad use weighted_segment_aggregate's chunked_grad order.  As
           deterministic as the default.  The forward of a request without such segments, and the gradients of one that
           also names no row more than 256 times, are the default's bits
  An empty segment is 0.  Only the gradients that are needed are computed.  Anything else raises ValueError.
  """
  who = "dot_attention"
  for name, x in (("q", q), ("k", k), ("v", v)) + ((("edge", edge),) if edge is not None else ()):
    if not isinstance(x, torch.Tensor):
      raise ValueError("{}: {} must be a torch tensor".format(who, name))
    if x.dtype != torch.float32:
      raise ValueError("{}: {} must be float32, not {}".format(who, name, x.dtype))
    if not x.is_cuda or x.dim() != 2 or not x.is_contiguous():
      raise ValueError("{}: {} must be a contiguous [N, D] CUDA tensor".format(who, name))
    if x.device != q.device:
      raise ValueError("{}: {} lives on {}, q on {}".format(who, name, x.device, q.device))
  if not isinstance(index, torch.Tensor) or index.dtype != torch.int64:
    raise ValueError("{}: index must be an int64 tensor".format(who))
  if index.device != q.device:
    raise ValueError("{}: index lives on {}, q on {}".format(who, index.device, q.device))
  D, heads = int(q.shape[1]), int(heads)
  if D < 1 or int(k.shape[1]) != D or tuple(v.shape) != tuple(k.shape):
    raise ValueError("{}: q [S, D], k [M, D] and v [M, D] must agree on D >= 1 and M".format(who))
  if heads < 1 or D % heads != 0:
    raise ValueError("{}: the number of heads ({}) must divide D ({})".format(who, heads, D))
  num_segments = int(num_segments)
  if num_segments < 0 or int(q.shape[0]) != num_segments:
    raise ValueError("{}: q must have one row per segment ({}), not {}".format(who, num_segments, int(q.shape[0])))
  index = index.reshape(-1).contiguous()
  n = index.numel()
  if edge is not None and tuple(edge.shape) != (n, D):
    raise ValueError("{}: edge must be [n, D] = {}, not {}".format(who, (n, D), tuple(edge.shape)))
  if counts is not None:
    if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or counts.device != q.device:
      raise ValueError("{}: counts must be an int32 tensor on q's device".format(who))
    if counts.dim() != 1 or counts.numel() != num_segments:
      raise ValueError("{}: counts must have one entry per segment".format(who))
    counts = counts.contiguous()
  elif num_segments == 0 or n % num_segments != 0:
    raise ValueError("{}: without counts, index.numel() must be a multiple of num_segments".format(who))
  if n * heads > 2 ** 31 - 1 or num_segments * D > 2 ** 31 - 1:
    raise ValueError("{}: n * H or num_segments * D exceeds int32".format(who))
  if scale is None:
    scale = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(D // heads), dtype=torch.float32).sqrt())
  scale, dropout = float(scale), float(dropout)
  if scale != scale or scale in (float("inf"), float("-inf")):
    raise ValueError("{}: scale must be finite".format(who))
  if not 0.0 <= dropout < 1.0:
    raise ValueError("{}: dropout must lie in [0, 1)".format(who))
  seed, call = int(seed), int(call)
  if not (0 <= seed < 2 ** 64 and 0 <= call < 2 ** 64):
    raise ValueError("{}: seed and call must fit 64 unsigned bits".format(who))
  return _DotAttention.apply(q, k, v, edge, index, counts, heads, scale, dropout, seed, call, float(default_attr),
                             bool(chunked))


class _PairDot(torch.autograd.Function):

  @staticmethod
  def forward(ctx, xa, ia, xb, ib, heads, repeat, default_attr):
    xad, xbd = xa.detach(), xb.detach()
    out = _glx().pair_dot(xad, ia, xbd, ib, heads=heads, repeat=repeat, default_attr=default_attr)
    ctx.repeat, ctx.default_attr = repeat, default_attr
    ctx.save_for_backward(xad, ia, xbd, ib)
    return out

  @staticmethod
  def backward(ctx, grad):
    _no_double_backward("pair_dot")
    glx = _glx()
    xa, ia, xb, ib = ctx.saved_tensors
    grad = grad.to(torch.float32).contiguous()
    ga = gb = None
    if ctx.needs_input_grad[0]:
      ga = glx.pair_dot_backward(0, ia, ib, grad, xb, int(xa.shape[0]), repeat=ctx.repeat, default_attr=ctx.default_attr)
    if ctx.needs_input_grad[2]:
      gb = glx.pair_dot_backward(1, ia, ib, grad, xa, int(xb.shape[0]), repeat=ctx.repeat, default_attr=ctx.default_attr)
    return ga, None, gb, None, None, None, None


def pair_dot(xa, ia, xb, ib, heads=None, default_attr=0.0):
  """The score of every pair (ia, ib): the dot product of row ia of xa with row ib of xb, per head -- a fixed summation
  tree going forward, fadd(acc, fmul(g, row)) in ascending pair order going back, no atomics: bit-identical on every
  run.  Neither [n, D] gather is materialised.

  xa, xb   [Na, D], [Nb, D] contiguous CUDA tensors on one device, both float32 or both bfloat16; either may require
           grad, and they may be one tensor (autograd then adds the two sides' gradients: one more add per element, in
           the tables' dtype -- for bfloat16 one more rounding, torch's).  The scores are float32 either way (bfloat16:
           those of the .float() tables, bit for bit); each gradient has its table's dtype (bfloat16: the float32
           gradient rounded once per element)
  ib       int64 CUDA tensor of any shape (n pairs): rows of xb
  ia       int64 CUDA tensor (flattened) whose numel divides n: rows of xa; pair p takes ia[p // (n / ia.numel())] -- ia
           [B] with ib [B, K] scores each source against its K candidates; ia shaped like ib scores edges one to one
  heads    None: a tensor of ib's shape; H (dividing D): ib.shape + (H,), column c belongs to head c // (D // H)
  An index outside its table reads a row of `default_attr` and receives no gradient.  Only the gradients that are
  needed are computed.  Anything else raises ValueError.
  """
  who = "pair_dot"
  _check_inputs(xa, ia, who)
  _check_inputs(xb, ib, who)
  if xb.device != xa.device:
    raise ValueError("{}: xb lives on {}, xa on {}".format(who, xb.device, xa.device))
  if xb.dtype != xa.dtype:
    raise ValueError("{}: xa is {} and xb {}: both tables must have one dtype".format(who, xa.dtype, xb.dtype))
  D = int(xa.shape[1])
  if int(xb.shape[1]) != D:
    raise ValueError("{}: xa has {} columns, xb {}".format(who, D, int(xb.shape[1])))
  H = 1 if heads is None else int(heads)
  if H < 1 or D % H != 0:
    raise ValueError("{}: the number of heads ({}) must divide D ({})".format(who, H, D))
  shape = tuple(ib.shape)
  ia, ib = ia.reshape(-1).contiguous(), ib.reshape(-1).contiguous()
  n, m = ib.numel(), ia.numel()
  if (m == 0 and n != 0) or (m != 0 and n % m != 0):
    raise ValueError("{}: ia.numel() ({}) must divide ib.numel() ({})".format(who, m, n))
  if n * H > 2 ** 31 - 1:
    raise ValueError("{}: n * H exceeds int32".format(who))
  repeat = n // m if n else 1
  out = _PairDot.apply(xa, ia, xb, ib, H, repeat, float(default_attr))
  return out.reshape(shape if heads is None else shape + (H,))
