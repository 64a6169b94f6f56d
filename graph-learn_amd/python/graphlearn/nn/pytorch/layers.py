"""Model layers over the engine's deterministic training-path ops.

GATConv is the reference's multi-head GAT layer (graphlearn/python/nn/tf/layers/gat_conv.py:29-119) for a sampled
batch: one row of features per distinct node, the seeds' positions among them, and the neighbours of every seed as one
segment of a counts= request (a FullSampler hop) or of the implied layout (a fixed fan-out).

TransformerConv is the layer of the reference's GPU PyTorch model (graphlearn/examples/pytorch/tgn/train_and_eval.py:38-50:
TransformerConv(in, out // 2, heads=2, dropout=0.1, edge_dim=...)) over the same batches: scaled dot-product attention of
every seed over its neighbours, with the edge features mapped into the key and the value.
"""
import torch

from graphlearn.nn.pytorch.segment import dot_attention, gat_attention, gather_rows, weighted_segment_aggregate

__all__ = ["GATConv", "TransformerConv"]


class GATConv(torch.nn.Module):
  """out[s] = sum over the neighbours u of seed s of alpha[s, u, h] * (W x_u)[h], per head h, with
  alpha = dropout(softmax_u(leaky_relu(a_src[h] . (W x_s)[h] + a_dst[h] . (W x_u)[h]))) -- gat_conv.py:84-119.

  in_dim, out_dim   columns of x_nodes and of each head's output
  num_heads         H; concat=True returns [S, H * out_dim], concat=False the mean over the heads, [S, out_dim]
  dropout           on the attention coefficients, in training mode only (gat_conv.py:103-104).  The mask is the
                    engine's contract generator under (seed, call): `seed` defaults to torch.initial_seed() (read at
                    each forward) and `call` counts this module's training forwards, so after torch.manual_seed two
                    runs of one script give the same bits.  Layers that share a seed share their masks position by
                    position: give each layer of a model its own seed.
  use_bias          a bias of the OUTPUT's shape: [H * out_dim] when concat, [out_dim] otherwise.  (The reference has
                    the two shapes swapped, gat_conv.py:59-67: [out_dim] when concat, which cannot be added to its
                    [N, H * out_dim] output unless H == 1.)
  add_self_loops    every seed also attends to itself (gat_conv.py:85-87): its own row is inserted as one more
                    position of its segment, behind its neighbours

  Everything runs on one GPU; the segments are described by counts (or the implied layout), not by explicit segment
  ids.  In float32 every op is float32.  Under torch.autocast("cuda", dtype=torch.bfloat16) the projection z = W x is
  bfloat16; the two halves of the logit come out float32 (type promotion against the float32 attention parameters), so
  gat_attention runs in float32 as ever, and weighted_segment_aggregate reads the bfloat16 z as it is: the output and
  every parameter gradient equal, bit for bit, those of the same steps with z.float() handed to the reduce, and z's
  gradient is the float32 one rounded once per element (segment.py).
  """

  def __init__(self, in_dim, out_dim, num_heads=1, concat=False, dropout=0.0, use_bias=False, negative_slope=0.2,
               add_self_loops=True, seed=None):
    super().__init__()
    in_dim, out_dim, num_heads = int(in_dim), int(out_dim), int(num_heads)
    if in_dim < 1 or out_dim < 1 or num_heads < 1:
      raise ValueError("GATConv: in_dim, out_dim and num_heads must be positive")
    if not 0.0 <= float(dropout) < 1.0:
      raise ValueError("GATConv: dropout must lie in [0, 1)")
    self.in_dim, self.out_dim, self.num_heads = in_dim, out_dim, num_heads
    self.concat, self.dropout, self.negative_slope = bool(concat), float(dropout), float(negative_slope)
    self.add_self_loops = bool(add_self_loops)
    self.seed = None if seed is None else int(seed)
    self.calls = 0  # training forwards so far: the `call` of the next dropout mask
    self.linear = torch.nn.Linear(in_dim, num_heads * out_dim, bias=False)
    self.attn_src = torch.nn.Parameter(torch.empty(1, num_heads, out_dim))
    self.attn_dst = torch.nn.Parameter(torch.empty(1, num_heads, out_dim))
    torch.nn.init.xavier_uniform_(self.attn_src)
    torch.nn.init.xavier_uniform_(self.attn_dst)
    if use_bias:
      self.bias = torch.nn.Parameter(torch.zeros(num_heads * out_dim if self.concat else out_dim))
    else:
      self.register_parameter("bias", None)

  @staticmethod
  def with_self_loops(seed_local, index, counts, num_segments):
    """(index, counts) with seed s's own row behind the consumed positions of segment s: device-side index
    arithmetic, nothing is read back.  Positions that no segment consumed stay behind all the segments."""
    if counts is None:
      return torch.cat([index.reshape(num_segments, -1), seed_local.reshape(-1, 1)], dim=1).reshape(-1), None
    index = index.reshape(-1)
    n = index.numel()
    seg = torch.arange(num_segments, device=index.device)
    ends = torch.cumsum(counts.clamp(min=0).long(), 0).clamp(max=n)
    seg_of = torch.searchsorted(ends, torch.arange(n, device=index.device), right=True)
    out = torch.empty(n + num_segments, dtype=index.dtype, device=index.device)
    out[torch.arange(n, device=index.device) + seg_of] = index
    out[ends + seg] = seed_local
    starts = torch.cat([ends.new_zeros(1), ends[:-1]])
    return out, (ends - starts + 1).to(torch.int32)

  def forward(self, x_nodes, seed_local, index, counts=None):
    """x_nodes [M, in_dim]: the features of the batch's distinct nodes; seed_local [S] int64: the seeds' rows among
    them; index int64 (n positions, flattened): the neighbours' rows, segment s being the next counts[s] of them
    (counts int32 [S]), or n / S each when counts is None.  Returns [S, H * out_dim] or [S, out_dim]."""
    H, C = self.num_heads, self.out_dim
    seed_local = seed_local.reshape(-1)
    S = seed_local.numel()
    z = self.linear(x_nodes)                                                   # [M, H * C]
    zh = z.view(-1, H, C)
    src_e = (zh * self.attn_src).sum(-1).contiguous()                          # [M, H]
    dst_e = (zh * self.attn_dst).sum(-1).contiguous()
    s = gather_rows(src_e, seed_local)                                         # [S, H]
    if self.add_self_loops:
      index, counts = self.with_self_loops(seed_local, index, counts, S)
    drop, seed, call = 0.0, 0, 0
    if self.training and self.dropout > 0.0:
      drop = self.dropout
      seed = (torch.initial_seed() if self.seed is None else self.seed) & (2 ** 64 - 1)
      call = self.calls
      self.calls += 1
    alpha = gat_attention(s, dst_e, index, S, counts=counts, negative_slope=self.negative_slope, dropout=drop,
                          seed=seed, call=call)
    out = weighted_segment_aggregate(z, index, alpha, S, counts=counts)        # [S, H * C]
    if not self.concat:
      out = out.view(S, H, C).mean(1)
    if self.bias is not None:
      out = out + self.bias
    return out

  def extra_repr(self):
    return "in_dim={}, out_dim={}, num_heads={}, concat={}, dropout={}, negative_slope={}, add_self_loops={}".format(
        self.in_dim, self.out_dim, self.num_heads, self.concat, self.dropout, self.negative_slope, self.add_self_loops)


class TransformerConv(torch.nn.Module):
  """out[s] = sum over the neighbours u of seed s of alpha[s, u, h] * ((W_v x_u)[h] + (W_e e_su)[h]), per head h, with
  alpha = dropout(softmax_u(((W_q x_s)[h] . ((W_k x_u)[h] + (W_e e_su)[h])) / sqrt(out_dim))), plus W_skip x_s when
  root_weight -- the TransformerConv of train_and_eval.py:38-50 (Shi et al., "Masked Label Prediction", 2021) without
  its `beta` gate.  The attention, from the logits to the weighted sum, is one dot_attention call.

  in_dim, out_dim   columns of x_nodes and of each head's output
  heads             H; concat=True returns [S, H * out_dim], concat=False the mean over the heads, [S, out_dim]
  dropout           on the attention coefficients, in training mode only, seeded like GATConv: `seed` defaults to
                    torch.initial_seed() (read at each forward) and `call` counts this module's training forwards.
                    Layers that share a seed share their masks position by position: give each layer its own seed.
  edge_dim          None, or the columns of edge_attr: a bias-free linear map takes them to H * out_dim
  root_weight       add a linear map of the seed's own features (the skip connection), of the output's shape
  bias              of the query, key, value and skip maps
  chunked           passed to dot_attention: True sums a hub seed's neighbours (a segment of more than 256 positions)
                    chunk by chunk over many lane groups, in both directions, and the key and value gradients of a node
                    named more than 256 times likewise -- another fixed order, as deterministic as the default; a batch
                    without such seeds and nodes gets the default's bits.  For FullSampler hops over power-law seeds

  Every op is float32 on one GPU; the segments are described by counts (or the implied layout), not by explicit
  segment ids, and there is no mask for padded neighbours beyond counts.  dot_attention takes float32 only, so under
  bfloat16 autocast -- where the query, key and value maps come out bfloat16 -- the layer raises ValueError: run it
  outside the autocast region, or cast its projections with .float().
  """

  def __init__(self, in_dim, out_dim, heads=1, concat=True, dropout=0.0, edge_dim=None, root_weight=True, bias=True,
               seed=None, chunked=False):
    super().__init__()
    in_dim, out_dim, heads = int(in_dim), int(out_dim), int(heads)
    if in_dim < 1 or out_dim < 1 or heads < 1:
      raise ValueError("TransformerConv: in_dim, out_dim and heads must be positive")
    if not 0.0 <= float(dropout) < 1.0:
      raise ValueError("TransformerConv: dropout must lie in [0, 1)")
    if edge_dim is not None and int(edge_dim) < 1:
      raise ValueError("TransformerConv: edge_dim must be positive or None")
    self.in_dim, self.out_dim, self.heads = in_dim, out_dim, heads
    self.concat, self.dropout = bool(concat), float(dropout)
    self.edge_dim = None if edge_dim is None else int(edge_dim)
    self.seed = None if seed is None else int(seed)
    self.chunked = bool(chunked)
    self.calls = 0  # training forwards so far: the `call` of the next dropout mask
    self.lin_query = torch.nn.Linear(in_dim, heads * out_dim, bias=bool(bias))
    self.lin_key = torch.nn.Linear(in_dim, heads * out_dim, bias=bool(bias))
    self.lin_value = torch.nn.Linear(in_dim, heads * out_dim, bias=bool(bias))
    self.lin_edge = None if self.edge_dim is None else torch.nn.Linear(self.edge_dim, heads * out_dim, bias=False)
    if root_weight:
      self.lin_skip = torch.nn.Linear(in_dim, heads * out_dim if self.concat else out_dim, bias=bool(bias))
    else:
      self.lin_skip = None

  def forward(self, x_nodes, seed_local, nbr_local, counts=None, edge_attr=None):
    """x_nodes [M, in_dim]: the features of the batch's distinct nodes; seed_local [S] int64: the seeds' rows among
    them; nbr_local int64 (n positions, flattened): the neighbours' rows, segment s being the next counts[s] of them
    (counts int32 [S]), or n / S each when counts is None; edge_attr [n, edge_dim]: one row per position (required iff
    the layer has an edge map).  The query, key, value and skip maps run once per distinct node.  Returns
    [S, H * out_dim] or [S, out_dim]."""
    H, C = self.heads, self.out_dim
    seed_local = seed_local.reshape(-1)
    S = seed_local.numel()
    if (edge_attr is None) != (self.lin_edge is None):
      raise ValueError("TransformerConv: edge_attr is required iff the layer was built with edge_dim")
    q = gather_rows(self.lin_query(x_nodes), seed_local)                        # [S, H * C]
    k = self.lin_key(x_nodes)                                                   # [M, H * C]
    v = self.lin_value(x_nodes)
    edge = None if edge_attr is None else self.lin_edge(edge_attr.reshape(-1, self.edge_dim))
    drop, seed, call = 0.0, 0, 0
    if self.training and self.dropout > 0.0:
      drop = self.dropout
      seed = (torch.initial_seed() if self.seed is None else self.seed) & (2 ** 64 - 1)
      call = self.calls
      self.calls += 1
    out = dot_attention(q, k, v, nbr_local, S, counts=counts, edge=edge, heads=H, dropout=drop, seed=seed, call=call,
                        chunked=self.chunked)
    if not self.concat:
      out = out.view(S, H, C).mean(1)
    if self.lin_skip is not None:
      out = out + gather_rows(self.lin_skip(x_nodes), seed_local)
    return out

  def extra_repr(self):
    return "in_dim={}, out_dim={}, heads={}, concat={}, dropout={}, edge_dim={}, root_weight={}, chunked={}".format(
        self.in_dim, self.out_dim, self.heads, self.concat, self.dropout, self.edge_dim, self.lin_skip is not None,
        self.chunked)
