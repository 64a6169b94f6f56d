"""Device-resident mini-batch loader: the caller that sits right above the hot path in a
training loop (the role of graphlearn/python/nn/pytorch/data/{dataset,pyg_dataloader}.py,
which drive the same sample -> lookup steps through GSL and numpy).

Every batch is produced on the GPU and stays there: seed ids -> all hops in one
glx_sample_hops call -> float attributes of every frontier gathered by glx_lookup.  No
request objects, no host round trips, no worker processes: one iteration is a handful of
kernel launches on the current torch stream.

    loader = gl.NeighborLoader(g, "item", ["i2i", "i2i"], [15, 10], batch_size=1024,
                               strategy="edge_weight", shuffle=True)
    for batch in loader:                 # one epoch
        batch.seeds                      # [B] int64 cuda
        batch.nbr[h], batch.eid[h]       # hop h+1: [rows_h, fanout_h] int64 cuda
        batch.x[h]                       # float attributes of frontier h ([B, D], [B*f1, D], ...)
        src, dst = batch.edge_index(h)   # COO of hop h+1 in frontier-local positions

With dedup=True a batch is a CompactBatch: the same sample, plus the distinct node set of the batch (seeds first, in
order of first occurrence -- glx_unique, no sort), every sampled slot's position in it and ONE feature row per distinct
node instead of one per slot:

    for batch in gl.NeighborLoader(..., dedup=True):
        batch.nodes                      # [M] distinct ids; nodes[:num_nodes_upto[h]] = frontiers 0 .. h
        batch.local[h]                   # positions of frontier h in nodes, shaped like the frontier
        batch.x_nodes                    # [M, D] float attributes of nodes
        src, dst = batch.edge_index(h)   # COO of hop h+1 in node-set positions

Labels, weights, timestamps and int attributes ride along from HBM the same way (glx.Columns, one lookup per frontier,
or per node type with dedup=True); the names come from {"labels", "weights", "timestamps", "int_attrs"}:

    for batch in gl.NeighborLoader(..., node_columns=("labels", "int_attrs"), edge_columns=("weights",),
                                   edge_features=True):
        batch.y                          # [B] int32 labels of the seeds (when "labels" is asked for)
        batch.node_cols[h]["int_attrs"]  # shaped like frontier h, plus a trailing i_num axis
        batch.edge_cols[h]["weights"]    # shaped like nbr[h], gathered by eid[h] (-1 edge ids: the Default* flags)
        batch.edge_x[h]                  # [rows_h, fanout_h, D] float attributes of hop h+1's edges
        batch.node_cols_nodes[name]      # dedup=True: one row per distinct node (a dict per type like nodes)

The node set's size decides the shape of nodes / x_nodes, so each glx.unique call reads one int64 back from the device:
with dedup=True the loader waits for the stream once per node type per batch (the plain loader never does).

Seeding: batch i of epoch e uses call counter (e * batches_per_epoch + i) * hops, so a
(sampling seed, epoch, batch) triple always reproduces the same sample.

TemporalNeighborLoader walks the events of a timestamped edge type in time order and hands every event the history of
its end points BEFORE the event (glx_sample_temporal_hops: one cutoff per request row), for temporal models such as
TGN / TGAT:

    loader = gl.TemporalNeighborLoader(g, "interaction", "interaction", [10], batch_size=200, negatives=1)
    for batch in loader:                 # events in ascending (t, edge id) order; never shuffled
        batch.src, batch.dst, batch.t, batch.eid, batch.neg_dst
        blk = batch.block("src", 0)      # role "src" | "dst" | "neg", hop 0
        blk.nbr, blk.eid, blk.ts         # [rows, fanout] int64: neighbours over edges with ts < the row's cutoff
        blk.cnt, blk.rel_t, blk.edge_x   # valid slots per row, cutoff - ts, the sampled edges' float attributes
        rows, eid, ts, counts = batch.ragged("src", 0)   # the valid slots only: what dot_attention(counts=) takes
"""
import numpy as np

__all__ = ["NeighborLoader", "NeighborBatch", "CompactBatch", "TemporalNeighborLoader", "TemporalBatch", "TemporalBlock"]


_COLUMN_NAMES = ("labels", "weights", "timestamps", "int_attrs")


def _shaped(cols, shape):
  """a glx.Columns.lookup answer over flattened ids, back in the ids' shape (int_attrs keep their trailing axis)"""
  return {name: v.reshape(tuple(shape) + tuple(v.shape[1:])) for name, v in cols.items()}  # i_num may be 0: no -1


class NeighborBatch(object):
  """Tensors of one mini-batch (all on the GPU)."""

  def __init__(self, seeds, nbr, eid, x):
    self.seeds, self.nbr, self.eid, self.x = seeds, nbr, eid, x
    # filled when the loader was asked for them (node_columns / edge_columns / edge_features)
    self.node_cols = self.edge_cols = self.edge_x = self.y = None

  @property
  def num_hops(self):
    return len(self.nbr)

  def frontier(self, h):
    """ids of frontier h: the seeds (h = 0) or hop h's sampled neighbours, flattened"""
    return self.seeds if h == 0 else self.nbr[h - 1].reshape(-1)

  def edge_index(self, h):
    """(src, dst): position of each hop-(h+1) edge's source in frontier h and of its
    destination in frontier h+1 -- the dense fan-out layout makes both closed-form."""
    import torch
    rows, k = self.nbr[h].shape
    dst = torch.arange(rows * k, device=self.nbr[h].device)
    return torch.div(dst, k, rounding_mode="floor"), dst


class CompactBatch(NeighborBatch):
  """A mini-batch over its distinct nodes (NeighborLoader(..., dedup=True)).  seeds / nbr / eid are those of the plain
  batch.  The node set is kept per node type: frontiers of one type share a set, in hop order, so with distinct seeds
  nodes[:B] == seeds and nodes[:num_nodes_upto[h]] holds exactly the nodes of frontiers 0 .. h of that type.

    nodes            [M] int64 distinct ids -- a dict keyed by node type when the meta-path visits several types
    local[h]         positions of frontier h in the node set of its type, shaped like the frontier
    num_nodes_upto   [hops + 1] int64 CUDA tensor: size of frontier h's node set once frontier h is in
    x_nodes          [M, D] float attributes of nodes (dict keyed by type like nodes; None without float attributes)
    types[h]         node type of frontier h
  Building one costs a host read of the node set's size per node type (glx.unique), i.e. a wait for the stream.
  """

  def __init__(self, seeds, nbr, eid, types, nodes, local, num_nodes_upto, x_nodes):
    super(CompactBatch, self).__init__(seeds, nbr, eid, None)
    self.types, self.nodes, self.local = types, nodes, local
    self.num_nodes_upto, self.x_nodes = num_nodes_upto, x_nodes
    self.node_cols_nodes = None  # {name: one row per distinct node} (a dict per type like nodes) with node_columns

  def nodes_of(self, h):
    """the node set frontier h is numbered in"""
    return self.nodes[self.types[h]] if isinstance(self.nodes, dict) else self.nodes

  def edge_index(self, h):
    """(src, dst) of hop h+1 in node-set positions: local[h] repeated over the fan-out, local[h+1]."""
    k = self.nbr[h].shape[1]
    return self.local[h].reshape(-1).repeat_interleave(k), self.local[h + 1].reshape(-1)


class NeighborLoader(object):

  def __init__(self, graph, node_type, meta_path, fanouts, batch_size, strategy="random", shuffle=True,
               drop_last=False, with_features=True, seed_ids=None, dedup=False, node_columns=(), edge_columns=(),
               edge_features=False):
    import torch
    from graphlearn import settings
    for name in tuple(node_columns) + tuple(edge_columns):
      if name not in _COLUMN_NAMES:
        raise ValueError("unknown column {!r}: one of {}".format(name, _COLUMN_NAMES))
    self._graph = graph
    self._sampler = graph.neighbor_sampler(meta_path, fanouts, strategy=strategy)
    self._hops = len(fanouts)
    self._batch_size = int(batch_size)
    self._shuffle = shuffle
    self._drop_last = drop_last
    self._device = torch.device("cuda", settings._MIRROR.get("device_id", 0))  # pylint: disable=protected-access
    ids = graph.get_server().node_ids(node_type) if seed_ids is None else np.asarray(seed_ids, np.int64)
    self._ids = torch.from_numpy(np.ascontiguousarray(ids)).to(self._device)
    self._epoch = 0
    topo = graph.get_topology()
    types = [node_type] + [topo.get_dst_type(e) for e in (meta_path if isinstance(meta_path, (list, tuple)) else [meta_path])]
    self._types = types
    self._dedup = bool(dedup)
    self._feats = None
    if with_features:
      self._feats = []
      for t in types:
        try:
          self._feats.append(graph.device_features(t))
        except ValueError:
          self._feats.append(None)  # a type without float attributes
    edge_types = list(meta_path) if isinstance(meta_path, (list, tuple)) else [meta_path]
    self._node_columns, self._edge_columns = tuple(node_columns), tuple(edge_columns)
    self._ncols = [graph.device_columns(t) for t in types] if self._node_columns else None
    self._ecols = [graph.device_edge_columns(e) for e in edge_types] if self._edge_columns else None
    self._efeats = None
    if edge_features:
      self._efeats = []
      for e in edge_types:
        try:
          self._efeats.append(graph.device_edge_features(e))
        except ValueError:
          self._efeats.append(None)  # an edge type without float attributes

  def __len__(self):
    n = self._ids.shape[0]
    return n // self._batch_size if self._drop_last else (n + self._batch_size - 1) // self._batch_size

  def __iter__(self):
    import torch
    from graphlearn import settings
    n = self._ids.shape[0]
    order = self._ids
    if self._shuffle:
      gen = torch.Generator(device=self._device)
      gen.manual_seed(int(settings._MIRROR["sampling_seed"]) * 1000003 + self._epoch)  # pylint: disable=protected-access
      order = self._ids[torch.randperm(n, generator=gen, device=self._device)]
    batches = len(self)
    default_attr = float(settings._MIRROR.get("default_float_attr", 0.0))  # pylint: disable=protected-access
    for i in range(batches):
      seeds = order[i * self._batch_size:(i + 1) * self._batch_size].contiguous()
      cc = (self._epoch * batches + i) * self._hops
      hops = self._sampler.get_device(seeds, call_counter=cc)
      nbr = [h[0] for h in hops]
      eid = [h[1] for h in hops]
      if self._dedup:
        yield self._with_edge_data(self._compact(seeds, nbr, eid, default_attr), default_attr)
        continue
      x = None
      if self._feats is not None:
        x = []
        for h, f in enumerate(self._feats):
          ids = seeds if h == 0 else nbr[h - 1].reshape(-1)
          x.append(f.lookup(ids, default_attr) if f is not None else None)
      batch = NeighborBatch(seeds, nbr, eid, x)
      if self._ncols is not None:
        defaults = settings.column_defaults()
        batch.node_cols = []
        for h, c in enumerate(self._ncols):
          ids = seeds if h == 0 else nbr[h - 1]
          batch.node_cols.append(_shaped(c.lookup(ids.reshape(-1), self._node_columns, defaults), ids.shape))
        batch.y = batch.node_cols[0].get("labels")
      yield self._with_edge_data(batch, default_attr)
    self._epoch += 1

  def _with_edge_data(self, batch, default_attr):
    """edge_cols / edge_x of every hop, gathered by the hop's edge ids (the -1 of a default-filled row is unknown)."""
    from graphlearn import settings
    if self._ecols is not None:
      defaults = settings.column_defaults()
      batch.edge_cols = [_shaped(c.lookup(e.reshape(-1), self._edge_columns, defaults), e.shape)
                         for c, e in zip(self._ecols, batch.eid)]
    if self._efeats is not None:
      batch.edge_x = [f.lookup(e.reshape(-1), default_attr).reshape(tuple(e.shape) + (-1,)) if f is not None else None
                      for f, e in zip(self._efeats, batch.eid)]
    return batch

  def _compact(self, seeds, nbr, eid, default_attr):
    """One glx_unique over the frontiers of every node type (seeds, hop 1, ... in hop order), then one glx_lookup of
    the distinct nodes per type.  glx.unique reads the set's size on the host: one stream wait per node type."""
    import glx
    import torch
    frontiers = [seeds] + nbr
    kinds = list(dict.fromkeys(self._types))  # node types in order of first visit
    nodes, x_nodes, cols_nodes = {}, {}, {}
    local = [None] * len(frontiers)
    upto = torch.empty(len(frontiers), dtype=torch.int64, device=seeds.device)
    for t in kinds:
      hs = [h for h, th in enumerate(self._types) if th == t]
      nodes[t], inverse, part_end = glx.unique([frontiers[h] for h in hs])
      for h, inv in zip(hs, inverse):
        local[h] = inv
      for j, h in enumerate(hs):
        upto[h] = part_end[j]
      if self._feats is not None:
        f = self._feats[hs[0]]
        x_nodes[t] = f.lookup(nodes[t], default_attr) if f is not None else None
      if self._ncols is not None:  # one glx_columns_lookup per type, beside the one glx_lookup
        from graphlearn import settings
        cols_nodes[t] = self._ncols[hs[0]].lookup(nodes[t], self._node_columns, settings.column_defaults())
    if self._feats is None:
      x_nodes = None
    y = None
    if self._ncols is not None and "labels" in self._node_columns:
      y = cols_nodes[self._types[0]]["labels"][local[0]]
    if len(kinds) == 1:
      nodes = nodes[kinds[0]]
      x_nodes = x_nodes[kinds[0]] if x_nodes is not None else None
      cols_nodes = cols_nodes.get(kinds[0])
    batch = CompactBatch(seeds, nbr, eid, list(self._types), nodes, local, upto, x_nodes)
    if self._ncols is not None:
      batch.node_cols_nodes, batch.y = cols_nodes, y
    return batch


_ROLES = ("src", "dst", "neg")


class TemporalBlock(object):
  """One hop of one role of a TemporalBatch.  Request row r is the role's seed r (hop 0) or slot r of the previous hop.

    nbr, eid, ts   [rows, fanout] int64: the sampled neighbours, their edge ids and edge timestamps; a slot that holds no
                   edge is (default neighbour id, -1, default timestamp)
    cnt            [rows] int32: valid slots of the row -- the first cnt ("recent"), or all / none ("uniform")
    cutoff         [rows] int64: the time the row's history ends at (strictly before it unless inclusive)
    rel_t          [rows, fanout] int64: cutoff - ts, 0 where the slot holds no edge
    edge_x         [rows, fanout, D] float attributes of the sampled edges (None unless asked for / the type has none)
    edge_cols      {name: [rows, fanout (, i_num)]} columns of the sampled edges (None unless asked for)
  """

  def __init__(self, nbr, eid, ts, cnt, cutoff):
    import torch
    self.nbr, self.eid, self.ts, self.cnt, self.cutoff = nbr, eid, ts, cnt, cutoff
    self.valid = torch.arange(nbr.shape[1], device=nbr.device)[None, :] < cnt[:, None]
    self.rel_t = torch.where(self.valid, cutoff[:, None] - ts, torch.zeros_like(ts))
    self.edge_x = self.edge_cols = None


class TemporalBatch(object):
  """Tensors of one batch of events (all on the GPU): src, dst, t, eid [B]; neg_dst [B, negatives]; per role in
  ("src", "dst", "neg") a list over hops of TemporalBlock (blocks[role]; "neg" is empty without negatives).  The "neg"
  role's seeds are neg_dst flattened, each with its event's time."""

  def __init__(self, src, dst, t, eid, neg_dst, blocks):
    self.src, self.dst, self.t, self.eid, self.neg_dst, self.blocks = src, dst, t, eid, neg_dst, blocks

  def block(self, role, h):
    return self.blocks[role][h]

  def seeds(self, role):
    """ids the role's hop 0 was sampled for"""
    return {"src": self.src, "dst": self.dst, "neg": self.neg_dst.reshape(-1)}[role]

  def ragged(self, role, h, with_positions=False):
    """(rows, eid, ts, counts): the block's valid slots only, row after row -- the counts= layout of dot_attention and
    TransformerConv (rows = neighbour ids, counts = cnt).  One boolean-mask compaction: the number of valid slots decides
    the shapes, so this waits for the stream ONCE (the dense blocks never do).  with_positions=True appends the valid
    slots' flat positions in the dense block (to gather edge_x / rel_t the same way)."""
    blk = self.blocks[role][h]
    at = blk.valid.reshape(-1).nonzero().reshape(-1)  # the host sync
    out = (blk.nbr.reshape(-1)[at], blk.eid.reshape(-1)[at], blk.ts.reshape(-1)[at], blk.cnt)
    return out + (at,) if with_positions else out


class TemporalNeighborLoader(object):
  """Batches of timestamped events with the temporal neighbourhoods of their end points.

    graph       an initialised gl.Graph
    events      an edge type name -- its edges are the events: end points from the store, timestamps from the type's
                device columns, read once here -- or (src, dst, t[, eid]) arrays.  Iteration is in ascending (t, edge id)
                order (one stable sort on the device); temporal training is not shuffled.
    history     the timestamped edge type whose past is sampled.  Roles "src" sample its out-edges; roles "dst" / "neg"
                sample history + "_reverse" (a heterogeneous type declared directed=False) or the type itself (a
                homogeneous one); further hops alternate between the two.
    fanouts     neighbours per hop
    strategy    "recent" (the latest first) | "uniform" (with replacement)
    inclusive   cutoffs are strict by default: an event never sees itself or its same-timestamp siblings
    negatives   neg_dst[B, negatives] from the "random" negative sampler of `history` (what
                graph.negative_sampler(history, negatives, "random") draws under call counter epoch * len(loader) + batch)
  Batch i of epoch e samples role number r under call counter ((e * len(loader) + i) * 3 + r) * hops, so a (sampling
  seed, epoch, batch) triple reproduces its batch bit for bit.  Not served here: dedup=True, the distributed store,
  graph capture."""

  def __init__(self, graph, events, history, fanouts, batch_size, strategy="recent", inclusive=False, negatives=0,
               edge_features=True, edge_columns=(), drop_last=False):
    import glx
    import torch
    from graphlearn import settings
    for name in tuple(edge_columns):
      if name not in _COLUMN_NAMES:
        raise ValueError("unknown column {!r}: one of {}".format(name, _COLUMN_NAMES))
    if strategy not in glx.TEMPORAL_STRATEGIES:
      raise ValueError("unknown temporal strategy {!r}: one of {}".format(strategy, sorted(glx.TEMPORAL_STRATEGIES)))
    if getattr(graph, "_shard", (0, 1))[1] > 1:
      raise NotImplementedError("TemporalNeighborLoader does not serve the distributed store")
    self._graph = graph
    self._fanouts = [int(k) for k in fanouts]
    self._batch_size = int(batch_size)
    self._strategy, self._inclusive = strategy, bool(inclusive)
    self._negatives = int(negatives)
    self._drop_last = drop_last
    self._device = torch.device("cuda", settings._MIRROR.get("device_id", 0))  # pylint: disable=protected-access
    self._epoch = 0
    # the two directions of the history
    topo = graph.get_topology()
    graph.get_edge_decoder(history)
    if topo.get_src_type(history) == topo.get_dst_type(history):
      twin = history
    else:
      twin = history + "_reverse"
      if twin not in graph.get_edge_decoders():
        raise ValueError("destination-side roles sample the in-edges of {!r}: edge type {!r} is missing (declare the "
                         "type with directed=False)".format(history, twin))
    out_types = [history if h % 2 == 0 else twin for h in range(len(self._fanouts))]
    in_types = [twin if h % 2 == 0 else history for h in range(len(self._fanouts))]
    self._types = {"src": out_types, "dst": in_types, "neg": in_types}
    self._graphs = {}
    for e in set(out_types + in_types):
      self._graphs[e] = graph.device_graph(e)
      if not self._graphs[e].has_timestamps:
        raise ValueError("edge type {!r} keeps no timestamps (Decoder(timestamped=True))".format(e))
    self._efeats, self._ecols = {}, {}
    for e in self._graphs:
      if edge_features:
        try:
          self._efeats[e] = graph.device_edge_features(e)
        except ValueError:
          self._efeats[e] = None  # an edge type without float attributes
      if edge_columns:
        self._ecols[e] = graph.device_edge_columns(e)
    self._edge_columns = tuple(edge_columns)
    self._negative = glx.Negative.from_graph(self._graphs[history]) if self._negatives > 0 else None
    # the events, in (t, edge id) order
    if isinstance(events, str):
      server = graph.get_server()
      src, dst = np.asarray(server.edge_src_ids(events), np.int64), np.asarray(server.edge_dst_ids(events), np.int64)
      eid = torch.arange(src.shape[0], dtype=torch.int64, device=self._device)
      t = graph.device_edge_columns(events).lookup(eid, ("timestamps",), settings.column_defaults())["timestamps"]
    else:
      src, dst, t = (np.ascontiguousarray(np.asarray(a, np.int64)) for a in events[:3])
      t = torch.from_numpy(t).to(self._device)
      eid = (torch.from_numpy(np.ascontiguousarray(np.asarray(events[3], np.int64))).to(self._device)
             if len(events) > 3 else torch.arange(src.shape[0], dtype=torch.int64, device=self._device))
    src, dst = (torch.from_numpy(np.ascontiguousarray(a)).to(self._device) for a in (src, dst))
    by_eid = torch.sort(eid, stable=True)[1]
    order = by_eid[torch.sort(t[by_eid], stable=True)[1]]
    self._src, self._dst, self._t, self._eid = (a[order].contiguous() for a in (src, dst, t.to(torch.int64), eid))

  def __len__(self):
    n = self._src.shape[0]
    return n // self._batch_size if self._drop_last else (n + self._batch_size - 1) // self._batch_size

  def __iter__(self):
    import glx
    from graphlearn import settings
    flags = settings._MIRROR  # pylint: disable=protected-access
    batches, hops = len(self), len(self._fanouts)
    for i in range(batches):
      lo, hi = i * self._batch_size, (i + 1) * self._batch_size
      src, dst, t, eid = (a[lo:hi] for a in (self._src, self._dst, self._t, self._eid))
      step = self._epoch * batches + i
      neg_dst = src.new_empty((src.shape[0], 0))
      if self._negative is not None:
        neg_dst = self._negative.sample(src, self._negatives, default_neighbor_id=flags["default_neighbor_id"],
                                        seed=flags["sampling_seed"], call_counter=step)
      seeds = {"src": (src, t), "dst": (dst, t), "neg": (neg_dst.reshape(-1), t.repeat_interleave(self._negatives))}
      blocks = {}
      for r, role in enumerate(_ROLES):
        blocks[role] = []
        if role == "neg" and self._negative is None:
          continue
        ids, cutoff = seeds[role]
        out = glx.sample_temporal_hops([self._graphs[e] for e in self._types[role]], ids, cutoff, self._fanouts,
                                       strategy=self._strategy, inclusive=self._inclusive, seed=flags["sampling_seed"],
                                       call_counter=(step * len(_ROLES) + r) * hops,
                                       default_neighbor_id=flags["default_neighbor_id"],
                                       default_timestamp=flags["default_timestamp"])
        for h, (nbr, e, ts, cnt) in enumerate(out):
          blk = TemporalBlock(nbr, e, ts, cnt, cutoff)
          self._with_edge_data(blk, self._types[role][h])
          blocks[role].append(blk)
          cutoff = ts.reshape(-1)
      yield TemporalBatch(src, dst, t, eid, neg_dst, blocks)
    self._epoch += 1

  def _with_edge_data(self, blk, edge_type):
    """edge_x / edge_cols of a block, gathered by its edge ids as NeighborLoader._with_edge_data does (the -1 of a slot
    that holds no edge is unknown: the defaults)"""
    from graphlearn import settings
    f = self._efeats.get(edge_type)
    if f is not None:
      default_attr = float(settings._MIRROR.get("default_float_attr", 0.0))  # pylint: disable=protected-access
      blk.edge_x = f.lookup(blk.eid.reshape(-1), default_attr).reshape(tuple(blk.eid.shape) + (-1,))
    c = self._ecols.get(edge_type)
    if c is not None:
      blk.edge_cols = _shaped(c.lookup(blk.eid.reshape(-1), self._edge_columns, settings.column_defaults()), blk.eid.shape)
