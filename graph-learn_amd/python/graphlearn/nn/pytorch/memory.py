"""The memory module of TGN with its message store in HBM: the torch surface of glx_tgn_store_update, glx_tgn_message,
glx_tgn_message_backward and glx_tgn_memory_write (include/glx.h).

The role of torch_geometric.nn.TGNMemory with IdentityMessage and LastAggregator in the reference's TGN example
(graphlearn/examples/pytorch/tgn/train_and_eval.py:27-31, :70-78, used at :118 and :130):

    memory = TGNMemory(num_nodes, raw_msg_dim=172, memory_dim=100, time_dim=100).cuda()
    gnn = GraphAttentionEmbedding(100, 100, 172, memory.time_enc)      # shares the time encoder, as in the reference
    z, last_update = memory(n_id)                                      # gru(message, memory[n_id]) with a gradient
    ...loss...
    memory.update_state(src, dst, t, raw_msg)                          # before loss.backward(), as in the reference
    loss.backward(); opt.step(); memory.detach()

torch_geometric keeps the messages in two Python dicts keyed by node id and walks them with n_id.tolist() on every
forward and every update_state.  With the Last aggregator and a message function without parameters the only stored
message of a node that is ever used is its latest event over both roles, so the store here is ONE pending slot per node,
in six persistent buffers (state_dict() carries the store):

    memory [N, M] float32, last_update [N] int64, pend_t [N] int64 (the event's time), pend_seq [N] int64 (its sequence
    number, -1: none), pend_other [N] int64 (its other end point), pend_raw [N, R] float32 (its raw message)

The slot of node v holds the event with the largest (t, seq) that ever named v as src or dst, seq counting the events
passed to update_state since the last reset_state(): on a time-ordered stream that is TGNMemory + LastAggregator with the
tie between two events of one timestamp decided (the later position wins), so two runs give the same bits.  On a stream
that is not time-ordered the rule is still total and then differs from torch_geometric, which lets a later call overwrite
a role's list whatever its timestamps are.  No call reads anything back on the host; the number of events seen is a
Python int carried by get_extra_state() / set_extra_state().

Limits: Last aggregator and identity message only; float32 memory and int64 ids and times; one GPU (not the
distributed store); no graph capture; a gradient reaches the GRU's and the time encoder's parameters only (the memory
and the raw messages are buffers: constants, as after the reference's detach()); N * (4 M + 4 R + 32) bytes of state.
"""
import torch

from graphlearn.nn.pytorch.segment import _glx, _no_double_backward

__all__ = ["TGNMemory", "TimeEncoder"]

_INT64_MIN = -2 ** 63
_INT32_MAX = 2 ** 31 - 1


class TimeEncoder(torch.nn.Module):
  """cos(rel_t[:, None] * weight + bias): torch_geometric's TimeEncoder (a Linear(1, out_channels) under a cosine) with
  its weight as a vector, so that the kernels and the reference's GraphAttentionEmbedding share one set of parameters."""

  def __init__(self, out_channels):
    super().__init__()
    self.out_channels = int(out_channels)
    self.weight = torch.nn.Parameter(torch.empty(self.out_channels))
    self.bias = torch.nn.Parameter(torch.empty(self.out_channels))
    self.reset_parameters()

  def reset_parameters(self):
    # Linear(1, T)'s own initial values: fan_in = 1 makes both uniform on [-1, 1)
    torch.nn.init.uniform_(self.weight, -1.0, 1.0)
    torch.nn.init.uniform_(self.bias, -1.0, 1.0)

  def forward(self, rel_t):
    return torch.cos(rel_t[:, None] * self.weight + self.bias)


class _Message(torch.autograd.Function):
  """(msg, h, t) of glx_tgn_message; the gradient of msg goes to the time encoder's weight and bias alone."""

  @staticmethod
  def forward(ctx, weight, bias, module, n_id):
    glx = _glx()
    msg, h, dt, t, has = glx.tgn_message(module.memory, module.last_update, module.pend_t, module.pend_seq,
                                          module.pend_other, module.pend_raw, weight.detach(), bias.detach(), n_id)
    ctx.time_off = 2 * module.memory_dim + module.raw_msg_dim
    ctx.save_for_backward(weight, bias, dt, has)
    ctx.mark_non_differentiable(h, t)
    return msg, h, t

  @staticmethod
  def backward(ctx, grad_msg, _grad_h, _grad_t):
    _no_double_backward("TGNMemory")
    need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    if not (need_w or need_b):
      return None, None, None, None
    weight, bias, dt, has = ctx.saved_tensors
    grad_w, grad_b = _glx().tgn_message_backward(grad_msg.to(torch.float32).contiguous(), dt, has, weight.detach(),
                                                 bias.detach(), ctx.time_off)
    return (grad_w if need_w else None), (grad_b if need_b else None), None, None


class TGNMemory(torch.nn.Module):
  """TGNMemory(num_nodes, raw_msg_dim, memory_dim, time_dim) with torch_geometric's methods: forward(n_id),
  update_state(src, dst, t, raw_msg), reset_state(), detach().  Move it to the GPU before use (.cuda())."""

  def __init__(self, num_nodes, raw_msg_dim, memory_dim, time_dim):
    super().__init__()
    num_nodes, raw_msg_dim, memory_dim, time_dim = int(num_nodes), int(raw_msg_dim), int(memory_dim), int(time_dim)
    if num_nodes < 0 or num_nodes >= _INT32_MAX:
      raise ValueError("TGNMemory: num_nodes must be in [0, 2^31 - 1), not {}".format(num_nodes))
    if raw_msg_dim < 0 or memory_dim < 1 or time_dim < 1:
      raise ValueError("TGNMemory: raw_msg_dim >= 0, memory_dim >= 1 and time_dim >= 1 are required")
    self.num_nodes, self.raw_msg_dim, self.memory_dim, self.time_dim = num_nodes, raw_msg_dim, memory_dim, time_dim
    self.time_enc = TimeEncoder(time_dim)
    self.gru = torch.nn.GRUCell(2 * memory_dim + raw_msg_dim + time_dim, memory_dim)
    self.register_buffer("memory", torch.empty(num_nodes, memory_dim))
    self.register_buffer("last_update", torch.empty(num_nodes, dtype=torch.int64))
    self.register_buffer("pend_t", torch.empty(num_nodes, dtype=torch.int64))
    self.register_buffer("pend_seq", torch.empty(num_nodes, dtype=torch.int64))
    self.register_buffer("pend_other", torch.empty(num_nodes, dtype=torch.int64))
    self.register_buffer("pend_raw", torch.empty(num_nodes, raw_msg_dim))
    self.seq_base = 0  # events passed to update_state since the last reset: a Python int, never a device read
    self.reset_state()

  def reset_parameters(self):
    self.time_enc.reset_parameters()
    self.gru.reset_parameters()
    self.reset_state()

  def reset_state(self):
    """A fresh memory and an empty store."""
    with torch.no_grad():
      self.memory.zero_()
      self.last_update.zero_()
      self.pend_t.fill_(_INT64_MIN)
      self.pend_seq.fill_(-1)
      self.pend_other.fill_(-1)
      self.pend_raw.zero_()
    self.seq_base = 0

  def detach(self):
    """Detaches the memory from a gradient graph (it never carries one here: update_state writes it in place)."""
    self.memory.detach_()

  def get_extra_state(self):
    return {"seq_base": int(self.seq_base)}

  def set_extra_state(self, state):
    self.seq_base = int(state["seq_base"])

  def _check_ids(self, x, name):
    if not isinstance(x, torch.Tensor) or x.dtype != torch.int64 or x.dim() != 1:
      raise ValueError("TGNMemory: {} must be a one-dimensional int64 tensor".format(name))
    if x.device != self.memory.device or not x.is_cuda:
      raise ValueError("TGNMemory: {} must live on the module's GPU ({}), not {}".format(name, self.memory.device, x.device))
    return x.contiguous()

  def forward(self, n_id):
    """(memory [n, M], last_update [n]) of the nodes n_id.  In training mode the memory is gru(message, memory[n_id]) of
    the pending messages, with a gradient for the GRU and the time encoder -- a node without a message passes the GRU
    with a zero input -- and last_update the message's time; in eval mode both are the stored values.  An id outside the
    table counts as a node with a zero memory, no message and time 0 in either mode."""
    n_id = self._check_ids(n_id, "n_id")
    if self.training:
      msg, h, t = _Message.apply(self.time_enc.weight, self.time_enc.bias, self, n_id)
      return self.gru(msg, h), t
    # an id outside the table reads a zero row and time 0, as in the kernels (and never an out-of-range gather)
    inside = (n_id >= 0) & (n_id < self.num_nodes)
    if self.num_nodes == 0:
      return self.memory.new_zeros((n_id.numel(), self.memory_dim)), torch.zeros_like(n_id)
    rows = n_id.clamp(0, self.num_nodes - 1)
    memory = self.memory.index_select(0, rows)
    last_update = self.last_update.index_select(0, rows)
    return (torch.where(inside[:, None], memory, torch.zeros_like(memory)),
            torch.where(inside, last_update, torch.zeros_like(last_update)))

  def _write_memory(self, u):
    glx = _glx()
    with torch.no_grad():
      msg, h, _, t, _ = glx.tgn_message(self.memory, self.last_update, self.pend_t, self.pend_seq, self.pend_other,
                                        self.pend_raw, self.time_enc.weight.detach(), self.time_enc.bias.detach(), u)
      glx.tgn_memory_write(self.memory, self.last_update, u, self.gru(msg, h).contiguous(), t)

  def update_state(self, src, dst, t, raw_msg):
    """Takes the events (src[p], dst[p], t[p], raw_msg[p]) in: the memory of their end points moves on to
    gru(message, memory) of the messages pending for them, and the events become the pending messages of their end
    points -- in training mode the memory first (the events' own messages wait for the next call), in eval mode the
    store first, as in torch_geometric.  No host sync: the distinct end points are used at their padded length."""
    src, dst, t = self._check_ids(src, "src"), self._check_ids(dst, "dst"), self._check_ids(t, "t")
    B = int(src.shape[0])
    if int(dst.shape[0]) != B or int(t.shape[0]) != B:
      raise ValueError("TGNMemory: src, dst and t must have one entry per event")
    if (not isinstance(raw_msg, torch.Tensor) or raw_msg.dtype != torch.float32
        or tuple(raw_msg.shape) != (B, self.raw_msg_dim) or raw_msg.device != self.memory.device):
      raise ValueError("TGNMemory: raw_msg must be a float32 [{}, {}] tensor on the module's GPU".format(B, self.raw_msg_dim))
    if B == 0:
      return
    glx = _glx()
    raw_msg = raw_msg.detach().contiguous()
    u = glx.unique([src, dst], return_inverse=False, pad=-1)[0]  # [2B]: the distinct ids, then -1, which both kernels skip
    if self.training:
      self._write_memory(u)
    glx.tgn_store_update(src, dst, t, raw_msg, self.seq_base, self.pend_t, self.pend_seq, self.pend_other, self.pend_raw)
    if not self.training:
      self._write_memory(u)
    self.seq_base += B
