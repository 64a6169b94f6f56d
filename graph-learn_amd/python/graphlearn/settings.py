"""Process-wide engine flags (graphlearn/python/config.py; GLOBAL_FLAG in
graphlearn/src/include/config.h).  The thread-pool / RPC knobs of the reference's
service layer are accepted and ignored: there is no service layer between Python and
the GPU here.  `set_sampling_seed`, `set_device_id` and `set_feature_dtype` are new."""
from graphlearn import pywrap_graphlearn as pywrap

__all__ = [
    "set_default_neighbor_id", "set_padding_mode", "set_default_int_attribute",
    "set_default_float_attribute", "set_default_string_attribute", "set_default_weight",
    "set_default_label", "set_default_timestamp", "set_ignore_invalid", "set_sampler_retry_times",
    "set_default_full_nbr_num",
    "set_inter_threadnum", "set_intra_threadnum", "set_inner_threadnum", "set_datainit_batchsize",
    "set_inmemory_queuesize", "set_shuffle_buffer_size", "set_tracker_mode", "set_storage_mode",
    "set_retry_times", "set_timeout", "set_sampling_seed", "set_device_id", "set_feature_dtype",
]


# flags the device-tensor path (NeighborSampler.get_device) passes to the C-ABI itself
_MIRROR = {"padding_mode": 1, "default_neighbor_id": 0, "sampling_seed": 0, "default_float_attr": 0.0, "device_id": 0,
           "default_full_nbr_num": 100, "default_weight": 0.0, "feature_dtype": "float32", "default_int_attr": 0,
           "default_label": -1, "default_timestamp": -1}


def column_defaults():
  """What the device column lookups (glx.Columns.lookup) answer for an unknown id: the Default* flags as the host
  operators read them."""
  return {"weights": _MIRROR["default_weight"], "labels": _MIRROR["default_label"],
          "timestamps": _MIRROR["default_timestamp"], "int_attrs": _MIRROR["default_int_attr"]}

# storage types of the node feature tables (include/glx.h GLX_DTYPE_*)
_FEATURE_DTYPES = {"float32": 0, "bfloat16": 1, "float16": 2, "float8_e4m3fn": 8, "float8_e5m2": 9}


def set_default_neighbor_id(nbr_id):
  pywrap.set_default_neighbor_id(int(nbr_id))
  _MIRROR["default_neighbor_id"] = int(nbr_id)


def set_padding_mode(mode):
  """gl.REPLICATE or gl.CIRCULAR (the engine default, like the reference's)."""
  pywrap.set_padding_mode(int(mode))
  _MIRROR["padding_mode"] = int(mode)


def set_default_int_attribute(value=0):
  pywrap.set_default_int_attr(int(value))
  _MIRROR["default_int_attr"] = int(value)


def set_default_float_attribute(value=0.0):
  pywrap.set_default_float_attr(float(value))
  _MIRROR["default_float_attr"] = float(value)


def set_default_string_attribute(value=""):
  pywrap.set_default_string_attr(str(value))


def set_default_weight(value=0.0):
  pywrap.set_default_weight(float(value))
  _MIRROR["default_weight"] = float(value)


def set_default_full_nbr_num(num):
  """Neighbours a node2vec step looks at (GLOBAL_FLAG(DefaultFullNbrNum), 100)."""
  pywrap.set_default_full_nbr_num(int(num))
  _MIRROR["default_full_nbr_num"] = int(num)


def set_default_label(value=-1):
  pywrap.set_default_label(int(value))
  _MIRROR["default_label"] = int(value)


def set_default_timestamp(value=-1):
  pywrap.set_default_timestamp(int(value))
  _MIRROR["default_timestamp"] = int(value)


def set_ignore_invalid(value):
  pywrap.set_ignore_invalid(1 if value else 0)


def set_sampler_retry_times(value):
  pywrap.set_sampler_retry_times(int(value))


def set_shuffle_buffer_size(value):
  """How many consecutive ids a "shuffle" traversal (node_sampler / edge_sampler / g.V().shuffle(traverse=True)) shuffles at
  a time (GLOBAL_FLAG(ShuffleBufferSize), 10240: node_generator.h:168-190)."""
  pywrap.set_shuffle_buffer_size(int(value))


def set_sampling_seed(seed):
  """Seed of the counter-based random streams of the samplers;
  the reference's samplers cannot be seeded."""
  pywrap.set_sampling_seed(int(seed))
  _MIRROR["sampling_seed"] = int(seed)


def set_device_id(device):
  """GPU that holds this process' graph store (one process per GPU)."""
  pywrap.set_device_id(int(device))
  _MIRROR["device_id"] = int(device)


def set_feature_dtype(dtype):
  """Storage type of the node float attributes in HBM: "float32" (the default), "bfloat16", "float16",
  "float8_e4m3fn" or "float8_e5m2".  Half tables hold half the bytes, float8 tables a quarter; aggregation and lookup
  still accumulate and answer in float32 (each result equals the float32 one over the attributes rounded to `dtype`).
  float8_e4m3fn has no infinity: an attribute beyond +-464 is stored as NaN, so normalise such attributes first.
  Takes effect for the node types Graph.init() builds after it; the distributed store (sharded_store) takes float32
  tables only."""
  if dtype not in _FEATURE_DTYPES:
    raise ValueError("feature dtype must be one of {}, not {!r}".format(sorted(_FEATURE_DTYPES), dtype))
  pywrap.set_feature_dtype(_FEATURE_DTYPES[dtype])
  _MIRROR["feature_dtype"] = dtype


def _ignored(name):
  def setter(value=0):
    getattr(pywrap, name)(int(value))
  setter.__name__ = name
  setter.__doc__ = "Accepted for source compatibility; has no effect on the device engine."
  return setter


for _n in ("set_inter_threadnum", "set_intra_threadnum", "set_inner_threadnum", "set_datainit_batchsize",
           "set_inmemory_queuesize", "set_tracker_mode", "set_storage_mode",
           "set_retry_times", "set_timeout"):
  globals()[_n] = _ignored(_n)
