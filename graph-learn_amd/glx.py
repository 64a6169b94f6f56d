"""ctypes harness over the glx C-ABI (include/glx.h) for tests and bench.py.

This is plumbing, not the product: the product is libglx.so (HIP kernels behind
the C-ABI) and libglx_host.so (the C++ mirror of graphlearn::op).  numpy arrays
are passed as host pointers (GLX_PTR_HOST), torch CUDA tensors as device
pointers (GLX_PTR_DEVICE) on the current torch stream.  There is no CPU
fallback anywhere: a missing library or a missing GPU raises.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GLX_LIB") or os.path.join(_HERE, "lib", "libglx.so")  # GLX_LIB: A/B builds

PTR_HOST, PTR_DEVICE = 0, 1
RANDOM, RANDOM_WITHOUT_REPLACEMENT, EDGE_WEIGHT, TOPK, IN_DEGREE = 0, 1, 2, 3, 4
SUM, MEAN, MAX, MIN, PROD = 0, 1, 2, 3, 4
PAD_REPLICATE, PAD_CIRCULAR = 0, 1

# registry names of the reference (REGISTER_OPERATOR(...)) -> ids of the C-ABI
SAMPLER_IDS = {
    "RandomSampler": RANDOM,
    "RandomWithoutReplacementSampler": RANDOM_WITHOUT_REPLACEMENT,
    "EdgeWeightSampler": EDGE_WEIGHT,
    "TopkSampler": TOPK,
}
# further registry names served on the device
EXTRA_SAMPLER_IDS = {"InDegreeSampler": IN_DEGREE}
AGGREGATOR_IDS = {
    "SumAggregator": SUM,
    "MeanAggregator": MEAN,
    "MaxAggregator": MAX,
    "MinAggregator": MIN,
    "ProdAggregator": PROD,
}

EXPORTS = [
    "glx_abi_version", "glx_device_count", "glx_last_error", "glx_host_register", "glx_host_unregister",
    "glx_graph_create", "glx_graph_build", "glx_graph_build_ordered", "glx_graph_destroy", "glx_graph_info", "glx_graph_export_alias",
    "glx_graph_edge_weight_packed", "glx_graph_edge_weight_record_bytes", "glx_graph_row_dir",
    "glx_graph_degrees", "glx_graph_in_degrees", "glx_sample", "glx_sample_ex", "glx_sample_hops",
    "glx_graph_enable_in_degree", "glx_graph_enable_default_weight", "glx_sample_full_sizes", "glx_sample_full",
    "glx_graph_set_timestamps", "glx_sample_filtered", "glx_sample_full_filtered", "glx_random_walk",
    "glx_graph_has_timestamps", "glx_sample_temporal", "glx_sample_temporal_hops",
    "glx_features_create", "glx_features_view", "glx_features_destroy", "glx_features_info",
    "glx_features_create_ex", "glx_features_view_ex", "glx_features_dtype", "glx_features_convert_host",
    "glx_knn_search", "glx_knn_merge",
    "glx_knn_ivf_build", "glx_knn_ivf_search", "glx_knn_ivf_info", "glx_knn_ivf_export", "glx_knn_ivf_destroy",
    "glx_knn_ivfpq_build", "glx_knn_ivfpq_search", "glx_knn_ivfpq_info", "glx_knn_ivfpq_export",
    "glx_knn_ivfpq_destroy",
    "glx_aggregate", "glx_lookup", "glx_aggregate_arg", "glx_aggregate_backward",
    "glx_aggregate_weighted", "glx_aggregate_weighted_backward_x", "glx_aggregate_weighted_backward_w",
    "glx_segment_softmax", "glx_segment_softmax_backward",
    "glx_gat_attention", "glx_gat_attention_backward",
    "glx_dot_attention", "glx_dot_attention_backward",
    "glx_pair_dot", "glx_pair_dot_backward",
    "glx_aggregate_backward_ex", "glx_aggregate_weighted_ex", "glx_aggregate_weighted_backward_x_ex",
    "glx_aggregate_weighted_backward_w_ex", "glx_pair_dot_ex", "glx_pair_dot_backward_ex",
    "glx_aggregate_backward_chunked", "glx_aggregate_weighted_backward_x_chunked",
    "glx_dot_attention_chunked", "glx_dot_attention_backward_chunked",
    "glx_rows_coalesce", "glx_embedding_update",
    "glx_tgn_store_update", "glx_tgn_message", "glx_tgn_message_backward", "glx_tgn_memory_write",
    "glx_partition", "glx_stitch_i64", "glx_stitch_f32", "glx_aggregate_stitch",
    "glx_negative_create", "glx_negative_from_graph", "glx_negative_destroy", "glx_negative_info",
    "glx_negative_export", "glx_graph_enable_negative", "glx_negative_sample",
    "glx_profile_enable", "glx_profile_collect",
    "glx_comm_unique_id", "glx_comm_init_rccl", "glx_comm_init_local", "glx_comm_init_callbacks", "glx_comm_destroy",
    "glx_comm_info", "glx_comm_set_max_message_bytes", "glx_exchange_v", "glx_comm_allgather_i64", "glx_comm_barrier",
    "glx_dist_store_create", "glx_dist_store_destroy", "glx_dist_store_set_cache", "glx_dist_store_set_graph_replica",
    "glx_dist_build_graph_replica", "glx_dist_sample_full_sizes", "glx_dist_sample_full", "glx_dist_sample_full_filtered",
    "glx_dist_in_degrees", "glx_dist_negative_create", "glx_dist_negative_sample", "glx_dist_random_walk", "glx_dist_random_walk_ex",
    "glx_dist_last_sample_rows", "glx_dist_hot_ids",
    "glx_dist_enable_in_degree",
    "glx_dist_sample", "glx_dist_aggregate", "glx_dist_aggregate_partial", "glx_dist_aggregate_begin", "glx_dist_aggregate_end", "glx_dist_aggregate_end_range", "glx_dist_lookup",
    "glx_dist_last_stats",
    "glx_dist_ledger_create", "glx_dist_ledger_destroy", "glx_dist_store_set_ledger", "glx_dist_confirm",
    "glx_dist_ledger_get_stats", "glx_dist_ledger_set_slack",
    "glx_plan_create", "glx_plan_run", "glx_plan_output", "glx_plan_destroy",
    "glx_probe_bandwidth", "glx_tune", "glx_subgraph_induce",
    "glx_cond_table_create", "glx_cond_table_destroy", "glx_cond_negative_sample",
    "glx_unique",
    "glx_columns_create", "glx_columns_destroy", "glx_columns_info", "glx_columns_lookup",
]


FILTER_NONE, FILTER_EQUAL, FILTER_LARGER_THAN = 0, 1, 2
TEMPORAL_RECENT, TEMPORAL_UNIFORM = 0, 1
TEMPORAL_STRATEGIES = {"recent": TEMPORAL_RECENT, "uniform": TEMPORAL_UNIFORM}
FILTER_FIELD_NONE, FILTER_FIELD_ID, FILTER_FIELD_TIMESTAMP = 0, 1, 2


class Filter(ctypes.Structure):
    """glx_filter (include/glx.h): type, field, values[batch], retry_times, default_timestamp."""
    _fields_ = [("type", ctypes.c_int32), ("field", ctypes.c_int32), ("values", ctypes.c_void_p),
                ("retry_times", ctypes.c_int32), ("default_timestamp", ctypes.c_int64)]


class DistStats(ctypes.Structure):
    """glx_dist_stats (include/glx.h): where the ids of a store's last aggregate / lookup came from."""
    _fields_ = [(n, ctypes.c_int64) for n in ("ids", "from_replica", "from_own_shard", "remote", "remote_distinct",
                                                "served_rows", "bytes_sent", "bytes_received", "exchange_rounds",
                                                "host_syncs", "host_stall_us")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


# int (*)(void* user, const void* send, const int64_t* send_counts, void* recv, const int64_t* recv_counts, int64_t eb)
HOST_ALLTOALLV_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_int64)
# int (*)(void* user, const void* send, void* recv, int64_t bytes_per_rank)
HOST_ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)


ABORTED = 10  # GLX_ABORTED: a speculated exchange did not fit (Ledger); repeat the unconfirmed calls


class GlxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("glx error %d: %s" % (code, msg))
        self.code = code


_lib = None


def lib():
    """Loads libglx.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GlxError(14, "libglx.so not built: run `python -c 'import __graft_entry__ as g; g.build()'`"
                               " (expected at %s)" % LIB_PATH)
        # torch bundles its own HIP runtime (torch/lib/libamdhip64.so, SONAME
        # libamdhip64.so.7).  It must be in the process BEFORE libglx.so so that
        # libglx's NEEDED libamdhip64.so.7 binds to the same runtime; two HIP
        # runtimes in one process cannot share device pointers.
        if not os.environ.get("GLX_NO_TORCH"):  # (debug knob: run on the system HIP runtime)
            import torch  # noqa: F401
        L = ctypes.CDLL(LIB_PATH)
        vp, i32, i64, u64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float
        ci = ctypes.c_int
        L.glx_last_error.restype = ctypes.c_char_p
        L.glx_device_count.argtypes = [ctypes.POINTER(ci)]
        L.glx_host_register.argtypes = [vp, u64]
        L.glx_host_unregister.argtypes = [vp]
        L.glx_graph_create.argtypes = [ci, i64, i64, vp, vp, vp, vp, vp, ci, vp, ctypes.POINTER(vp)]
        L.glx_graph_build.argtypes = [ci, i64, vp, vp, vp, vp, ci, ci, vp, ctypes.POINTER(vp)]
        L.glx_graph_destroy.argtypes = [vp]
        L.glx_graph_destroy.restype = None
        L.glx_graph_info.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(ci),
                                     ctypes.POINTER(ci), ctypes.POINTER(ci)]
        L.glx_graph_edge_weight_packed.argtypes = [vp, ctypes.POINTER(ci)]
        L.glx_graph_edge_weight_record_bytes.argtypes = [vp, ctypes.POINTER(ci)]
        L.glx_graph_row_dir.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ctypes.c_int64)]
        L.glx_graph_export_alias.argtypes = [vp, vp, vp, ci, vp]
        L.glx_graph_build_ordered.argtypes = [ci, i64, vp, vp, vp, vp, vp, ci, ci, vp, ctypes.POINTER(vp)]
        L.glx_graph_degrees.argtypes = [vp, vp, i64, vp, ci, vp]
        L.glx_graph_in_degrees.argtypes = [vp, vp, i64, vp, ci, vp]
        L.glx_sample.argtypes = [vp, ci, vp, i32, i32, ci, i64, u64, u64, vp, vp, ci, vp]
        L.glx_sample_ex.argtypes = [vp, ci, vp, vp, i32, i32, ci, i64, u64, u64, vp, vp, ci, vp]
        L.glx_sample_hops.argtypes = [vp, i32, ci, vp, i32, vp, ci, i64, u64, u64, vp, vp, ci, vp]
        L.glx_graph_enable_in_degree.argtypes = [vp, vp]
        L.glx_graph_enable_default_weight.argtypes = [vp, ctypes.c_float, vp]
        L.glx_sample_full_sizes.argtypes = [vp, vp, i32, i32, vp, vp, ci, vp]
        L.glx_sample_full.argtypes = [vp, vp, i32, i32, vp, vp, vp, ci, vp]
        L.glx_graph_set_timestamps.argtypes = [vp, vp, ci, vp]
        L.glx_graph_has_timestamps.argtypes = [vp, ctypes.POINTER(ci)]
        L.glx_sample_temporal.argtypes = [vp, ci, vp, vp, vp, i32, i32, ci, i64, i64, u64, u64, vp, vp, vp, vp, ci, vp]
        L.glx_sample_temporal_hops.argtypes = [vp, i32, ci, vp, vp, i32, vp, ci, i64, i64, u64, u64, vp, vp, vp, vp, ci,
                                               vp]
        L.glx_random_walk.argtypes = [vp, vp, i32, i32, f32, f32, i32, f32, i64, u64, u64, vp, ci, vp]
        L.glx_sample_filtered.argtypes = [vp, ci, vp, vp, i32, i32, ci, i64, u64, u64, ctypes.POINTER(Filter), vp, vp, ci,
                                          vp]
        L.glx_sample_full_filtered.argtypes = [vp, vp, i32, i32, vp, ci, i64, ctypes.POINTER(Filter), vp, vp, ci, vp]
        L.glx_features_view.argtypes = [ci, i64, i32, vp, ctypes.POINTER(vp)]
        L.glx_features_create.argtypes = [ci, i64, i32, vp, vp, ci, vp, ctypes.POINTER(vp)]
        L.glx_features_create_ex.argtypes = [ci, i64, i32, vp, ci, ci, vp, ci, vp, ctypes.POINTER(vp)]
        L.glx_features_view_ex.argtypes = [ci, i64, i32, vp, ci, ctypes.POINTER(vp)]
        L.glx_features_dtype.argtypes = [vp, ctypes.POINTER(ci)]
        L.glx_features_convert_host.argtypes = [vp, i64, ci, vp]
        L.glx_features_destroy.argtypes = [vp]
        L.glx_features_destroy.restype = None
        L.glx_features_info.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i32), ctypes.POINTER(ci),
                                        ctypes.POINTER(ci)]
        L.glx_aggregate.argtypes = [vp, ci, vp, vp, i32, i32, f32, vp, vp, ci, vp]
        L.glx_lookup.argtypes = [vp, vp, i64, f32, vp, ci, vp]
        L.glx_aggregate_arg.argtypes = [vp, ci, vp, vp, i32, i32, f32, vp, vp, vp, ci, vp]
        L.glx_aggregate_backward.argtypes = [ci, ci, vp, vp, vp, i32, i32, i64, i32, vp, vp, ci, vp]
        L.glx_aggregate_weighted.argtypes = [ci, ci, vp, i64, i32, vp, vp, i32, vp, i32, i32, f32, vp, ci, vp]
        L.glx_aggregate_weighted_backward_x.argtypes = [ci, ci, vp, vp, i32, vp, i32, i32, i64, i32, vp, vp, ci, vp]
        L.glx_aggregate_weighted_backward_w.argtypes = [ci, ci, vp, i64, i32, vp, i32, vp, i32, i32, f32, vp, vp, ci, vp]
        L.glx_segment_softmax.argtypes = [ci, vp, i32, vp, i32, i32, vp, ci, vp]
        L.glx_segment_softmax_backward.argtypes = [ci, vp, vp, i32, vp, i32, i32, vp, ci, vp]
        L.glx_gat_attention.argtypes = [ci, vp, vp, i64, vp, i32, vp, i32, i32, f32, f32, f32, u64, u64, vp, vp, ci, vp]
        L.glx_gat_attention_backward.argtypes = [ci, vp, vp, vp, vp, i64, vp, i32, vp, i32, i32, f32, f32, f32, u64, u64,
                                                 vp, vp, vp, ci, vp]
        L.glx_dot_attention.argtypes = [ci, vp, vp, vp, i64, i32, i32, vp, vp, vp, i32, i32, f32, f32, f32, u64, u64, vp,
                                        vp, vp, ci, vp]
        L.glx_dot_attention_backward.argtypes = [ci, vp, vp, vp, i64, i32, i32, vp, vp, vp, i32, i32, f32, f32, f32, u64,
                                                 u64, vp, vp, vp, vp, vp, vp, vp, ci, vp]
        L.glx_pair_dot.argtypes = [ci, vp, i64, vp, i64, i32, i32, vp, vp, i32, i32, f32, vp, ci, vp]
        L.glx_pair_dot_backward.argtypes = [ci, ci, vp, vp, i32, i32, vp, i32, vp, i64, i32, i64, f32, vp, ci, vp]
        # the _ex siblings: the table pointer is followed (or, for pair_dot, the pair of tables is followed) by a dtype id
        L.glx_aggregate_backward_ex.argtypes = [ci, ci, vp, vp, vp, i32, i32, i64, i32, vp, vp, ci, ci, vp]
        L.glx_aggregate_weighted_ex.argtypes = [ci, ci, vp, ci, i64, i32, vp, vp, i32, vp, i32, i32, f32, vp, ci, vp]
        L.glx_aggregate_weighted_backward_x_ex.argtypes = [ci, ci, vp, vp, i32, vp, i32, i32, i64, i32, vp, vp, ci, ci,
                                                           vp]
        L.glx_aggregate_weighted_backward_w_ex.argtypes = [ci, ci, vp, ci, i64, i32, vp, i32, vp, i32, i32, f32, vp, vp,
                                                           ci, vp]
        L.glx_pair_dot_ex.argtypes = [ci, vp, i64, vp, i64, ci, i32, i32, vp, vp, i32, i32, f32, vp, ci, vp]
        L.glx_pair_dot_backward_ex.argtypes = [ci, ci, vp, vp, i32, i32, vp, i32, vp, i64, i32, i64, f32, vp, ci, ci,
                                               vp]
        # the chunked order of the two row gradients: their _ex siblings' arguments
        L.glx_aggregate_backward_chunked.argtypes = L.glx_aggregate_backward_ex.argtypes
        L.glx_aggregate_weighted_backward_x_chunked.argtypes = L.glx_aggregate_weighted_backward_x_ex.argtypes
        # the chunked order of dot-product attention: the default entry points' arguments
        L.glx_dot_attention_chunked.argtypes = L.glx_dot_attention.argtypes
        L.glx_dot_attention_backward_chunked.argtypes = L.glx_dot_attention_backward.argtypes
        L.glx_rows_coalesce.argtypes =[ci, vp, i32, i64, i32, vp, vp, vp, vp, ci, vp]
        L.glx_embedding_update.argtypes = [ci, ci, vp, vp, vp, i64, i32, vp, vp, i32, f32, f32, f32, f32, f32, f32, vp]
        L.glx_tgn_store_update.argtypes = [ci, i64, i32, vp, vp, vp, vp, i32, i64, vp, vp, vp, vp, vp]
        L.glx_tgn_message.argtypes = [ci, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp,
                                      vp]
        L.glx_tgn_message_backward.argtypes = [ci, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.glx_tgn_memory_write.argtypes = [ci, i64, i32, vp, i32, vp, vp, vp, vp, vp]
        L.glx_partition.argtypes = [ci, vp, i64, i32, vp, vp, vp, vp]
        L.glx_stitch_i64.argtypes = [ci, vp, vp, i64, i32, vp, vp]
        L.glx_stitch_f32.argtypes = [ci, vp, vp, i64, i32, vp, vp]
        L.glx_aggregate_stitch.argtypes = [ci, ci, i32, vp, vp, i32, i32, f32, vp, vp, vp]
        L.glx_negative_create.argtypes = [ci, i64, vp, vp, ci, vp, ctypes.POINTER(vp)]
        L.glx_negative_from_graph.argtypes = [vp, ci, vp, ctypes.POINTER(vp)]
        L.glx_negative_destroy.argtypes = [vp]
        L.glx_negative_destroy.restype = None
        L.glx_negative_info.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(ci)]
        L.glx_negative_export.argtypes = [vp, vp, vp, vp, vp]
        L.glx_graph_enable_negative.argtypes = [vp, vp]
        L.glx_negative_sample.argtypes = [vp, ci, vp, vp, i32, i32, i64, u64, u64, vp, ci, vp]
        L.glx_profile_enable.argtypes = [ci]
        L.glx_profile_collect.argtypes = [ci, vp, i32, ctypes.POINTER(i32)]
        L.glx_comm_unique_id.argtypes = [vp]
        L.glx_comm_init_rccl.argtypes = [ci, ci, ci, vp, ctypes.POINTER(vp)]
        L.glx_comm_init_local.argtypes = [i64, ci, ci, ci, ctypes.POINTER(vp)]
        L.glx_comm_init_callbacks.argtypes = [ci, ci, ci, HOST_ALLTOALLV_FN, HOST_ALLGATHER_FN, vp, ctypes.POINTER(vp)]
        L.glx_comm_destroy.argtypes = [vp]
        L.glx_comm_destroy.restype = None
        L.glx_comm_info.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci)]
        L.glx_comm_set_max_message_bytes.argtypes = [vp, i64]
        L.glx_comm_set_max_message_bytes.restype = i64
        L.glx_exchange_v.argtypes = [vp, vp, vp, vp, vp, i64, ci, vp]
        L.glx_comm_allgather_i64.argtypes = [vp, vp, i32, vp, ci, vp]
        L.glx_comm_barrier.argtypes = [vp, vp]
        L.glx_dist_store_create.argtypes = [vp, vp, vp, ctypes.POINTER(vp)]
        L.glx_dist_store_destroy.argtypes = [vp]
        L.glx_dist_store_destroy.restype = None
        L.glx_dist_store_set_cache.argtypes = [vp, vp, i64, f32, ci, vp]
        L.glx_dist_store_set_graph_replica.argtypes = [vp, vp]
        L.glx_dist_build_graph_replica.argtypes = [vp, vp, i64, ci, vp, vp]
        L.glx_dist_random_walk.argtypes = [vp, vp, i32, i32, f32, f32, i64, u64, u64, vp, ci, vp]
        L.glx_dist_random_walk_ex.argtypes = [vp, vp, i32, i32, f32, f32, i32, f32, i64, u64, u64, vp, ci, vp]
        L.glx_dist_sample_full_sizes.argtypes = [vp, vp, i32, i32, vp, vp, ci, vp]
        L.glx_dist_sample_full.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, i64, ci, vp]
        L.glx_dist_sample_full_filtered.argtypes = [vp, vp, i32, i32, vp, vp, ci, i64, vp, vp, vp, i64, ci, vp]
        L.glx_dist_in_degrees.argtypes = [vp, vp, i32, vp, ci, vp]
        L.glx_dist_negative_create.argtypes = [vp, ci, vp, ctypes.POINTER(vp)]
        L.glx_dist_negative_sample.argtypes = [vp, vp, ci, vp, i32, i32, i64, u64, u64, vp, ci, vp]
        L.glx_dist_last_sample_rows.argtypes = [vp, vp, vp, vp]
        L.glx_dist_hot_ids.argtypes = [vp, i64, vp, ctypes.POINTER(i64), vp]
        L.glx_dist_enable_in_degree.argtypes = [vp, vp, vp]
        L.glx_dist_sample.argtypes = [vp, ci, vp, i32, i32, ci, i64, u64, u64, ctypes.POINTER(Filter), vp, vp, ci, vp]
        L.glx_dist_aggregate.argtypes = [vp, ci, vp, vp, i32, i32, f32, vp, vp, ci, vp]
        L.glx_dist_aggregate_partial.argtypes = [vp, ci, vp, vp, i32, i32, f32, vp, vp, ci, vp]
        L.glx_dist_lookup.argtypes = [vp, vp, i64, f32, vp, ci, vp]
        L.glx_dist_aggregate_begin.argtypes = [vp, i32, vp, i32, f32, vp]
        L.glx_dist_aggregate_end.argtypes = [vp, i32, ci, vp, i32, vp, vp, vp]
        L.glx_dist_aggregate_end_range.argtypes = [vp, i32, i32, i32, ci, ci, vp, i32, vp, vp, vp]
        L.glx_dist_last_stats.argtypes = [vp, ctypes.POINTER(DistStats)]
        L.glx_dist_ledger_create.argtypes = [ci, ctypes.POINTER(vp)]
        L.glx_dist_ledger_destroy.argtypes = [vp]
        L.glx_dist_ledger_destroy.restype = None
        L.glx_dist_store_set_ledger.argtypes = [vp, vp]
        L.glx_dist_confirm.argtypes = [vp, vp]
        L.glx_dist_ledger_get_stats.argtypes = [vp, ctypes.POINTER(LedgerStats)]
        L.glx_dist_ledger_set_slack.argtypes = [vp, ctypes.c_double, i64]
        L.glx_plan_create.argtypes = [vp, i32, ci, vp, i32, ci, i64, u64, vp, ci, f32, ctypes.POINTER(vp)]
        L.glx_plan_run.argtypes = [vp, vp, u64, vp]
        L.glx_plan_output.argtypes = [vp, i32, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp),
                                      ctypes.POINTER(vp), ctypes.POINTER(i64), ctypes.POINTER(i32)]
        L.glx_plan_destroy.argtypes = [vp]
        L.glx_cond_table_create.argtypes = [ci, i64, vp, vp, i32, vp, ci, vp, ctypes.POINTER(vp)]
        L.glx_cond_table_destroy.argtypes = [vp]
        L.glx_cond_table_destroy.restype = None
        L.glx_cond_negative_sample.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, ci, ci, i32, i64, u64, u64, vp, ci, vp]
        L.glx_subgraph_induce.argtypes = [ci, vp, i32, vp, vp, vp, vp, vp, vp, i64, ctypes.POINTER(i64), ci, vp]
        L.glx_probe_bandwidth.argtypes = [ci, ci, i64, i64, i32, i32, ctypes.POINTER(ctypes.c_double),
                                          ctypes.POINTER(ctypes.c_double), vp]
        L.glx_tune.argtypes = [ctypes.c_char_p, i32]
        L.glx_knn_search.argtypes = [vp, ci, vp, i32, i32, vp, vp, ci, vp]
        L.glx_knn_merge.argtypes = [ci, ci, i32, vp, vp, i32, i32, vp, vp, ci, vp]
        L.glx_knn_ivf_build.argtypes = [vp, i32, i32, i64, vp, ci, vp, ctypes.POINTER(vp)]
        L.glx_knn_ivf_search.argtypes = [vp, ci, vp, i32, i32, i32, vp, vp, ci, vp]
        L.glx_knn_ivf_info.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i64),
                                       ctypes.POINTER(i64), ctypes.POINTER(i64)]
        L.glx_knn_ivf_export.argtypes = [vp, vp, vp, vp, ci, vp]
        L.glx_knn_ivf_destroy.argtypes = [vp]
        L.glx_knn_ivf_destroy.restype = None
        L.glx_knn_ivfpq_build.argtypes = [vp, i32, i32, i64, vp, ci, vp, ctypes.POINTER(vp)]
        L.glx_knn_ivfpq_search.argtypes = [vp, ci, vp, i32, i32, i32, i32, vp, vp, ci, vp]
        L.glx_knn_ivfpq_info.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i64),
                                         ctypes.POINTER(i64)]
        L.glx_knn_ivfpq_export.argtypes = [vp, vp, vp, ci, vp]
        L.glx_knn_ivfpq_destroy.argtypes = [vp]
        L.glx_knn_ivfpq_destroy.restype = None
        L.glx_unique.argtypes = [ci, vp, vp, i32, vp, vp, vp, ci, vp]
        L.glx_columns_create.argtypes = [ci, i64, i32, vp, vp, vp, vp, vp, vp, ci, vp, ctypes.POINTER(vp)]
        L.glx_columns_destroy.argtypes = [vp]
        L.glx_columns_destroy.restype = None
        L.glx_columns_info.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i32), ctypes.POINTER(ci), ctypes.POINTER(ci),
                                       ctypes.POINTER(ci), ctypes.POINTER(i32), ctypes.POINTER(ci), ctypes.POINTER(ci)]
        L.glx_columns_lookup.argtypes = [vp, vp, i64, f32, i32, i64, i64, vp, vp, vp, vp, ci, vp]
        L.glx_plan_destroy.restype = None
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise GlxError(rc, lib().glx_last_error().decode())


def device_count():
    n = ctypes.c_int(0)
    _check(lib().glx_device_count(ctypes.byref(n)))
    return n.value


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _ptr(x, dtype=None):
    """(pointer, kind) of a numpy array or a torch CUDA tensor; None -> NULL."""
    if x is None:
        return None, None
    if _is_torch(x):
        assert x.is_cuda and x.is_contiguous(), "torch inputs must be contiguous CUDA tensors"
        return ctypes.c_void_p(x.data_ptr()), PTR_DEVICE
    assert isinstance(x, np.ndarray) and x.flags["C_CONTIGUOUS"]
    if dtype is not None:
        assert x.dtype == dtype, (x.dtype, dtype)
    return ctypes.c_void_p(x.ctypes.data), PTR_HOST


def _kind(*xs):
    kinds = set(k for _, k in xs if k is not None)
    assert len(kinds) == 1, "all data pointers of a call must be host (numpy) or device (torch)"
    return kinds.pop()


def _stream(kind, device=None):
    """torch's current stream ON THE DEVICE THE HANDLE LIVES ON (not on torch's current device: a process
    that drives several GPUs, or set_device_id() without torch.cuda.set_device(), would otherwise pass a
    stream of another device)."""
    if kind == PTR_DEVICE:
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    return None


class Graph:
    """Device-resident CSR of one edge type (glx_graph)."""

    def __init__(self, row_ptr, col, eid, weight=None, ids=None, device=0):
        ptrs = [_ptr(row_ptr), _ptr(col), _ptr(eid), _ptr(weight), _ptr(ids)]
        kind = _kind(*ptrs)
        self.num_rows = int(row_ptr.shape[0]) - 1
        self.num_edges = int(col.shape[0])
        self.device = device
        h = ctypes.c_void_p()
        _check(lib().glx_graph_create(device, self.num_rows, self.num_edges, ptrs[0][0], ptrs[1][0],
                                      ptrs[2][0], ptrs[3][0], ptrs[4][0], kind, _stream(kind, self.device),
                                      ctypes.byref(h)))
        self._h = h

    @classmethod
    def from_edges(cls, src, dst, weight=None, edge_ids=None, sort_by_weight=True, device=0, timestamp=None):
        """Device-side build from a raw edge list in insertion order (edge id = index,
        or edge_ids[i] for a shard's subset of a global edge list).  Rows are ordered by
        timestamp ascending when timestamps are given (timestamped edge types), else by
        weight descending (sort_by_weight), else left in insertion order."""
        self = cls.__new__(cls)
        ptrs = [_ptr(src), _ptr(dst), _ptr(weight), _ptr(edge_ids), _ptr(timestamp)]
        kind = _kind(*ptrs)
        h = ctypes.c_void_p()
        order = 2 if timestamp is not None else (1 if sort_by_weight else 0)
        _check(lib().glx_graph_build_ordered(device, int(src.shape[0]), ptrs[0][0], ptrs[1][0], ptrs[2][0],
                                             ptrs[3][0], ptrs[4][0], order, kind, _stream(kind, device), ctypes.byref(h)))
        self._h = h
        self.device = device
        v, e = ctypes.c_int64(), ctypes.c_int64()
        _check(lib().glx_graph_info(h, ctypes.byref(v), ctypes.byref(e), None, None, None))
        self.num_rows, self.num_edges = v.value, e.value
        return self

    @classmethod
    def from_handle(cls, handle, device=0):
        """Borrow a glx_graph* owned by someone else (e.g. the C++ host layer's GraphStore)."""
        self = cls.__new__(cls)
        self._h = ctypes.c_void_p(int(handle))
        self._borrowed = True
        v, e, d = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
        _check(lib().glx_graph_info(self._h, ctypes.byref(v), ctypes.byref(e), None, None, ctypes.byref(d)))
        self.num_rows, self.num_edges = v.value, e.value
        self.device = d.value  # the device the handle lives on, whatever the caller passed
        return self

    def close(self):
        if getattr(self, "_borrowed", False):
            self._h = None
        if getattr(self, "_h", None):
            try:
                lib().glx_graph_destroy(self._h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None

    __del__ = close

    def enable_negative(self):
        """Sort every row's neighbour ids (the exclusion test of strict negative sampling)."""
        _check(lib().glx_graph_enable_negative(self._h, None))

    enable_id_index = enable_negative  # the same per-row id-sorted index serves id == value filters

    def enable_in_degree(self):
        """Build the in-degree alias tables InDegreeSampler needs (once, on the device)."""
        _check(lib().glx_graph_enable_in_degree(self._h, None))
        return self

    def enable_default_weight(self, default_weight=0.0):
        """EdgeWeightSampler on an unweighted graph: every slot weighs `default_weight` (the reference's
        GLOBAL_FLAG(DefaultWeight)); builds the alias tables of that.  No effect on a weighted graph."""
        _check(lib().glx_graph_enable_default_weight(self._h, ctypes.c_float(default_weight), None))
        return self

    def sample_full(self, src, max_limit=0):
        """FullSampler: -> (degrees[batch] int32, nbr[total], eid[total]) (sparse response)."""
        batch = int(src.shape[0])
        if _is_torch(src):
            import torch
            deg = torch.empty(batch, dtype=torch.int32, device=src.device)
            off = torch.empty(batch + 1, dtype=torch.int64, device=src.device)
            _check(lib().glx_sample_full_sizes(self._h, _ptr(src)[0], batch, max_limit, _ptr(deg)[0], _ptr(off)[0],
                                               PTR_DEVICE, _stream(PTR_DEVICE, self.device)))
            total = int(off[-1].item())
            nbr = torch.empty(total, dtype=torch.int64, device=src.device)
            eid = torch.empty(total, dtype=torch.int64, device=src.device)
            _check(lib().glx_sample_full(self._h, _ptr(src)[0], batch, max_limit, _ptr(off)[0], _ptr(nbr)[0],
                                         _ptr(eid)[0], PTR_DEVICE, _stream(PTR_DEVICE, self.device)))
            return deg, nbr, eid
        deg = np.empty(batch, np.int32)
        off = np.empty(batch + 1, np.int64)
        _check(lib().glx_sample_full_sizes(self._h, _ptr(src)[0], batch, max_limit, _ptr(deg)[0], _ptr(off)[0],
                                           PTR_HOST, None))
        total = int(off[-1])
        nbr = np.empty(total, np.int64)
        eid = np.empty(total, np.int64)
        _check(lib().glx_sample_full(self._h, _ptr(src)[0], batch, max_limit, _ptr(off)[0], _ptr(nbr)[0],
                                     _ptr(eid)[0], PTR_HOST, None))
        return deg, nbr, eid

    def set_timestamps(self, ts_slot):
        """Per-slot edge timestamps (CSR order) for a handle made from a CSR; mutates the handle."""
        p, kind = _ptr(ts_slot)
        _check(lib().glx_graph_set_timestamps(self._h, p, kind, _stream(kind, self.device)))

    @property
    def has_timestamps(self):
        """Whether the graph keeps per-slot timestamps (what sample_temporal needs)."""
        h = ctypes.c_int(0)
        _check(lib().glx_graph_has_timestamps(self._h, ctypes.byref(h)))
        return bool(h.value)

    def sample_temporal(self, src, cutoff, k, strategy="recent", inclusive=False, seed=0, call_counter=0,
                        default_neighbor_id=0, default_timestamp=-1, rng_rows=None):
        """The neighbours of src[i] over edges with a timestamp < cutoff[i] (<= when inclusive): the k latest, latest
        first ("recent"), or k uniform draws with replacement ("uniform").  -> (nbr[batch, k], eid[batch, k],
        ts[batch, k] int64, cnt[batch] int32): row i holds cnt[i] sampled edges in its first slots, the others are
        (default_neighbor_id, -1, default_timestamp).  numpy in -> numpy out, torch in -> torch out (nothing is read
        back; runs on torch's current stream)."""
        if isinstance(strategy, str):
            strategy = TEMPORAL_STRATEGIES[strategy]
        batch = int(src.shape[0])
        nbr, eid, ts, cnt = _temporal_outputs(src, batch, k)
        ps, pc, pr = _ptr(src), _ptr(cutoff), _ptr(rng_rows)
        pn, pe, pt, pk = _ptr(nbr), _ptr(eid), _ptr(ts), _ptr(cnt)
        kind = _kind(ps, pc, pr, pn)
        _check(lib().glx_sample_temporal(self._h, strategy, ps[0], pc[0], pr[0], batch, k, 1 if inclusive else 0,
                                         default_neighbor_id, default_timestamp, seed, call_counter, pn[0], pe[0],
                                         pt[0], pk[0], kind, _stream(kind, self.device)))
        return nbr, eid, ts, cnt

    def sample_filtered(self, sampler, src, k, filter_type, filter_field, values, seed=0, call_counter=0,
                        padding_mode=PAD_CIRCULAR, default_neighbor_id=0, retry_times=5, default_timestamp=-1,
                        rng_rows=None):
        """Sampling with a Filter: values[batch] is the expanded filter tensor (same kind as src)."""
        if isinstance(sampler, str):
            sampler = SAMPLER_IDS[sampler] if sampler in SAMPLER_IDS else EXTRA_SAMPLER_IDS[sampler]
        batch = int(src.shape[0])
        if _is_torch(src):
            import torch
            nbr = torch.empty((batch, k), dtype=torch.int64, device=src.device)
            eid = torch.empty((batch, k), dtype=torch.int64, device=src.device)
        else:
            nbr = np.empty((batch, k), np.int64)
            eid = np.empty((batch, k), np.int64)
        ps, pn, pe, pr, pv = _ptr(src), _ptr(nbr), _ptr(eid), _ptr(rng_rows), _ptr(values)
        kind = _kind(ps, pn, pe, pr, pv)
        flt = Filter(filter_type, filter_field, pv[0], retry_times, default_timestamp)
        _check(lib().glx_sample_filtered(self._h, sampler, ps[0], pr[0], batch, k, padding_mode, default_neighbor_id,
                                         seed, call_counter, ctypes.byref(flt), pn[0], pe[0], kind, _stream(kind, self.device)))
        return nbr, eid

    def sample_full_filtered(self, src, max_limit, filter_type, filter_field, values, padding_mode=PAD_CIRCULAR,
                             default_neighbor_id=0, default_timestamp=-1):
        """FullSampler with a Filter: -> (degrees, nbr, eid); the segments are the unfiltered ones."""
        batch = int(src.shape[0])
        torch_in = _is_torch(src)
        if torch_in:
            import torch
            deg = torch.empty(batch, dtype=torch.int32, device=src.device)
            off = torch.empty(batch + 1, dtype=torch.int64, device=src.device)
        else:
            deg = np.empty(batch, np.int32)
            off = np.empty(batch + 1, np.int64)
        kind = PTR_DEVICE if torch_in else PTR_HOST
        _check(lib().glx_sample_full_sizes(self._h, _ptr(src)[0], batch, max_limit, _ptr(deg)[0], _ptr(off)[0], kind,
                                           _stream(kind, self.device)))
        total = int(off[-1].item()) if torch_in else int(off[-1])
        if torch_in:
            nbr = torch.empty(total, dtype=torch.int64, device=src.device)
            eid = torch.empty(total, dtype=torch.int64, device=src.device)
        else:
            nbr = np.empty(total, np.int64)
            eid = np.empty(total, np.int64)
        flt = Filter(filter_type, filter_field, _ptr(values)[0], 0, default_timestamp)
        _check(lib().glx_sample_full_filtered(self._h, _ptr(src)[0], batch, max_limit, _ptr(off)[0], padding_mode,
                                              default_neighbor_id, ctypes.byref(flt), _ptr(nbr)[0], _ptr(eid)[0], kind,
                                              _stream(kind, self.device)))
        return deg, nbr, eid

    def random_walk(self, seeds, walk_len, p=1.0, q=1.0, full_nbr_num=100, default_weight=0.0, default_neighbor_id=0,
                    seed=0, call_counter=0):
        """RandomWalk operator: -> walks[batch, walk_len] (DeepWalk when p = q = 1, node2vec otherwise)."""
        batch = int(seeds.shape[0])
        if _is_torch(seeds):
            import torch
            walks = torch.empty((batch, walk_len), dtype=torch.int64, device=seeds.device)
        else:
            walks = np.empty((batch, walk_len), np.int64)
        ps, pw = _ptr(seeds), _ptr(walks)
        kind = _kind(ps, pw)
        _check(lib().glx_random_walk(self._h, ps[0], batch, walk_len, p, q, full_nbr_num, default_weight,
                                     default_neighbor_id, seed, call_counter, pw[0], kind, _stream(kind, self.device)))
        return walks

    def edge_weight_packed(self):
        """True when EdgeWeightSampler draws from the packed per-slot records (every edge id fits an int32)."""
        p = ctypes.c_int(0)
        _check(lib().glx_graph_edge_weight_packed(self._h, ctypes.byref(p)))
        return bool(p.value)

    def edge_weight_record_bytes(self):
        """Bytes per packed EdgeWeight record: 20 (int32 ids, three records to a 64-byte sector), 32 (int64 neighbour
        ids) or 0 (no records: the alias tables serve the draws)."""
        p = ctypes.c_int(0)
        _check(lib().glx_graph_edge_weight_record_bytes(self._h, ctypes.byref(p)))
        return int(p.value)

    def row_dir(self):
        """-> (form, bytes) of the row directory the samplers look ids up in: form "direct" (8 bytes per id in
        [0, max_id]), "hashed16" (16 bytes per slot of the id map) or None (the id map and row_ptr answer)."""
        f, b = ctypes.c_int(0), ctypes.c_int64(0)
        _check(lib().glx_graph_row_dir(self._h, ctypes.byref(f), ctypes.byref(b)))
        return (None, "direct", "hashed16")[f.value], int(b.value)

    def export_alias(self):
        prob = np.empty(self.num_edges, np.float32)
        alias = np.empty(self.num_edges, np.int32)
        _check(lib().glx_graph_export_alias(self._h, _ptr(prob)[0], _ptr(alias)[0], PTR_HOST, None))
        return prob, alias

    def degrees(self, src):
        if _is_torch(src):
            import torch
            out = torch.empty(src.shape[0], dtype=torch.int64, device=src.device)
        else:
            out = np.empty(src.shape[0], np.int64)
        (ps, k1), (po, _) = _ptr(src), _ptr(out)
        _check(lib().glx_graph_degrees(self._h, ps, src.shape[0], po, k1, _stream(k1, self.device)))
        return out

    def in_degrees(self, ids):
        """In-degrees of raw destination ids (needs enable_in_degree())."""
        if _is_torch(ids):
            import torch
            out = torch.empty(ids.shape[0], dtype=torch.int64, device=ids.device)
        else:
            out = np.empty(ids.shape[0], np.int64)
        (ps, k1), (po, _) = _ptr(ids), _ptr(out)
        _check(lib().glx_graph_in_degrees(self._h, ps, ids.shape[0], po, k1, _stream(k1, self.device)))
        return out

    def sample(self, sampler, src, k, seed=0, call_counter=0, padding_mode=PAD_CIRCULAR,
               default_neighbor_id=0, out=None, rng_rows=None):
        """-> (nbr[batch, k], eid[batch, k]) int64; numpy in -> numpy out, torch in -> torch out."""
        if isinstance(sampler, str):
            sampler = SAMPLER_IDS[sampler] if sampler in SAMPLER_IDS else EXTRA_SAMPLER_IDS[sampler]
        batch = int(src.shape[0])
        if out is not None:
            nbr, eid = out
        elif _is_torch(src):
            import torch
            nbr = torch.empty((batch, k), dtype=torch.int64, device=src.device)
            eid = torch.empty((batch, k), dtype=torch.int64, device=src.device)
        else:
            nbr = np.empty((batch, k), np.int64)
            eid = np.empty((batch, k), np.int64)
        ps, pn, pe, pr = _ptr(src), _ptr(nbr), _ptr(eid), _ptr(rng_rows)
        kind = _kind(ps, pn, pe, pr)
        _check(lib().glx_sample_ex(self._h, sampler, ps[0], pr[0], batch, k, padding_mode,
                                   default_neighbor_id, seed, call_counter, pn[0], pe[0], kind,
                                   _stream(kind, self.device)))
        return nbr, eid


# storage types of a feature table (GLX_DTYPE_*)
FEATURE_DTYPES = {"float32": 0, "bfloat16": 1, "float16": 2}
# OCP float8 storage (GLX_DTYPE_F8E4M3 / GLX_DTYPE_F8E5M2): one byte per element.  e4m3fn has no infinity: float32
# input beyond +-464 is stored as NaN, not as the largest number -- normalise such features first.
FP8_FEATURE_DTYPES = {"float8_e4m3fn": 8, "float8_e5m2": 9}
_ALL_FEATURE_DTYPES = dict(FEATURE_DTYPES, **FP8_FEATURE_DTYPES)
_FEATURE_DTYPE_NAMES = {v: k for k, v in _ALL_FEATURE_DTYPES.items()}


def _feature_dtype_of(X):
    """float32 / bfloat16 / float16 for a torch tensor or a numpy array, float8_e4m3fn / float8_e5m2 for a torch
    tensor (numpy has no float8 type: a uint8 matrix is not a feature matrix); anything else raises."""
    name = str(X.dtype).replace("torch.", "") if _is_torch(X) else str(np.dtype(X.dtype))
    if name not in _ALL_FEATURE_DTYPES:
        raise ValueError("a feature matrix holds float32, bfloat16, float16 or (torch) float8_e4m3fn / float8_e5m2, "
                         "not {}".format(X.dtype))
    return name


class Features:
    """Device-resident [V, D] node features of one node type (glx_features), stored as float32 (the default),
    bfloat16, float16, float8_e4m3fn or float8_e5m2.  aggregate(), lookup() and search() answer in float32 whatever
    the storage type."""

    def __init__(self, X, ids=None, device=0, view=False, dtype=None):
        """X: float32 / bfloat16 / float16 / float8 -- numpy (float32, float16) or torch (host or CUDA).  dtype=None
        stores X's own type; "bfloat16" / "float16" / "float8_e4m3fn" / "float8_e5m2" rounds float32 input on the device
        (round to nearest even, as torch's .to(); float8_e4m3fn turns overflow into NaN: it has no infinity).
        view=True: non-owning view of a torch CUDA matrix (dense ids, its own dtype); keeps X alive."""
        if dtype is not None and dtype not in _ALL_FEATURE_DTYPES:
            raise ValueError("dtype must be None or one of {}, not {!r}".format(sorted(_ALL_FEATURE_DTYPES), dtype))
        x_dtype = _feature_dtype_of(X)
        store = dtype or x_dtype
        if store != x_dtype and x_dtype != "float32":
            raise ValueError("only float32 input converts; a {} matrix cannot be stored as {}".format(x_dtype, store))
        self.dtype = store
        if view:
            assert ids is None and _is_torch(X)
            if store != x_dtype:
                raise ValueError("a view reads the caller's {} rows as they are; it cannot store {}".format(x_dtype, store))
            self.num_rows, self.dim = int(X.shape[0]), int(X.shape[1])
            self.device = device
            self._keep = X
            h = ctypes.c_void_p()
            _check(lib().glx_features_view_ex(device, self.num_rows, self.dim, _ptr(X)[0], _ALL_FEATURE_DTYPES[store],
                                              ctypes.byref(h)))
            self._h = h
            return
        if _is_torch(X) and not X.is_cuda:  # a host tensor: its bits as a numpy array (numpy has no bfloat16)
            import torch
            X = X.contiguous()
            if x_dtype == "float32":
                X = X.numpy()
            else:
                X = X.view(torch.uint8 if x_dtype in FP8_FEATURE_DTYPES else torch.int16).numpy()
        ptrs = [_ptr(X), _ptr(ids)]
        kind = _kind(*ptrs)
        self.num_rows, self.dim = int(X.shape[0]), int(X.shape[1])
        self.device = device
        h = ctypes.c_void_p()
        _check(lib().glx_features_create_ex(device, self.num_rows, self.dim, ptrs[0][0], _ALL_FEATURE_DTYPES[x_dtype],
                                            _ALL_FEATURE_DTYPES[store], ptrs[1][0], kind, _stream(kind, self.device),
                                            ctypes.byref(h)))
        self._h = h

    @classmethod
    def from_handle(cls, handle, device=0):
        """Borrow a glx_features* owned by someone else (the C++ host layer's Noder)."""
        self = cls.__new__(cls)
        self._h = ctypes.c_void_p(int(handle))
        self._borrowed = True
        v, d, dv = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int()
        _check(lib().glx_features_info(self._h, ctypes.byref(v), ctypes.byref(d), None, ctypes.byref(dv)))
        self.num_rows, self.dim = v.value, d.value
        self.device = dv.value  # the device the handle lives on, whatever the caller passed
        dt = ctypes.c_int()
        _check(lib().glx_features_dtype(self._h, ctypes.byref(dt)))
        self.dtype = _FEATURE_DTYPE_NAMES[dt.value]
        return self

    def close(self):
        if getattr(self, "_borrowed", False):
            self._h = None
        if getattr(self, "_h", None):
            try:
                lib().glx_features_destroy(self._h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None

    __del__ = close

    def aggregate(self, op, node_ids, segment_ids, num_segments, default_attr=0.0, out=None):
        """-> (emb[num_segments, D] float32, counts[num_segments] int32)."""
        if isinstance(op, str):
            op = AGGREGATOR_IDS[op]
        n = int(node_ids.shape[0])
        if out is not None:
            emb, cnt = out
        elif _is_torch(node_ids):
            import torch
            emb = torch.empty((num_segments, self.dim), dtype=torch.float32, device=node_ids.device)
            cnt = torch.empty((num_segments,), dtype=torch.int32, device=node_ids.device)
        else:
            emb = np.empty((num_segments, self.dim), np.float32)
            cnt = np.empty((num_segments,), np.int32)
        # segment_ids=None: num_segments equal segments of n / num_segments ids (a dense sampler response)
        pi, pg, pe, pc = _ptr(node_ids), _ptr(segment_ids), _ptr(emb), _ptr(cnt)
        kind = _kind(pi, pg, pe, pc)
        _check(lib().glx_aggregate(self._h, op, pi[0], pg[0], n, num_segments, default_attr, pe[0],
                                   pc[0], kind, _stream(kind, self.device)))
        return emb, cnt

    def aggregate_arg(self, op, node_ids, segment_ids, num_segments, default_attr=0.0, out=None):
        """aggregate() for Max / Min that also records where each extreme came from (glx_aggregate_arg)
        -> (emb[num_segments, D] float32, counts[num_segments] int32, arg[num_segments, D] int32): emb and counts are
        aggregate()'s bit for bit; arg is the request position of the first element that attains the extreme, -1 when
        nothing replaced the fold's start value.  aggregate_backward() takes counts and arg.
        out=(emb, counts, arg): buffers of those shapes and types to write into (torch CUDA tensors or numpy arrays,
        handed to the entry point as they are); anything of another shape or type raises ValueError."""
        if isinstance(op, str):
            op = AGGREGATOR_IDS[op]
        n = int(node_ids.shape[0])
        if out is not None:
            emb, cnt, arg = out
            want = (("emb", emb, (num_segments, self.dim), "float32"), ("counts", cnt, (num_segments,), "int32"),
                    ("arg", arg, (num_segments, self.dim), "int32"))
            for name, buf, shape, dtype in want:
                if tuple(buf.shape) != shape or str(buf.dtype).replace("torch.", "") != dtype:
                    raise ValueError("aggregate_arg: out's {} must be {} of shape {}, not {} of shape {}".format(
                        name, dtype, shape, buf.dtype, tuple(buf.shape)))
        elif _is_torch(node_ids):
            import torch
            emb = torch.empty((num_segments, self.dim), dtype=torch.float32, device=node_ids.device)
            cnt = torch.empty((num_segments,), dtype=torch.int32, device=node_ids.device)
            arg = torch.empty((num_segments, self.dim), dtype=torch.int32, device=node_ids.device)
        else:
            emb = np.empty((num_segments, self.dim), np.float32)
            cnt = np.empty((num_segments,), np.int32)
            arg = np.empty((num_segments, self.dim), np.int32)
        pi, pg, pe, pc, pa = _ptr(node_ids), _ptr(segment_ids), _ptr(emb), _ptr(cnt), _ptr(arg)
        kind = _kind(pi, pg, pe, pc, pa)
        _check(lib().glx_aggregate_arg(self._h, op, pi[0], pg[0], n, num_segments, default_attr, pe[0], pc[0], pa[0],
                                       kind, _stream(kind, self.device)))
        return emb, cnt, arg

    def lookup(self, node_ids, default_attr=0.0):
        n = int(node_ids.shape[0])
        if _is_torch(node_ids):
            import torch
            out = torch.empty((n, self.dim), dtype=torch.float32, device=node_ids.device)
        else:
            out = np.empty((n, self.dim), np.float32)
        pi, po = _ptr(node_ids), _ptr(out)
        kind = _kind(pi, po)
        _check(lib().glx_lookup(self._h, pi[0], n, default_attr, po[0], kind, _stream(kind, self.device)))
        return out


    def search(self, queries, k, metric="ip", out=None):
        """Exact k nearest rows of every query (glx_knn_search) -> (ids[n, k] int64, dist[n, k] float32), best first.
        queries[n, D] float32; metric "ip" (inner product, larger is better) or "l2" (squared distance by expansion,
        smaller is better).  The score is one ascending fmaf chain over the columns, ties go to the smaller storage
        row, NaN scores come last, k > num_rows pads with id -1 and dist -inf (ip) / +inf (l2); 1 <= k <= 1024.  ids are
        node ids (row numbers for a table without an id map).  Numpy in, numpy out; torch CUDA tensors in, torch CUDA
        tensors out on the current stream, nothing read back.  out=(ids, dist): buffers to write into."""
        return _knn_search(lib().glx_knn_search, lambda: self._h, self.dim, self.device, queries, k, metric, out)

    def build_ivf(self, nlist, niter=10, train_rows=None, centroids=None):
        """An IVF-Flat index over this table (glx_knn_ivf_build) -> KnnIvf.  nlist lists, niter Lloyd iterations over a
        sample of train_rows rows (None: min(num_rows, 256 * nlist)), starting from centroids[nlist, D] float32 (numpy
        or a torch CUDA tensor) when given, else from evenly spaced sample rows; niter=0 with centroids only assigns.
        The build is deterministic.  The index keeps this table alive."""
        return KnnIvf(self, nlist, niter, train_rows, centroids)

    def build_ivfpq(self, nlist, m, niter=10, train_rows=None, centroids=None, codebooks=None):
        """An IVF-PQ index over this table -> KnnIvfPq: build_ivf(nlist, niter, train_rows, centroids) and, on top of
        it, KnnIvf.build_pq(m, niter, train_rows, codebooks).  The returned object keeps the KnnIvf (its .ivf) and this
        table alive."""
        return self.build_ivf(nlist, niter, train_rows, centroids).build_pq(m, niter, train_rows, codebooks)


KNN_METRICS = {"l2": 0, "ip": 1}  # GLX_KNN_L2, GLX_KNN_IP


class _KnnIndex:
    """close() and the context manager of an index handle; a subclass names its destroy function."""
    _destroy = None

    def close(self):
        if getattr(self, "_h", None):
            try:
                getattr(lib(), self._destroy)(self._h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class KnnIvf(_KnnIndex):
    """IVF-Flat index over a Features table (glx_knn_ivf): centroids and inverted lists on the device, scores from the
    table itself.  search(..., nprobe=nlist) equals Features.search bit for bit; with fewer lists probed it equals the
    exact search restricted to the probed lists' rows."""
    _destroy = "glx_knn_ivf_destroy"

    def __init__(self, features, nlist, niter=10, train_rows=None, centroids=None):
        self._h = None
        nlist, niter = int(nlist), int(niter)
        if centroids is not None and (centroids.ndim != 2 or tuple(centroids.shape) != (nlist, features.dim)):
            raise ValueError("centroids must be [{}, {}], not {}".format(nlist, features.dim, tuple(centroids.shape)))
        if _is_torch(centroids):
            import torch
            assert centroids.dtype == torch.float32, centroids.dtype
        pc = _ptr(centroids, None if _is_torch(centroids) else np.float32)
        kind = PTR_HOST if pc[1] is None else pc[1]
        h = ctypes.c_void_p()
        _check(lib().glx_knn_ivf_build(features._h, nlist, niter, 0 if train_rows is None else int(train_rows), pc[0],
                                       kind, _stream(kind, features.device), ctypes.byref(h)))
        self._h = h
        self.features = features  # the lists index its rows: keep it alive
        self.device = features.device
        self.nlist, self.dim, self.num_rows = nlist, features.dim, features.num_rows

    def info(self):
        """-> dict(nlist, dim, num_rows, longest_list, device_bytes)"""
        nl, d = ctypes.c_int32(), ctypes.c_int32()
        n, longest, nbytes = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _check(lib().glx_knn_ivf_info(self._h, ctypes.byref(nl), ctypes.byref(d), ctypes.byref(n), ctypes.byref(longest),
                                      ctypes.byref(nbytes)))
        return {"nlist": nl.value, "dim": d.value, "num_rows": n.value, "longest_list": longest.value,
                "device_bytes": nbytes.value}

    def centroids(self):
        """-> centroids[nlist, D] float32 (numpy)"""
        out = np.empty((self.nlist, self.dim), np.float32)
        _check(lib().glx_knn_ivf_export(self._h, _ptr(out)[0], None, None, PTR_HOST, None))
        return out

    def lists(self):
        """-> (list_ptr[nlist + 1], list_rows[num_rows]) int64 (numpy): list l holds the storage rows
        list_rows[list_ptr[l]:list_ptr[l + 1]], ascending"""
        ptr, rows = np.empty(self.nlist + 1, np.int64), np.empty(self.num_rows, np.int64)
        _check(lib().glx_knn_ivf_export(self._h, None, _ptr(ptr)[0], _ptr(rows)[0], PTR_HOST, None))
        return ptr, rows

    def search(self, queries, k, metric="ip", nprobe=1, out=None):
        """The k best rows of every query among the rows of its nprobe best lists (glx_knn_ivf_search) ->
        (ids[n, k] int64, dist[n, k] float32), best first, under Features.search's contract: the same chain, order, ids
        and padding (slots beyond the probed lists' rows hold id -1).  nprobe == nlist probes every list and equals
        Features.search bit for bit; otherwise 1 <= nprobe <= min(nlist, 1024).  Numpy in, numpy out; torch CUDA tensors
        in, torch CUDA tensors out on the current stream, nothing read back.  out=(ids, dist): buffers to write into."""
        return _knn_search(lib().glx_knn_ivf_search, lambda: self._h, self.dim, self.device, queries, k, metric, out,
                           int(nprobe))

    def build_pq(self, m, niter=10, train_rows=None, codebooks=None):
        """An IVF-PQ index on top of this index (glx_knn_ivfpq_build) -> KnnIvfPq: m sub-quantisers of 256 codewords
        over the rows' residuals (dim % m == 0, 1 <= m <= 64, num_rows >= 256), trained by niter Lloyd iterations over
        a sample of train_rows rows (None: min(num_rows, 65536)), starting from codebooks[m, 256, dim / m] float32
        (numpy or a torch CUDA tensor) when given; niter=0 with codebooks only encodes.  The build is deterministic.
        The returned index keeps this one alive."""
        return KnnIvfPq(self, m, niter, train_rows, codebooks)


class KnnIvfPq(_KnnIndex):
    """IVF-PQ index on top of a KnnIvf (glx_knn_ivfpq): m codebooks and one m-byte code per row on the device.
    search(..., refine=0) ranks the probed lists' rows by the coded (ADC) score; refine=R re-scores the R best of them
    from the table itself, so every returned distance is Features.search's distance of that row."""
    _destroy = "glx_knn_ivfpq_destroy"

    def __init__(self, ivf, m, niter=10, train_rows=None, codebooks=None):
        self._h = None
        m, niter = int(m), int(niter)
        dsub = ivf.dim // m if m > 0 and ivf.dim % m == 0 else None
        if codebooks is not None and (dsub is None or tuple(codebooks.shape) != (m, 256, dsub)):
            raise ValueError("codebooks must be [m, 256, dim / m] = [{}, 256, {}], not {}".format(
                m, dsub, tuple(codebooks.shape)))
        if _is_torch(codebooks):
            import torch
            assert codebooks.dtype == torch.float32, codebooks.dtype
        if not getattr(ivf, "_h", None):
            raise ValueError("the IVF index is closed")
        pc = _ptr(codebooks, None if _is_torch(codebooks) else np.float32)
        kind = PTR_HOST if pc[1] is None else pc[1]
        h = ctypes.c_void_p()
        _check(lib().glx_knn_ivfpq_build(ivf._h, m, niter, 0 if train_rows is None else int(train_rows), pc[0], kind,
                                         _stream(kind, ivf.device), ctypes.byref(h)))
        self._h = h
        self.ivf = ivf  # the codes follow its lists: keep it (and through it the table) alive
        self.device = ivf.device
        self.m, self.dsub, self.dim, self.num_rows = m, dsub, ivf.dim, ivf.num_rows

    def _handle(self):
        if not self._h or not self.ivf._h:
            raise ValueError("the index is closed")
        return self._h

    def info(self):
        """-> dict(m, dsub, num_rows, device_bytes)"""
        m, d = ctypes.c_int32(), ctypes.c_int32()
        n, nbytes = ctypes.c_int64(), ctypes.c_int64()
        _check(lib().glx_knn_ivfpq_info(self._handle(), ctypes.byref(m), ctypes.byref(d), ctypes.byref(n),
                                        ctypes.byref(nbytes)))
        return {"m": m.value, "dsub": d.value, "num_rows": n.value, "device_bytes": nbytes.value}

    def codebooks(self):
        """-> codebooks[m, 256, dsub] float32 (numpy)"""
        out = np.empty((self.m, 256, self.dsub), np.float32)
        _check(lib().glx_knn_ivfpq_export(self._handle(), _ptr(out)[0], None, PTR_HOST, None))
        return out

    def codes(self):
        """-> codes[num_rows, m] uint8 (numpy) in list order: row p is the code of storage row ivf.lists()[1][p]"""
        out = np.empty((self.num_rows, self.m), np.uint8)
        _check(lib().glx_knn_ivfpq_export(self._handle(), None, _ptr(out)[0], PTR_HOST, None))
        return out

    def search(self, queries, k, metric="ip", nprobe=1, refine=0, out=None):
        """The k best rows of every query among the rows of its nprobe best lists (glx_knn_ivfpq_search) ->
        (ids[n, k] int64, dist[n, k] float32), best first; the probe sets, ids and padding are KnnIvf.search's.
        refine=0: ranked by the coded (ADC) score, which dist holds.  k <= refine <= 1024: the refine best by that score
        are re-scored from the table and the k best of those returned, dist being Features.search's distance of the row
        bit for bit.  Numpy in, numpy out; torch CUDA tensors in, torch CUDA tensors out on the current stream, nothing
        read back.  out=(ids, dist): buffers to write into."""
        return _knn_search(lib().glx_knn_ivfpq_search, self._handle, self.dim, self.device, queries, k, metric, out,
                           int(nprobe), int(refine))


def _knn_search(call, handle, dim, device, queries, k, metric, out, *extra):
    """The three search methods: call(handle(), metric, queries, n, k, *extra, ids, dist, ptr kind, stream)."""
    if metric not in KNN_METRICS:
        raise ValueError("metric must be one of {}, not {!r}".format(sorted(KNN_METRICS), metric))
    if queries.ndim != 2 or int(queries.shape[1]) != dim:
        raise ValueError("queries must be [n, {}], not {}".format(dim, tuple(queries.shape)))
    n, k = int(queries.shape[0]), int(k)
    ids, dist = _knn_out(out, queries, n, k)
    pq, pi, pd = _ptr(queries, None if _is_torch(queries) else np.float32), _ptr(ids), _ptr(dist)
    kind = _kind(pq, pi, pd)
    _check(call(handle(), KNN_METRICS[metric], pq[0], n, k, *extra, pi[0], pd[0], kind, _stream(kind, device)))
    return ids, dist


def _knn_out(out, like, n, k):
    if out is not None:
        ids, dist = out
        for name, buf, dtype in (("ids", ids, "int64"), ("dist", dist, "float32")):
            if tuple(buf.shape) != (n, k) or str(buf.dtype).replace("torch.", "") != dtype:
                raise ValueError("knn: out's {} must be {} of shape {}, not {} of shape {}".format(
                    name, dtype, (n, k), buf.dtype, tuple(buf.shape)))
        return ids, dist
    if _is_torch(like):
        import torch
        assert like.dtype == torch.float32, like.dtype
        return (torch.empty((n, k), dtype=torch.int64, device=like.device),
                torch.empty((n, k), dtype=torch.float32, device=like.device))
    return np.empty((n, k), np.int64), np.empty((n, k), np.float32)


def knn_merge(ids, dist, metric="ip", out=None, device=0):
    """The k best of several search results per query (glx_knn_merge): ids / dist [num_parts, n, k] -> ([n, k], [n, k]).
    Same order as Features.search on dist; ties go to the lower part, then to the earlier position; id -1 entries are
    absent.  Merging the searches of consecutive row ranges of one table equals the whole-table search bit for bit."""
    if metric not in KNN_METRICS:
        raise ValueError("metric must be one of {}, not {!r}".format(sorted(KNN_METRICS), metric))
    if ids.ndim != 3 or tuple(ids.shape) != tuple(dist.shape):
        raise ValueError("ids and dist must both be [num_parts, n, k]")
    parts, n, k = (int(v) for v in ids.shape)
    oi, od = _knn_out(out, dist, n, k)
    pi, pd, poi, pod = _ptr(ids, None if _is_torch(ids) else np.int64), _ptr(dist, None if _is_torch(dist) else np.float32), _ptr(oi), _ptr(od)
    kind = _kind(pi, pd, poi, pod)
    if kind == PTR_DEVICE:
        device = od.device.index or 0
    _check(lib().glx_knn_merge(device, KNN_METRICS[metric], parts, pi[0], pd[0], n, k, poi[0], pod[0], kind,
                               _stream(kind, device)))
    return oi, od


# The [rows, D] matrices of the training path hold float32 or bfloat16 (the _ex entry points of include/glx.h).
TRAIN_DTYPES = {"float32": FEATURE_DTYPES["float32"], "bfloat16": FEATURE_DTYPES["bfloat16"]}


def _train_buf(x, what):
    """(buffer for _ptr, dtype name) of a float32 / bfloat16 matrix of the training path: a torch CUDA tensor as it is,
    a host torch tensor as a numpy view of its memory, a numpy float32 array, or a numpy uint16 / int16 array of
    bfloat16 codes (numpy has no bfloat16).  Anything else raises ValueError before the call."""
    if _is_torch(x):
        name = str(x.dtype).replace("torch.", "")
        if name not in TRAIN_DTYPES:
            raise ValueError("{} must be float32 or bfloat16, not {}: bfloat16 is the half type that has a gradient "
                             "contract (float16 gradients need loss scaling)".format(what, x.dtype))
        if not x.is_cuda:
            import torch
            assert x.is_contiguous(), "host tensors must be contiguous"
            x = x.numpy() if name == "float32" else x.view(torch.int16).numpy()
        return x, name
    if isinstance(x, np.ndarray) and x.dtype == np.float32:
        return x, "float32"
    if isinstance(x, np.ndarray) and x.dtype in (np.uint16, np.int16):
        return x, "bfloat16"
    raise ValueError("{} must be float32 or bfloat16 (numpy: uint16 / int16 codes), not {}".format(
        what, getattr(x, "dtype", type(x))))


def _train_out(out, out_dtype, like, shape, what):
    """the row gradient of a call: (what to return, buffer for _ptr, dtype name) -- `out` in its own dtype, or a new
    buffer of `like`'s kind holding out_dtype elements (torch: a bfloat16 tensor; numpy: the uint16 codes)"""
    if out is not None:
        buf, name = _train_buf(out, what)
        return out, buf, name
    if out_dtype not in TRAIN_DTYPES:
        raise ValueError("{} holds float32 or bfloat16, not {!r}".format(what, out_dtype))
    if _is_torch(like):
        import torch
        res = torch.empty(shape, dtype=getattr(torch, out_dtype), device=like.device)
    else:
        res = np.empty(shape, np.float32 if out_dtype == "float32" else np.uint16)
    return res, res, out_dtype


def aggregate_backward(op, rows, cnt, grad_out, num_rows, arg=None, out=None, device=0, out_dtype="float32",
                       chunked=False):
    """Gradient of Features.aggregate with respect to the rows of a [num_rows, D] table with dense ids
    (glx_aggregate_backward_ex) -> grad_x[num_rows, D], every row written (rows nobody references: zeros).
    rows[n] int64: the request's ids; cnt[num_segments] int32: the counts the forward returned (None: the implied
    layout of n // num_segments positions per segment); grad_out[num_segments, D] float32; arg: Max / Min only, what
    Features.aggregate_arg recorded.  Each element adds its terms in float32 in ascending request position and no float
    atomic is used: the same inputs give the same bits on every run.  Prod raises (its gradient divides by the element).
    out_dtype "float32" or "bfloat16" (out=: the buffer's own dtype): a bfloat16 grad_x is the float32 gradient rounded
    once per element, to nearest even (a torch bfloat16 tensor on the device, numpy uint16 codes on the host).
    chunked=True (glx_aggregate_backward_chunked) sums the same terms in the CHUNKED order instead: a row's list of
    positions is cut into chunks of COALESCE_CHUNK (256) entries -- entries, whether a Max / Min arg selects them or
    not -- each chunk is summed from +0.0 in ascending position by its own lane group, and the row is +0.0 plus the
    partial sums in ascending chunk.  A row referenced at most 256 times gets the default bits; Sum equals rows_coalesce
    of the gathered grad_out rows; still no atomics and the same bits on every call, a bfloat16 grad_x still rounded
    once.  For requests in which a few hub rows take a large share of the positions.
    Torch CUDA tensors are device pointers on the current stream, numpy arrays host pointers."""
    if isinstance(op, str):
        op = AGGREGATOR_IDS[op]
    n = int(rows.shape[0])
    num_segments, dim = int(grad_out.shape[0]), int(grad_out.shape[1])
    grad_x, buf, name = _train_out(out, out_dtype, grad_out, (num_rows, dim), "aggregate_backward: grad_x")
    pr, pc, pa, pg, px = _ptr(rows), _ptr(cnt), _ptr(arg), _ptr(grad_out), _ptr(buf)
    kind = _kind(pr, pc, pa, pg, px)
    if kind == PTR_DEVICE:
        device = grad_x.device.index or 0
    entry = lib().glx_aggregate_backward_chunked if chunked else lib().glx_aggregate_backward_ex
    _check(entry(device, op, pr[0], pc[0], pa[0], n, num_segments, num_rows, dim, pg[0], px[0], TRAIN_DTYPES[name], kind,
                 _stream(kind, device)))
    return grad_x


def _weighted_out(out, like, shape):
    """the float32 output of a weighted-aggregation call: `out`, or a new buffer of `like`'s kind"""
    if out is not None:
        return out
    if _is_torch(like):
        import torch
        return torch.empty(shape, dtype=torch.float32, device=like.device)
    return np.empty(shape, np.float32)


def _weighted_heads(w, n):
    """heads of a weight buffer w[n] or w[n, heads]"""
    assert int(w.shape[0]) == n, "one weight row per position"
    return 1 if len(w.shape) == 1 else int(w.shape[1])


def aggregate_weighted(op, x, rows, w, num_segments, cnt=None, default_attr=0.0, out=None, device=0):
    """Weighted Sum / Mean over segments of gathered rows (glx_aggregate_weighted) -> emb[num_segments, D] float32.
    x[num_rows, D] float32; rows[n] int64 (a value outside [0, num_rows) reads a row of default_attr); w[n] or
    w[n, heads] float32, column c belongs to head c // (D // heads); cnt[num_segments] int32 (None: the implied layout
    of n // num_segments positions per segment).  Every element folds fadd(acc, fmul(w, x)) left to right: bit-exact,
    and with all-ones weights equal to Features(x, view=True).aggregate.  Max / Min / Prod raise.
    x may hold bfloat16 (a torch bfloat16 tensor, or numpy uint16 / int16 codes): emb stays float32 and equals the call
    on the float32 matrix of x's values bit for bit.  Any other dtype raises ValueError.
    Torch CUDA tensors are device pointers on the current stream, numpy arrays host pointers."""
    if isinstance(op, str):
        op = AGGREGATOR_IDS[op]
    n = int(rows.shape[0])
    num_rows, dim = int(x.shape[0]), int(x.shape[1])
    heads = _weighted_heads(w, n)
    xb, x_dtype = _train_buf(x, "aggregate_weighted: x")
    emb = _weighted_out(out, xb, (num_segments, dim))
    px, pr, pw, pc, pe = _ptr(xb), _ptr(rows), _ptr(w), _ptr(cnt), _ptr(emb)
    kind = _kind(px, pr, pw, pc, pe)
    if kind == PTR_DEVICE:
        device = emb.device.index or 0
    _check(lib().glx_aggregate_weighted_ex(device, op, px[0], TRAIN_DTYPES[x_dtype], num_rows, dim, pr[0], pw[0], heads,
                                           pc[0], n, num_segments, default_attr, pe[0], kind, _stream(kind, device)))
    return emb


def aggregate_weighted_backward_x(op, rows, w, cnt, grad_out, num_rows, out=None, device=0, out_dtype="float32",
                                  chunked=False):
    """Gradient of aggregate_weighted with respect to the rows (glx_aggregate_weighted_backward_x_ex) ->
    grad_x[num_rows, D], every row written.  aggregate_backward's contract with one more factor: each element adds
    fmul(w[p, head], term) in float32 in ascending request position, no float atomic: the same bits on every run.
    out_dtype / out= as in aggregate_backward: a bfloat16 grad_x is the float32 gradient rounded once per element.
    chunked=True (glx_aggregate_weighted_backward_x_chunked): aggregate_backward's chunked order over the same
    two-rounding terms -- chunks of 256 list entries summed apart, partial sums added in chunk order; a row referenced
    at most 256 times gets the default bits."""
    if isinstance(op, str):
        op = AGGREGATOR_IDS[op]
    n = int(rows.shape[0])
    num_segments, dim = int(grad_out.shape[0]), int(grad_out.shape[1])
    heads = _weighted_heads(w, n)
    grad_x, buf, name = _train_out(out, out_dtype, grad_out, (num_rows, dim), "aggregate_weighted_backward_x: grad_x")
    pr, pw, pc, pg, px = _ptr(rows), _ptr(w), _ptr(cnt), _ptr(grad_out), _ptr(buf)
    kind = _kind(pr, pw, pc, pg, px)
    if kind == PTR_DEVICE:
        device = grad_x.device.index or 0
    entry = lib().glx_aggregate_weighted_backward_x_chunked if chunked else lib().glx_aggregate_weighted_backward_x_ex
    _check(entry(device, op, pr[0], pw[0], heads, pc[0], n, num_segments, num_rows, dim, pg[0], px[0],
                 TRAIN_DTYPES[name], kind, _stream(kind, device)))
    return grad_x


def aggregate_weighted_backward_w(op, x, rows, heads, cnt, grad_out, default_attr=0.0, out=None, device=0):
    """Gradient of aggregate_weighted with respect to the weights (glx_aggregate_weighted_backward_w) ->
    grad_w[n, heads] float32, every element written (a position that was not consumed: +0.0).  grad_w[p, h] is the dot
    product of grad_out[s(p)] and the gathered row over the columns of head h (Mean: / count); a fixed lane mapping
    and reduction tree, no atomics: the same bits on every run, within C * 2^-23 * sum|terms| of the exact value.
    x may hold bfloat16, as in aggregate_weighted: grad_w stays float32 and equals the call on the float32 matrix of
    x's values bit for bit (the same mapping and tree)."""
    if isinstance(op, str):
        op = AGGREGATOR_IDS[op]
    n = int(rows.shape[0])
    num_rows, dim = int(x.shape[0]), int(x.shape[1])
    num_segments = int(grad_out.shape[0])
    assert int(grad_out.shape[1]) == dim
    xb, x_dtype = _train_buf(x, "aggregate_weighted_backward_w: x")
    grad_w = _weighted_out(out, grad_out, (n, heads))
    px, pr, pc, pg, pw = _ptr(xb), _ptr(rows), _ptr(cnt), _ptr(grad_out), _ptr(grad_w)
    kind = _kind(px, pr, pc, pg, pw)
    if kind == PTR_DEVICE:
        device = grad_w.device.index or 0
    _check(lib().glx_aggregate_weighted_backward_w_ex(device, op, px[0], TRAIN_DTYPES[x_dtype], num_rows, dim, pr[0],
                                                      heads, pc[0], n, num_segments, default_attr, pg[0], pw[0], kind,
                                                      _stream(kind, device)))
    return grad_w


def segment_softmax(e, num_segments, cnt=None, out=None, device=0):
    """Softmax of the logits e[n] or e[n, heads] float32 over the segments of a request, per head
    (glx_segment_softmax) -> alpha of e's shape.  cnt[num_segments] int32: aggregate_weighted's layout (None: the
    implied layout of n // num_segments positions per segment).  Every element is written, a position that is not
    consumed is +0.0; a column with a NaN or +inf logit, or only -inf ones, is NaN.  No atomics: the same bits on every
    call.  Torch CUDA tensors are device pointers on the current stream, numpy arrays host pointers."""
    n = int(e.shape[0])
    heads = _weighted_heads(e, n)
    alpha = _weighted_out(out, e, tuple(e.shape))
    pe, pc, pa = _ptr(e), _ptr(cnt), _ptr(alpha)
    kind = _kind(pe, pc, pa)
    if kind == PTR_DEVICE:
        device = alpha.device.index or 0
    _check(lib().glx_segment_softmax(device, pe[0], heads, pc[0], n, num_segments, pa[0], kind, _stream(kind, device)))
    return alpha


def segment_softmax_backward(alpha, grad_alpha, cnt, num_segments, out=None, device=0):
    """Gradient of segment_softmax with respect to the logits (glx_segment_softmax_backward) -> grad_e of alpha's
    shape: alpha * (grad_alpha - sum over the segment of alpha * grad_alpha), from the forward's own output.  Every
    element is written, a position that is not consumed is +0.0; a fixed reduction tree, no atomics: the same bits on
    every call."""
    n = int(alpha.shape[0])
    heads = _weighted_heads(alpha, n)
    assert tuple(grad_alpha.shape) == tuple(alpha.shape), "grad_alpha must have alpha's shape"
    grad_e = _weighted_out(out, alpha, tuple(alpha.shape))
    pa, pg, pc, po = _ptr(alpha), _ptr(grad_alpha), _ptr(cnt), _ptr(grad_e)
    kind = _kind(pa, pg, pc, po)
    if kind == PTR_DEVICE:
        device = grad_e.device.index or 0
    _check(lib().glx_segment_softmax_backward(device, pa[0], pg[0], heads, pc[0], n, num_segments, po[0], kind,
                                              _stream(kind, device)))
    return grad_e


def _gat_shapes(s, t, rows):
    """(n, num_segments, num_rows, heads) of a gat_attention request: s[S] or s[S, heads], t[M] or t[M, heads]"""
    heads = 1 if len(s.shape) == 1 else int(s.shape[1])
    assert (1 if len(t.shape) == 1 else int(t.shape[1])) == heads, "s and t must have the same number of heads"
    return int(rows.shape[0]), int(s.shape[0]), int(t.shape[0]), heads


def gat_attention(s, t, rows, cnt=None, negative_slope=0.2, default_attr=0.0, drop_p=0.0, seed=0, call=0,
                  want_soft=True, out=None, soft_out=None, device=0):
    """The attention coefficients of a GAT layer in one launch (glx_gat_attention) -> (alpha, soft), both [n, heads]
    float32: the logit leaky_relu(s[segment, h] + t[rows[p], h]) of every position and head, its softmax over each
    segment (`soft`, glx_segment_softmax's definition) and dropout on it (`alpha`: a kept element is soft / (1 - drop_p),
    a dropped one +0.0; the mask is a pure function of (seed, call, p, h)).  s[S] or s[S, heads], t[M] or t[M, heads]
    float32, rows[n] int64 (a value outside [0, M) reads default_attr: -inf masks the position), cnt[S] int32 (None: the
    implied layout of n // S positions per segment).  want_soft=False with drop_p == 0 skips the second output (soft
    is then None; alpha is it).  No atomics: the same bits on every call.  Torch CUDA tensors are device pointers on
    the current stream, numpy arrays host pointers."""
    n, num_segments, num_rows, heads = _gat_shapes(s, t, rows)
    alpha = _weighted_out(out, s, (n, heads))
    soft = soft_out
    if soft is None and (want_soft or drop_p != 0.0):
        soft = _weighted_out(None, s, (n, heads))
    ps, pt, pr, pc, pso, pa = _ptr(s), _ptr(t), _ptr(rows), _ptr(cnt), _ptr(soft), _ptr(alpha)
    kind = _kind(ps, pt, pr, pc, pso, pa)
    if kind == PTR_DEVICE:
        device = alpha.device.index or 0
    _check(lib().glx_gat_attention(device, ps[0], pt[0], num_rows, pr[0], heads, pc[0], n, num_segments, negative_slope,
                                   default_attr, drop_p, seed, call, pso[0], pa[0], kind, _stream(kind, device)))
    return alpha, soft


def gat_attention_backward(soft, grad_alpha, s, t, rows, cnt=None, negative_slope=0.2, default_attr=0.0, drop_p=0.0,
                           seed=0, call=0, want_s=True, want_t=True, out=None, out_s=None, out_t=None, device=0):
    """Gradients of gat_attention (glx_gat_attention_backward) -> (grad_e[n, heads], grad_s[S, heads] or None,
    grad_t[M, heads] or None) from the forward's `soft`, the gradient of its `alpha` and the forward's own arguments
    (the dropout mask is recomputed from seed and call).  grad_e is the gradient of the logits before leaky_relu;
    grad_s sums it per segment (a fixed tree), grad_t per row of t in ascending position (the bits of
    aggregate_backward(SUM, rows, None, grad_e, M)).  Every element is written; no atomics: the same bits on every
    call.  want_s / want_t = False skips that gradient."""
    n, num_segments, num_rows, heads = _gat_shapes(s, t, rows)
    grad_e = _weighted_out(out, soft, (n, heads))
    grad_s = _weighted_out(out_s, soft, (num_segments, heads)) if (want_s or out_s is not None) else None
    grad_t = _weighted_out(out_t, soft, (num_rows, heads)) if (want_t or out_t is not None) else None
    pso, pg, ps, pt, pr, pc = _ptr(soft), _ptr(grad_alpha), _ptr(s), _ptr(t), _ptr(rows), _ptr(cnt)
    pe, pgs, pgt = _ptr(grad_e), _ptr(grad_s), _ptr(grad_t)
    kind = _kind(pso, pg, ps, pt, pr, pc, pe, pgs, pgt)
    if kind == PTR_DEVICE:
        device = grad_e.device.index or 0
    _check(lib().glx_gat_attention_backward(device, pso[0], pg[0], ps[0], pt[0], num_rows, pr[0], heads, pc[0], n,
                                            num_segments, negative_slope, default_attr, drop_p, seed, call, pe[0],
                                            pgs[0], pgt[0], kind, _stream(kind, device)))
    return grad_e, grad_s, grad_t


def _dot_shapes(q, k, v, rows, edge, heads):
    """(n, num_segments, num_rows, dim) of a dot_attention request"""
    n, dim = int(rows.shape[0]), int(q.shape[1])
    assert int(k.shape[1]) == dim and tuple(v.shape) == tuple(k.shape), "q, k and v must have the same columns"
    assert edge is None or tuple(edge.shape) == (n, dim), "edge must be [n, D]"
    assert heads >= 1 and dim % heads == 0, "heads must divide D"
    return n, int(q.shape[0]), int(k.shape[0]), dim


def _same_table(k, v):
    """is v the very buffer of k (one table serving as key and value)"""
    if k is v:
        return True
    if _is_torch(k) and _is_torch(v):
        return k.data_ptr() == v.data_ptr()
    return isinstance(k, np.ndarray) and isinstance(v, np.ndarray) and k.ctypes.data == v.ctypes.data


def dot_attention(q, k, v, rows, cnt=None, edge=None, heads=1, scale=None, default_attr=0.0, drop_p=0.0, seed=0, call=0,
                  want_logit=False, out=None, soft_out=None, logit_out=None, device=0, chunked=False):
    """Scaled dot-product attention of every segment over its positions, with an edge term on the key and on the value
    (glx_dot_attention) -> (out[S, D], soft[n, heads], logit[n, heads] or None), float32.  q[S, D] one query per
    segment; k, v[M, D] (they may be one buffer); rows[n] int64 (a value outside [0, M) reads a row of default_attr in
    both tables); edge[n, D] or None; cnt[S] int32 (None: the implied layout of n // S positions per segment); column c
    belongs to head c // (D // heads).  logit = (q . (k[rows] + edge)) * scale per head (scale None: 1 / sqrt(D // heads)
    rounded to float32), soft its softmax over each segment (glx_segment_softmax's definition), alpha gat_attention's
    dropout of soft under (seed, call), out the sum of alpha * (v[rows] + edge) in ascending position: bit-exact from
    soft, an empty segment is +0.0.  No atomics: the same bits on every call.  Torch CUDA tensors are device pointers
    on the current stream, numpy arrays host pointers.
    chunked=True (glx_dot_attention_chunked) is the CHUNKED order, for requests with hub segments: a segment of more
    than 256 positions is cut into chunks of 256, its softmax runs in a fixed tree over one workgroup (the same
    definition, rules and bound; other bits) and its `out` adds each chunk from +0.0 in ascending position, then the
    partial sums in chunk order.  logit has the default's bits everywhere, and so has every output of a segment of at
    most 256 positions; as deterministic as the default."""
    n, num_segments, num_rows, dim = _dot_shapes(q, k, v, rows, edge, heads)
    if scale is None:
        scale = float(np.float32(1.0) / np.sqrt(np.float32(dim // heads)))
    res = _weighted_out(out, q, (num_segments, dim))
    soft = _weighted_out(soft_out, q, (n, heads))
    logit = _weighted_out(logit_out, q, (n, heads)) if (want_logit or logit_out is not None) else None
    pq, pk, pr, pe, pc = _ptr(q), _ptr(k), _ptr(rows), _ptr(edge), _ptr(cnt)
    pv = pk if _same_table(k, v) else _ptr(v)
    pl, ps, po = _ptr(logit), _ptr(soft), _ptr(res)
    kind = _kind(pq, pk, pv, pr, pe, pc, pl, ps, po)
    if kind == PTR_DEVICE:
        device = res.device.index or 0
    entry = lib().glx_dot_attention_chunked if chunked else lib().glx_dot_attention
    _check(entry(device, pq[0], pk[0], pv[0], num_rows, dim, heads, pr[0], pe[0], pc[0], n, num_segments, scale,
                 default_attr, drop_p, seed, call, pl[0], ps[0], po[0], kind, _stream(kind, device)))
    return res, soft, logit


def dot_attention_backward(soft, grad_out, q, k, v, rows, cnt=None, edge=None, heads=1, scale=None, default_attr=0.0,
                           drop_p=0.0, seed=0, call=0, want_q=True, want_k=True, want_v=True, want_edge=True, out=None,
                           out_q=None, out_k=None, out_v=None, out_edge=None, device=0, chunked=False):
    """Gradients of dot_attention (glx_dot_attention_backward) -> (grad_e[n, heads], grad_q[S, D], grad_k[M, D],
    grad_v[M, D], grad_edge[n, D]; None for a gradient that was not asked for, and grad_edge is None without edge) from
    the forward's `soft`, the gradient of its `out` and the forward's own arguments (alpha and the dropout mask are
    recomputed from soft, seed and call).  grad_e is the gradient of the logits; grad_q and grad_edge are bit-exact
    folds of it, grad_k and grad_v the bits of aggregate_weighted_backward_x(SUM, rows, grad_e, cnt, q, M) and of
    aggregate_weighted_backward_x(SUM, rows, alpha, cnt, grad_out, M) on one transpose.  Every element is written; no
    atomics: the same bits on every call.
    chunked=True (glx_dot_attention_backward_chunked) is dot_attention's CHUNKED order going back: the softmax gradient
    of a segment of more than 256 positions runs over one workgroup, its grad_q is summed chunk by chunk (each chunk of
    256 positions from +0.0, the partial sums in chunk order), and grad_k / grad_v are the bits of
    aggregate_weighted_backward_x(..., chunked=True).  A request without such segments and without rows named more than
    256 times gets the default's bits in every output."""
    n, num_segments, num_rows, dim = _dot_shapes(q, k, v, rows, edge, heads)
    if scale is None:
        scale = float(np.float32(1.0) / np.sqrt(np.float32(dim // heads)))
    grad_e = _weighted_out(out, soft, (n, heads))
    grad_q = _weighted_out(out_q, soft, (num_segments, dim)) if (want_q or out_q is not None) else None
    grad_k = _weighted_out(out_k, soft, (num_rows, dim)) if (want_k or out_k is not None) else None
    grad_v = _weighted_out(out_v, soft, (num_rows, dim)) if (want_v or out_v is not None) else None
    grad_edge = None
    if edge is not None and (want_edge or out_edge is not None):
        grad_edge = _weighted_out(out_edge, soft, (n, dim))
    pq, pk, pr, pe, pc = _ptr(q), _ptr(k), _ptr(rows), _ptr(edge), _ptr(cnt)
    pv = pk if _same_table(k, v) else _ptr(v)
    pso, pg = _ptr(soft), _ptr(grad_out)
    pge, pgq, pgk, pgv, pged = _ptr(grad_e), _ptr(grad_q), _ptr(grad_k), _ptr(grad_v), _ptr(grad_edge)
    kind = _kind(pq, pk, pv, pr, pe, pc, pso, pg, pge, pgq, pgk, pgv, pged)
    if kind == PTR_DEVICE:
        device = grad_e.device.index or 0
    entry = lib().glx_dot_attention_backward_chunked if chunked else lib().glx_dot_attention_backward
    _check(entry(device, pq[0], pk[0], pv[0], num_rows, dim, heads, pr[0], pe[0], pc[0], n, num_segments, scale,
                 default_attr, drop_p, seed, call, pso[0], pg[0], pge[0], pgq[0], pgk[0], pgv[0], pged[0], kind,
                 _stream(kind, device)))
    return grad_e, grad_q, grad_k, grad_v, grad_edge


def _pair_counts(ia, ib, repeat):
    """(num_pairs, repeat) of a pair request; ia has one entry per `repeat` entries of ib"""
    n, repeat = int(np.prod(ib.shape)), int(repeat)
    assert repeat >= 1 and int(np.prod(ia.shape)) * repeat == n, "ia needs one entry per `repeat` entries of ib"
    return n, repeat


def pair_dot(xa, ia, xb, ib, heads=1, repeat=1, default_attr=0.0, out=None, device=0):
    """Per-pair, per-head dot products of gathered rows (glx_pair_dot) -> out[n, heads] float32, n = ib's size.
    xa[Na, D], xb[Nb, D] float32 (they may be one table); ib[n] int64 and ia[n // repeat] int64: pair p joins row
    ia[p // repeat] of xa with row ib[p] of xb (repeat = K: a [B, K] negative-sampler response against its B sources);
    an index outside its table reads a row of default_attr; column c belongs to head c // (D // heads).  A fixed lane
    mapping and reduction tree, no atomics: the same bits on every call, within (D // heads) * 2^-23 * sum|terms| of
    the exact value.  xa and xb may both hold bfloat16 (torch bfloat16 tensors, or numpy uint16 / int16 codes): out stays
    float32 and equals the call on the float32 tables of their values bit for bit; tables of two different dtypes, or of
    any other dtype, raise ValueError.
    Torch CUDA tensors are device pointers on the current stream, numpy arrays host pointers."""
    n, repeat = _pair_counts(ia, ib, repeat)
    num_rows_a, dim = int(xa.shape[0]), int(xa.shape[1])
    num_rows_b = int(xb.shape[0])
    assert int(xb.shape[1]) == dim, "xa and xb must have the same number of columns"
    xa_buf, a_dtype = _train_buf(xa, "pair_dot: xa")
    xb_buf, b_dtype = _train_buf(xb, "pair_dot: xb")
    if a_dtype != b_dtype:
        raise ValueError("pair_dot: xa holds {} and xb {}: both tables must have one dtype".format(a_dtype, b_dtype))
    res = _weighted_out(out, xa_buf, (n, heads))
    pa, pia, pb, pib, po = _ptr(xa_buf), _ptr(ia), _ptr(xb_buf), _ptr(ib), _ptr(res)
    kind = _kind(pa, pia, pb, pib, po)
    if kind == PTR_DEVICE:
        device = res.device.index or 0
    _check(lib().glx_pair_dot_ex(device, pa[0], num_rows_a, pb[0], num_rows_b, TRAIN_DTYPES[a_dtype], dim, heads, pia[0],
                                 pib[0], n, repeat, default_attr, po[0], kind, _stream(kind, device)))
    return res


def pair_dot_backward(side, ia, ib, g, x_other, num_rows_self, repeat=1, default_attr=0.0, out=None, device=0):
    """Gradient of pair_dot with respect to xa (side 0) or xb (side 1) (glx_pair_dot_backward) ->
    grad_self[num_rows_self, D] float32, every row written.  g[n, heads] (or g[n]) is the gradient of pair_dot's output,
    x_other the other side's table.  Each element adds fmul(g[p, head], other_row(p)) over the pairs that refer to its
    row in ascending p, no float atomic: the same bits on every run.  An own index outside the table gets nothing, an
    other-side index outside its table multiplies a row of default_attr.
    grad_self takes x_other's dtype: for a bfloat16 x_other it is the float32 gradient (summed in float32 over the exactly
    upcast rows) rounded once per element, to nearest even; an out= of another dtype raises ValueError."""
    n, repeat = _pair_counts(ia, ib, repeat)
    heads = _weighted_heads(g, n)
    num_rows_other, dim = int(x_other.shape[0]), int(x_other.shape[1])
    xo, x_dtype = _train_buf(x_other, "pair_dot_backward: x_other")
    grad, buf, name = _train_out(out, x_dtype, xo, (num_rows_self, dim), "pair_dot_backward: grad_self")
    if name != x_dtype:
        raise ValueError("pair_dot_backward: grad_self holds {} and x_other {}: both must have one dtype".format(
            name, x_dtype))
    pia, pib, pg, px, po = _ptr(ia), _ptr(ib), _ptr(g), _ptr(xo), _ptr(buf)
    kind = _kind(pia, pib, pg, px, po)
    if kind == PTR_DEVICE:
        device = grad.device.index or 0
    _check(lib().glx_pair_dot_backward_ex(device, side, pia[0], pib[0], n, repeat, pg[0], heads, px[0], num_rows_other,
                                          dim, num_rows_self, default_attr, po[0], TRAIN_DTYPES[x_dtype], kind,
                                          _stream(kind, device)))
    return grad


EMB_SGD, EMB_ADAGRAD, EMB_ADAM = 0, 1, 2  # GLX_EMB_*
COALESCE_CHUNK = 256  # GLX_COALESCE_CHUNK


def rows_coalesce(rows, g, num_rows, out_rows=None, out_g=None, device=0):
    """The gradient g[n, D] float32 of a lookup of rows[n] int64, summed per distinct row (glx_rows_coalesce) ->
    (urows[n] int64, ug[n, D] float32, count).  A row outside [0, num_rows) is dropped; the U distinct remaining rows
    are urows[:U], ascending, and urows[U:] is -1; ug[:U] holds their sums and ug[U:] is NOT written; count is U.  Each
    list of positions is summed in ascending position in chunks of COALESCE_CHUNK entries whose partial sums are then
    added in order, no float atomic: the same bits on every run, and for lists of at most COALESCE_CHUNK positions the
    rows of aggregate_backward(SUM, ...).  Nothing scales with num_rows.  Torch CUDA tensors are device pointers on the
    current stream and count stays a one-element CUDA tensor (no host read); numpy arrays are host pointers and count
    is an int."""
    n, dim = int(rows.shape[0]), int(g.shape[1])
    assert int(g.shape[0]) == n, "one gradient row per position"
    torch_in = _is_torch(g)
    if torch_in:
        import torch
        urows = out_rows if out_rows is not None else torch.empty((n,), dtype=torch.int64, device=g.device)
        ug = out_g if out_g is not None else torch.empty((n, dim), dtype=torch.float32, device=g.device)
        count = torch.empty((1,), dtype=torch.int64, device=g.device)
    else:
        urows = out_rows if out_rows is not None else np.empty((n,), np.int64)
        ug = out_g if out_g is not None else np.empty((n, dim), np.float32)
        count = np.empty((1,), np.int64)
    pr, pg, pu, po, pc = _ptr(rows), _ptr(g), _ptr(urows), _ptr(ug), _ptr(count)
    kind = _kind(pr, pg, pu, po, pc)
    if kind == PTR_DEVICE:
        device = ug.device.index or 0
    _check(lib().glx_rows_coalesce(device, pr[0], n, num_rows, dim, pg[0], pu[0], po[0], pc[0], kind,
                                   _stream(kind, device)))
    return urows, ug, (count if torch_in else int(count[0]))


def embedding_update(algo, W, urows, ug, state1=None, state2=None, alpha=0.0, eps=0.0, beta1=0.0, c1=0.0, beta2=0.0,
                     c2=0.0):
    """One sparse optimizer step in place on the rows urows[n] names (glx_embedding_update); torch CUDA tensors only.
    W[num_rows, D] float32 and the state tables of its shape: EMB_SGD none, EMB_ADAGRAD state1 (the accumulator),
    EMB_ADAM state1 and state2 (first and second moment).  ug[n, D] is the gradient of entry u's row; an entry outside
    [0, num_rows) -- the -1 tail of rows_coalesce -- is skipped.  The valid entries must name distinct rows (not
    detected: a repeated row is a lost update).  Every operation is one correctly rounded float32 operation; the
    scalars are rounded to float32 once (see include/glx.h for what they are per algorithm)."""
    num_rows, dim = int(W.shape[0]), int(W.shape[1])
    n = int(urows.shape[0])
    assert int(ug.shape[0]) == n and int(ug.shape[1]) == dim, "ug must be [n, D]"
    pw, pu, pg, p1, p2 = _ptr(W), _ptr(urows), _ptr(ug), _ptr(state1), _ptr(state2)
    assert _kind(pw, pu, pg, p1, p2) == PTR_DEVICE, "the tables live on the device: torch CUDA tensors only"
    device = W.device.index or 0
    _check(lib().glx_embedding_update(device, algo, pw[0], p1[0], p2[0], num_rows, dim, pu[0], pg[0], n, alpha, eps,
                                      beta1, c1, beta2, c2, _stream(PTR_DEVICE, device)))


def tgn_backward_depth(n):
    """GLX_TGN_BWD_DEPTH(n): the float32 additions on the longest path of tgn_message_backward's tree over n rows."""
    return 72 + (int(n) + 16383) // 16384


def _tgn_device(*tensors):
    ptrs = [_ptr(x) for x in tensors]
    assert _kind(*ptrs) == PTR_DEVICE, "the TGN memory lives on the device: torch CUDA tensors only"
    first = next(x for x in tensors if x is not None)
    assert all(x is None or x.device == first.device for x in tensors), "every tensor must live on one device"
    return [p[0] for p in ptrs], first.device.index or 0


def tgn_store_update(src, dst, t, raw_msg, seq_base, pend_t, pend_seq, pend_other, pend_raw):
    """One update of the one-slot-per-node message store (glx_tgn_store_update); torch CUDA tensors only, in place, on
    the current stream.  src, dst, t [B] int64, raw_msg [B, R] float32; pend_t, pend_seq, pend_other [N] int64,
    pend_raw [N, R] float32.  Event p has sequence number seq_base + p (a Python int: the number of events of earlier
    calls); the slot of node v ends up holding the event with the largest (t, seq) that ever named v as src or dst.
    Ids outside [0, N) are dropped.  Nothing is read back."""
    N, R, B = int(pend_t.shape[0]), int(pend_raw.shape[1]), int(src.shape[0])
    assert int(dst.shape[0]) == B and int(t.shape[0]) == B and tuple(raw_msg.shape) == (B, R), "one event per position"
    assert int(pend_seq.shape[0]) == N and int(pend_other.shape[0]) == N and int(pend_raw.shape[0]) == N
    p, device = _tgn_device(src, dst, t, raw_msg, pend_t, pend_seq, pend_other, pend_raw)
    _check(lib().glx_tgn_store_update(device, N, R, p[0], p[1], p[2], p[3], B, int(seq_base), p[4], p[5], p[6], p[7],
                                      _stream(PTR_DEVICE, device)))


def tgn_message(memory, last_update, pend_t, pend_seq, pend_other, pend_raw, time_w, time_b, n_id):
    """The fused message of the nodes n_id[n] (glx_tgn_message); torch CUDA tensors only, on the current stream ->
    (msg [n, 2M + R + T], h [n, M], dt [n] float32, t [n] int64, has [n] int32).  For a node with a pending message:
    msg = [memory[v] | memory[other] | raw | cos(time_w * dt + time_b)], dt = float(pend_t[v] - last_update[v]),
    t = pend_t[v]; for any other entry a zero row, dt = 0 and t = last_update[v] (0 outside the table).  h = memory[v]."""
    import torch
    N, M, R, T, n = int(memory.shape[0]), int(memory.shape[1]), int(pend_raw.shape[1]), int(time_w.shape[0]), int(n_id.shape[0])
    assert int(time_b.shape[0]) == T and int(pend_raw.shape[0]) == N and int(last_update.shape[0]) == N
    dev = memory.device
    msg = torch.empty((n, 2 * M + R + T), dtype=torch.float32, device=dev)
    h = torch.empty((n, M), dtype=torch.float32, device=dev)
    dt = torch.empty((n,), dtype=torch.float32, device=dev)
    t_out = torch.empty((n,), dtype=torch.int64, device=dev)
    has = torch.empty((n,), dtype=torch.int32, device=dev)
    p, device = _tgn_device(memory, last_update, pend_t, pend_seq, pend_other, pend_raw, time_w, time_b, n_id, msg, h, dt,
                            t_out, has)
    _check(lib().glx_tgn_message(device, N, M, R, T, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], n, p[9], p[10],
                                 p[11], p[12], p[13], _stream(PTR_DEVICE, device)))
    return msg, h, dt, t_out, has


def tgn_message_backward(grad_msg, dt, has, time_w, time_b, time_off):
    """(grad_w [T], grad_b [T]) of the time encoding in columns [time_off, time_off + T) of grad_msg[n, width], from the
    dt and has of tgn_message (glx_tgn_message_backward); torch CUDA tensors only.  A fixed reduction tree of
    tgn_backward_depth(n) additions on its longest path: the same bits on every call.  Rows with has == 0 contribute
    nothing."""
    import torch
    n, width, T = int(grad_msg.shape[0]), int(grad_msg.shape[1]), int(time_w.shape[0])
    assert int(dt.shape[0]) == n and int(has.shape[0]) == n and int(time_b.shape[0]) == T
    grad_w, grad_b = torch.empty_like(time_w), torch.empty_like(time_b)
    p, device = _tgn_device(grad_msg, dt, has, time_w, time_b, grad_w, grad_b)
    _check(lib().glx_tgn_message_backward(device, n, width, int(time_off), T, p[0], p[1], p[2], p[3], p[4], p[5], p[6],
                                          _stream(PTR_DEVICE, device)))
    return grad_w, grad_b


def tgn_memory_write(memory, last_update, n_id, new_memory, t_new):
    """memory[n_id[i]] = new_memory[i] and last_update[n_id[i]] = t_new[i], in place (glx_tgn_memory_write); torch CUDA
    tensors only.  An id outside the table is skipped.  The valid ids must be distinct (not detected: a repeated id is
    a lost update)."""
    N, M, n = int(memory.shape[0]), int(memory.shape[1]), int(n_id.shape[0])
    assert tuple(new_memory.shape) == (n, M) and int(t_new.shape[0]) == n and int(last_update.shape[0]) == N
    p, device = _tgn_device(n_id, new_memory, t_new, memory, last_update)
    _check(lib().glx_tgn_memory_write(device, N, M, p[0], n, p[1], p[2], p[3], p[4], _stream(PTR_DEVICE, device)))


COLUMN_NAMES = ("weights", "labels", "timestamps", "int_attrs")
COLUMNS_MAP_DENSE, COLUMNS_MAP_OWN, COLUMNS_MAP_BORROWED = 0, 1, 2
# what a requested column answers for an id the table does not know (the reference's Default* flags, config.cc)
COLUMN_DEFAULTS = {"weights": 0.0, "labels": -1, "timestamps": -1, "int_attrs": 0}


def columns_layout(i_num, has_weight=False, has_label=False, has_timestamp=False):
    """The record of a glx_columns table (include/glx.h): byte offsets of the fields a type has
    (None for the others) and the padded record size.  int_attrs int64[i_num] | timestamp int64 | weight float32 |
    label int32, padded to 8 bytes and to a multiple of 16 from 16 bytes on; 0 bytes without any column."""
    at = 8 * i_num
    off = {"int_attrs": 0 if i_num > 0 else None, "timestamps": None, "weights": None, "labels": None}
    if has_timestamp:
        off["timestamps"] = at
        at += 8
    if has_weight:
        off["weights"] = at
        at += 4
    if has_label:
        off["labels"] = at
        at += 4
    at = (at + 7) // 8 * 8
    if at >= 16:
        at = (at + 15) // 16 * 16
    off["record_bytes"] = at
    return off


class Columns:
    """Device-resident label / weight / timestamp / int-attribute columns of one node or edge type (glx_columns)."""

    def __init__(self, num_rows, weights=None, labels=None, timestamps=None, int_attrs=None, ids=None, map_of=None,
                 device=0):
        """Columns: numpy arrays or torch CUDA tensors (all of one kind) -- weights float32[V], labels int32[V],
        timestamps int64[V], int_attrs int64[V, i_num]; None = the type does not have it.  ids: the rows' raw ids (an
        own id map); map_of: a glx.Features of the same rows whose map is borrowed (kept alive); neither: id r is row r."""
        i_num = 0 if int_attrs is None else int(int_attrs.shape[1])
        ptrs = [_ptr(weights), _ptr(labels), _ptr(timestamps), _ptr(int_attrs), _ptr(ids)]
        kinds = set(k for _, k in ptrs if k is not None)
        assert len(kinds) <= 1, "all data pointers of a call must be host (numpy) or device (torch)"
        kind = kinds.pop() if kinds else PTR_HOST
        for x, dt in ((weights, "float32"), (labels, "int32"), (timestamps, "int64"), (int_attrs, "int64"), (ids, "int64")):
            assert x is None or str(x.dtype).replace("torch.", "") == dt, (x.dtype, dt)
        self.device = device
        self._keep = map_of
        h = ctypes.c_void_p()
        _check(lib().glx_columns_create(device, int(num_rows), i_num, ptrs[0][0], ptrs[1][0], ptrs[2][0], ptrs[3][0],
                                        ptrs[4][0], map_of._h if map_of is not None else None, kind,
                                        _stream(kind, device), ctypes.byref(h)))
        self._h = h
        self._read_info()

    def _read_info(self):
        v, i, w, l, t, rb, m, dv = (ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(),
                                    ctypes.c_int32(), ctypes.c_int(), ctypes.c_int())
        _check(lib().glx_columns_info(self._h, ctypes.byref(v), ctypes.byref(i), ctypes.byref(w), ctypes.byref(l),
                                      ctypes.byref(t), ctypes.byref(rb), ctypes.byref(m), ctypes.byref(dv)))
        self.num_rows, self.i_num = v.value, i.value
        self.has = {"weights": bool(w.value), "labels": bool(l.value), "timestamps": bool(t.value),
                    "int_attrs": i.value > 0}
        self.record_bytes, self.id_map, self.device = rb.value, m.value, dv.value

    @classmethod
    def from_handle(cls, handle, device=0):
        """Borrow a glx_columns* owned by someone else (the C++ host layer's Noder / Graph)."""
        self = cls.__new__(cls)
        self._h = ctypes.c_void_p(int(handle))
        self._borrowed = True
        self._keep = None
        self._read_info()
        return self

    def close(self):
        if getattr(self, "_borrowed", False):
            self._h = None
        if getattr(self, "_h", None):
            try:
                lib().glx_columns_destroy(self._h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None

    __del__ = close

    def lookup(self, ids, want=COLUMN_NAMES, defaults=None):
        """-> {name: values} for the names in `want`: weights float32[n], labels int32[n], timestamps int64[n],
        int_attrs int64[n, i_num]; CUDA tensors for CUDA ids, numpy arrays for numpy ids.  defaults: {name: value} an
        unknown id answers with (COLUMN_DEFAULTS for the names left out); a column the type lacks answers 0.0 / -1 / -1."""
        want = tuple(want)
        for name in want:
            if name not in COLUMN_NAMES:
                raise ValueError("unknown column {!r}: one of {}".format(name, COLUMN_NAMES))
        dflt = dict(COLUMN_DEFAULTS)
        dflt.update(defaults or {})
        n = int(ids.shape[0])
        shapes = {"weights": ((n,), "float32"), "labels": ((n,), "int32"), "timestamps": ((n,), "int64"),
                  "int_attrs": ((n, self.i_num), "int64")}
        out = {}
        for name in want:
            shape, dt = shapes[name]
            if _is_torch(ids):
                import torch
                out[name] = torch.empty(shape, dtype=getattr(torch, dt), device=ids.device)
            else:
                out[name] = np.empty(shape, dt)
        pi = _ptr(ids)
        po = [_ptr(out.get(name)) for name in COLUMN_NAMES]
        kind = pi[1]
        _check(lib().glx_columns_lookup(self._h, pi[0], n, dflt["weights"], dflt["labels"], dflt["timestamps"],
                                        dflt["int_attrs"], po[0][0], po[1][0], po[2][0], po[3][0], kind,
                                        _stream(kind, self.device)))
        return out


def sample_hops(graphs, sampler, seeds, fanouts, seed=0, call_counter=0, padding_mode=PAD_CIRCULAR,
                default_neighbor_id=0):
    """Multi-hop driver (NeighborSampler.get): hop h from graphs[h] with fanouts[h].
    -> list of (nbr[rows_h, fanouts[h]], eid[...]) per hop."""
    if isinstance(sampler, str):
        sampler = SAMPLER_IDS[sampler]
    L = len(fanouts)
    assert len(graphs) == L
    rows = int(seeds.shape[0])
    outs = []
    torch_mode = _is_torch(seeds)
    for k in fanouts:
        if torch_mode:
            import torch
            nbr = torch.empty((rows, k), dtype=torch.int64, device=seeds.device)
            eid = torch.empty((rows, k), dtype=torch.int64, device=seeds.device)
        else:
            nbr = np.empty((rows, k), np.int64)
            eid = np.empty((rows, k), np.int64)
        outs.append((nbr, eid))
        rows *= k
    kind = PTR_DEVICE if torch_mode else PTR_HOST
    gh = (ctypes.c_void_p * L)(*[g._h for g in graphs])
    fo = (ctypes.c_int32 * L)(*fanouts)
    pn = (ctypes.c_void_p * L)(*[_ptr(o[0])[0] for o in outs])
    pe = (ctypes.c_void_p * L)(*[_ptr(o[1])[0] for o in outs])
    _check(lib().glx_sample_hops(gh, L, sampler, _ptr(seeds)[0], int(seeds.shape[0]), fo, padding_mode,
                                 default_neighbor_id, seed, call_counter, pn, pe, kind, _stream(kind, graphs[0].device)))
    return outs


def _temporal_outputs(like, rows, k):
    """(nbr, eid, ts, cnt) buffers of one temporal request of `rows` rows, of the kind of `like`."""
    if _is_torch(like):
        import torch
        nbr, eid, ts = (torch.empty((rows, k), dtype=torch.int64, device=like.device) for _ in range(3))
        return nbr, eid, ts, torch.empty(rows, dtype=torch.int32, device=like.device)
    return (np.empty((rows, k), np.int64), np.empty((rows, k), np.int64), np.empty((rows, k), np.int64),
            np.empty(rows, np.int32))


def sample_temporal_hops(graphs, seeds, cutoff, fanouts, strategy="recent", inclusive=False, seed=0, call_counter=0,
                         default_neighbor_id=0, default_timestamp=-1):
    """Multi-hop temporal sampling: hop 0 is Graph.sample_temporal of (seeds, cutoff) on graphs[0]; request row r of
    hop h >= 1 is slot r of hop h - 1 -- its id is that slot's neighbour, its cutoff that slot's edge timestamp -- on
    graphs[h] with stream (seed, call_counter + h).  A default-filled slot yields a default-filled row with cnt = 0.
    -> list over hops of (nbr, eid, ts, cnt), hop h shaped [batch * fanouts[0] * ... * fanouts[h-1], fanouts[h]]."""
    if isinstance(strategy, str):
        strategy = TEMPORAL_STRATEGIES[strategy]
    L = len(fanouts)
    assert len(graphs) == L
    rows = int(seeds.shape[0])
    outs = []
    for k in fanouts:
        outs.append(_temporal_outputs(seeds, rows, k))
        rows *= k
    ps, pc = _ptr(seeds), _ptr(cutoff)
    kind = _kind(ps, pc)
    gh = (ctypes.c_void_p * L)(*[g._h for g in graphs])
    fo = (ctypes.c_int32 * L)(*fanouts)
    po = [(ctypes.c_void_p * L)(*[_ptr(o[i])[0] for o in outs]) for i in range(4)]
    _check(lib().glx_sample_temporal_hops(gh, L, strategy, ps[0], pc[0], int(seeds.shape[0]), fo, 1 if inclusive else 0,
                                          default_neighbor_id, default_timestamp, seed, call_counter, po[0], po[1],
                                          po[2], po[3], kind, _stream(kind, graphs[0].device)))
    return outs


def partition(ids, num_shards):
    """Device HashPartitioner: torch int64 CUDA ids -> (bucketed, order, counts)."""
    import torch
    n = int(ids.shape[0])
    bucketed = torch.empty_like(ids)
    order = torch.empty_like(ids)
    counts = torch.empty(num_shards, dtype=torch.int64, device=ids.device)
    dev = ids.device.index or 0
    _check(lib().glx_partition(dev, _ptr(ids)[0], n, num_shards, _ptr(bucketed)[0], _ptr(order)[0],
                               _ptr(counts)[0], _stream(PTR_DEVICE, dev)))
    return bucketed, order, counts


def stitch(rows, order):
    """Device Stitcher: out[order[i]] = rows[i]; rows is [n, width] int64 or float32 (torch CUDA)."""
    import torch
    n = int(rows.shape[0])
    width = int(rows.numel() // max(n, 1)) if n else 1
    out = torch.empty_like(rows)
    dev = rows.device.index or 0
    fn = lib().glx_stitch_i64 if rows.dtype == torch.int64 else lib().glx_stitch_f32
    assert rows.dtype in (torch.int64, torch.float32)
    _check(fn(dev, _ptr(rows)[0], _ptr(order)[0], n, width, _ptr(out)[0], _stream(PTR_DEVICE, dev)))
    return out


def unique(parts, return_inverse=True, pad=None):
    """Distinct ids of the stream parts[0], parts[1], ... (1 .. 16 int64 arrays of any shape, at most 2^31 - 1 ids in
    all) in order of first occurrence -- no sort, the same answer on every run.
    -> (nodes[m], [inverse of each part, shaped like the part] or None, part_end[len(parts)]):
    nodes[inverse[p]] == parts[p], and nodes[:part_end[p]] is the distinct set of parts[0 .. p].
    Torch CUDA tensors are device pointers on the current stream (the outputs are CUDA tensors, part_end included);
    numpy arrays are host pointers.  The device path reads m = part_end[-1] back with ONE host read, to slice nodes --
    unless `pad` is given (torch only): then nothing is read back and nodes comes at its full length n, the distinct ids
    followed by n - m copies of `pad` (an id the consumer skips, such as -1)."""
    parts = list(parts)
    assert parts, "unique() needs at least one part"
    torch_mode = _is_torch(parts[0])
    if any(_is_torch(p) != torch_mode for p in parts):
        raise ValueError("unique(): every part must be of one kind, numpy arrays or torch CUDA tensors")
    if torch_mode and any(p.device != parts[0].device for p in parts):
        raise ValueError("unique(): every part must live on one device, got {}".format(sorted({str(p.device) for p in parts})))
    lens = [int(np.prod(p.shape)) for p in parts]
    n, P = sum(lens), len(parts)
    if torch_mode:
        import torch
        dev = parts[0].device
        nodes = (torch.empty(n, dtype=torch.int64, device=dev) if pad is None
                 else torch.full((n,), int(pad), dtype=torch.int64, device=dev))
        inverse = torch.empty(n, dtype=torch.int64, device=dev) if return_inverse else None
        part_end = torch.empty(P, dtype=torch.int64, device=dev)
        assert all(p.dtype == torch.int64 for p in parts)
        device = dev.index or 0
    else:
        if pad is not None:
            raise ValueError("unique(): pad needs torch CUDA tensors")
        nodes = np.empty(n, np.int64)
        inverse = np.empty(n, np.int64) if return_inverse else None
        part_end = np.empty(P, np.int64)
        device = 0
    ptrs = [_ptr(p, None if torch_mode else np.int64) for p in parts]
    kind = _kind(*ptrs, _ptr(nodes))
    pp = (ctypes.c_void_p * P)(*[p[0] for p in ptrs])
    pl = (ctypes.c_int64 * P)(*lens)
    _check(lib().glx_unique(device, pp, pl, P, _ptr(nodes)[0], _ptr(inverse)[0], _ptr(part_end)[0], kind,
                            _stream(kind, device)))
    m = n if pad is not None else int(part_end[-1])
    inv = None
    if return_inverse:
        inv, at = [], 0
        for p, k in zip(parts, lens):
            inv.append(inverse[at:at + k].reshape(p.shape))
            at += k
    return nodes[:m], inv, part_end


NEG_EXCLUDE_NONE, NEG_EXCLUDE_NEIGHBORS, NEG_EXCLUDE_BATCH = 0, 1, 2


class Negative:
    """Candidate list of the negative samplers in HBM (glx_negative)."""

    def __init__(self, ids, weights=None, device=0):
        ptrs = [_ptr(ids), _ptr(weights)]
        kind = _kind(*ptrs)
        h = ctypes.c_void_p()
        _check(lib().glx_negative_create(device, int(ids.shape[0]), ptrs[0][0], ptrs[1][0], kind, _stream(kind, device),
                                         ctypes.byref(h)))
        self._h = h
        self.device = device
        self._info()

    @classmethod
    def from_graph(cls, graph, by_in_degree=False):
        """Distinct destination ids of the edge type in first-appearance order, uniform or
        weighted by in-degree."""
        self = cls.__new__(cls)
        h = ctypes.c_void_p()
        _check(lib().glx_negative_from_graph(graph._h, 1 if by_in_degree else 0, None, ctypes.byref(h)))
        self._h = h
        self.device = graph.device
        self._info()
        return self

    def _info(self):
        n, w = ctypes.c_int64(), ctypes.c_int()
        _check(lib().glx_negative_info(self._h, ctypes.byref(n), ctypes.byref(w)))
        self.num_ids, self.weighted = n.value, bool(w.value)

    def close(self):
        if getattr(self, "_h", None):
            try:
                lib().glx_negative_destroy(self._h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None

    __del__ = close

    def export(self):
        """-> (ids, prob or None, alias or None) as numpy arrays."""
        ids = np.zeros(self.num_ids, np.int64)
        prob = np.zeros(self.num_ids, np.float32) if self.weighted else None
        alias = np.zeros(self.num_ids, np.int32) if self.weighted else None
        _check(lib().glx_negative_export(self._h, _ptr(ids)[0], _ptr(prob)[0], _ptr(alias)[0], None))
        return ids, prob, alias

    def sample(self, src, count, exclude=NEG_EXCLUDE_NONE, graph=None, default_neighbor_id=0, seed=0,
               call_counter=0):
        """-> out[batch, count] candidate ids (numpy in -> numpy out, torch CUDA in -> torch CUDA out)."""
        batch = int(src.shape[0])
        if _is_torch(src):
            import torch
            out = torch.empty((batch, count), dtype=torch.int64, device=src.device)
        else:
            out = np.empty((batch, count), np.int64)
        ps, po = _ptr(src), _ptr(out)
        kind = _kind(ps, po)
        _check(lib().glx_negative_sample(self._h, exclude, graph._h if graph is not None else None, ps[0], batch,
                                         count, default_neighbor_id, seed, call_counter, po[0], kind, _stream(kind, self.device)))
        return out


def aggregate_stitch(op, parts, cnts, default_attr=0.0):
    """Device AggregatingResponse::Stitch: parts [P, Sg, D] float32 + cnts [P, Sg] int32
    (torch CUDA, contiguous: the receive buffers of one all-to-all) -> (emb [Sg, D], cnt [Sg])."""
    import torch
    if isinstance(op, str):
        op = AGGREGATOR_IDS[op]
    P, sg, dim = (int(x) for x in parts.shape)
    assert parts.dtype == torch.float32 and cnts.dtype == torch.int32 and tuple(cnts.shape) == (P, sg)
    assert parts.is_contiguous() and cnts.is_contiguous()
    emb = torch.empty((sg, dim), dtype=torch.float32, device=parts.device)
    cnt = torch.empty((sg,), dtype=torch.int32, device=parts.device)
    dev = parts.device.index or 0
    _check(lib().glx_aggregate_stitch(dev, op, P, _ptr(parts)[0], _ptr(cnts)[0], sg, dim, default_attr,
                                      _ptr(emb)[0], _ptr(cnt)[0], _stream(PTR_DEVICE, dev)))
    return emb, cnt


COMM_RCCL, COMM_LOCAL, COMM_CALLBACKS = 0, 1, 2
UNIQUE_ID_BYTES = 128


class Comm:
    """Shard communicator (glx_comm): RCCL over xGMI, in-process threads, or host-staged callbacks."""

    def __init__(self, handle, keep=None):
        self._h = handle
        self._keep = keep  # ctypes callback objects must outlive the handle
        r, w, d, t = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(lib().glx_comm_info(handle, ctypes.byref(r), ctypes.byref(w), ctypes.byref(d), ctypes.byref(t)))
        self.rank, self.world, self.device, self.transport = r.value, w.value, d.value, t.value

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(UNIQUE_ID_BYTES)
        _check(lib().glx_comm_unique_id(buf))
        return buf.raw

    @classmethod
    def rccl(cls, device, rank, world, unique_id):
        h = ctypes.c_void_p()
        assert len(unique_id) == UNIQUE_ID_BYTES
        _check(lib().glx_comm_init_rccl(device, rank, world, ctypes.c_char_p(unique_id), ctypes.byref(h)))
        return cls(h)

    @classmethod
    def local(cls, fabric_key, device, rank, world):
        """Ranks = threads of this process (ctypes releases the GIL inside the collectives)."""
        h = ctypes.c_void_p()
        _check(lib().glx_comm_init_local(fabric_key, device, rank, world, ctypes.byref(h)))
        return cls(h)

    @classmethod
    def callbacks(cls, device, rank, world, alltoallv, allgather):
        """Host-staged transport.  alltoallv(send_u8, send_counts, recv_u8, recv_counts, elem_bytes) and
        allgather(send_u8, recv_u8) get numpy views of the pinned staging buffers."""
        def _a2a(_user, send, send_counts, recv, recv_counts, eb):
            try:
                sc = np.ctypeslib.as_array((ctypes.c_int64 * world).from_address(send_counts)).copy()
                rc = np.ctypeslib.as_array((ctypes.c_int64 * world).from_address(recv_counts)).copy()
                ns, nr = int(sc.sum()) * eb, int(rc.sum()) * eb
                sb = np.ctypeslib.as_array((ctypes.c_uint8 * max(ns, 1)).from_address(send))[:ns] if send else np.empty(0, np.uint8)
                rb = np.ctypeslib.as_array((ctypes.c_uint8 * max(nr, 1)).from_address(recv))[:nr] if recv else np.empty(0, np.uint8)
                alltoallv(sb, sc, rb, rc, int(eb))
                return 0
            except Exception:  # noqa: BLE001 -- an exception must not unwind through C
                import traceback
                traceback.print_exc()
                return 1

        def _ag(_user, send, recv, nbytes):
            try:
                sb = np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(send))
                rb = np.ctypeslib.as_array((ctypes.c_uint8 * (nbytes * world)).from_address(recv))
                allgather(sb, rb)
                return 0
            except Exception:  # noqa: BLE001
                import traceback
                traceback.print_exc()
                return 1
        c1, c2 = HOST_ALLTOALLV_FN(_a2a), HOST_ALLGATHER_FN(_ag)
        h = ctypes.c_void_p()
        _check(lib().glx_comm_init_callbacks(device, rank, world, c1, c2, None, ctypes.byref(h)))
        return cls(h, keep=(c1, c2))

    def close(self):
        if getattr(self, "_h", None):
            try:
                lib().glx_comm_destroy(self._h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None

    __del__ = close

    def set_max_message_bytes(self, nbytes):
        return int(lib().glx_comm_set_max_message_bytes(self._h, int(nbytes)))

    def exchange_v(self, send, send_counts, recv_counts):
        """all-to-all(v) of the rows of `send` (numpy or torch CUDA, packed peer-major) -> received rows."""
        sc = np.ascontiguousarray(send_counts, dtype=np.int64)
        rc = np.ascontiguousarray(recv_counts, dtype=np.int64)
        n = int(rc.sum())
        width = 1
        for d in send.shape[1:]:
            width *= int(d)
        if _is_torch(send):
            import torch
            out = torch.empty((n,) + tuple(send.shape[1:]), dtype=send.dtype, device=send.device)
            eb = send.element_size() * width
        else:
            out = np.empty((n,) + tuple(send.shape[1:]), send.dtype)
            eb = send.dtype.itemsize * width
        ps, po = _ptr(send), _ptr(out)
        kind = _kind(ps, po)
        _check(lib().glx_exchange_v(self._h, ps[0], _ptr(sc)[0], po[0], _ptr(rc)[0], eb, kind, _stream(kind, self.device)))
        return out

    def allgather_i64(self, vals):
        """vals[nvals] int64 (numpy or torch CUDA) of every rank -> [world, nvals] of the same kind."""
        n = int(vals.shape[0])
        if _is_torch(vals):
            import torch
            out = torch.empty((self.world, n), dtype=torch.int64, device=vals.device)
        else:
            out = np.empty((self.world, n), np.int64)
        pv, po = _ptr(vals), _ptr(out)
        kind = _kind(pv, po)
        _check(lib().glx_comm_allgather_i64(self._h, pv[0], n, po[0], kind, _stream(kind, self.device)))
        return out

    def barrier(self):
        _check(lib().glx_comm_barrier(self._h, _stream(PTR_DEVICE, self.device)))


class DistStore:
    """One rank's shard of an edge-cut partitioned graph + feature table behind a communicator
    (glx_dist_store): the device-resident DistributeRunner.  Every method except stats() is
    COLLECTIVE: all ranks of the communicator call it together, each with its own request."""

    def __init__(self, comm, graph=None, features=None):
        h = ctypes.c_void_p()
        _check(lib().glx_dist_store_create(comm._h, graph._h if graph is not None else None,
                                           features._h if features is not None else None, ctypes.byref(h)))
        self._h = h
        self.comm, self.graph, self.features = comm, graph, features
        self.dim = features.dim if features is not None else None

    def close(self):
        if getattr(self, "_h", None):
            try:
                lib().glx_dist_store_destroy(self._h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None

    __del__ = close

    def set_cache(self, hot_ids, default_attr=0.0):
        """Replicate the rows of hot_ids (same list on every rank) on this GPU; empty list drops the replica."""
        n = int(hot_ids.shape[0])
        p, kind = _ptr(hot_ids) if n else (None, PTR_HOST)
        _check(lib().glx_dist_store_set_cache(self._h, p, n, default_attr, kind, _stream(kind, self.comm.device)))

    def set_graph_replica(self, replica):
        """Serve request rows of the vertices `replica` (a glx.Graph built with explicit ids, holding their complete
        adjacency rows) on this GPU instead of sending them to their owners; None detaches it.  The store keeps a
        reference so the replica outlives its use."""
        _check(lib().glx_dist_store_set_graph_replica(self._h, replica._h if replica is not None else None))
        self._graph_replica = replica

    def build_graph_replica(self, hot_ids, attach=True):
        """Collective: the complete adjacency rows of hot_ids (same list on every rank; unique ids), cut out of the
        shards by their owners and all-gathered -> a glx.Graph on this GPU (owned by the caller).  attach=True also
        makes the store serve those vertices' sampling requests from it (set_graph_replica)."""
        n = int(hot_ids.shape[0])
        p, kind = _ptr(hot_ids)
        h = ctypes.c_void_p()
        _check(lib().glx_dist_build_graph_replica(self._h, p, n, kind, _stream(kind, self.comm.device), ctypes.byref(h)))
        g = Graph.from_handle(h.value)
        g._borrowed = False  # ours to destroy
        if attach:
            self.set_graph_replica(g)
        return g

    def sample_full(self, src, max_limit=0, filter_type=FILTER_NONE, filter_field=FILTER_FIELD_NONE, values=None,
                    padding_mode=PAD_CIRCULAR, default_neighbor_id=0, default_timestamp=-1):
        """Collective FullSampler over the shards: -> (degrees[batch] int32, nbr[total], eid[total]) for this rank's
        rows, as Graph.sample_full / sample_full_filtered answer on one store (numpy in -> numpy out, torch CUDA in ->
        torch CUDA out).  With a filter: values[batch], same kind as src; every rank passes the same kind of filter."""
        batch = int(src.shape[0])
        if _is_torch(src):
            import torch
            mk = lambda n, dt: torch.empty(n, dtype=dt, device=src.device)  # noqa: E731
            deg, off, i64t = mk(batch, torch.int32), mk(batch + 1, torch.int64), torch.int64
        else:
            mk = lambda n, dt: np.empty(n, dt)  # noqa: E731
            deg, off, i64t = mk(batch, np.int32), mk(batch + 1, np.int64), np.int64
        ps, kind = _ptr(src) if batch else (None, PTR_DEVICE if _is_torch(src) else PTR_HOST)
        stream = _stream(kind, self.comm.device)
        _check(lib().glx_dist_sample_full_sizes(self._h, ps, batch, max_limit, _ptr(deg)[0] if batch else None, _ptr(off)[0],
                                                kind, stream))
        total = int(off[-1])
        nbr, eid = mk(total, i64t), mk(total, i64t)
        if filter_type != FILTER_NONE:
            flt = Filter(filter_type, filter_field, _ptr(values)[0] if batch else None, 0, default_timestamp)
            _check(lib().glx_dist_sample_full_filtered(self._h, ps, batch, max_limit, _ptr(deg)[0] if batch else None,
                                                       _ptr(off)[0], padding_mode, default_neighbor_id, ctypes.byref(flt),
                                                       _ptr(nbr)[0] if total else None, _ptr(eid)[0] if total else None, total,
                                                       kind, stream))
            return deg, nbr, eid
        _check(lib().glx_dist_sample_full(self._h, ps, batch, max_limit, _ptr(deg)[0] if batch else None, _ptr(off)[0],
                                          _ptr(nbr)[0] if total else None, _ptr(eid)[0] if total else None, total, kind, stream))
        return deg, nbr, eid

    def in_degrees(self, ids):
        """Collective GetDegree for destination ids: in-degrees summed over all shards (int32; numpy or torch CUDA)."""
        n = int(ids.shape[0])
        if _is_torch(ids):
            import torch
            out, kind = torch.empty(n, dtype=torch.int32, device=ids.device), PTR_DEVICE
        else:
            out, kind = np.empty(n, np.int32), PTR_HOST
        _check(lib().glx_dist_in_degrees(self._h, _ptr(ids)[0] if n else None, n, _ptr(out)[0] if n else None, kind,
                                         _stream(kind, self.comm.device)))
        return out

    def negative_table(self, by_in_degree=False):
        """Collective: the negative samplers' candidate list over the WHOLE edge type (every shard's destination ids,
        ascending, uniform or weighted by global in-degree) -> a Negative, identical on every rank."""
        t = Negative.__new__(Negative)
        h = ctypes.c_void_p()
        _check(lib().glx_dist_negative_create(self._h, 1 if by_in_degree else 0, _stream(PTR_DEVICE, self.comm.device),
                                              ctypes.byref(h)))
        t._h, t.device = h, self.comm.device
        t._info()
        return t

    def negative_sample(self, table, src, count, exclude=NEG_EXCLUDE_NONE, default_neighbor_id=0, seed=0, call_counter=0):
        """glx_negative_sample across the shards (collective for NEG_EXCLUDE_NEIGHBORS): -> out[batch, count]."""
        batch = int(src.shape[0])
        if _is_torch(src):
            import torch
            out, kind = torch.empty((batch, count), dtype=torch.int64, device=src.device), PTR_DEVICE
        else:
            out, kind = np.empty((batch, count), np.int64), PTR_HOST
        _check(lib().glx_dist_negative_sample(self._h, table._h, exclude, _ptr(src)[0] if batch else None, batch, count,
                                              default_neighbor_id, seed, call_counter,
                                              _ptr(out)[0] if batch * count else None, kind, _stream(kind, self.comm.device)))
        return out

    def random_walk(self, seeds, walk_len, p=1.0, q=1.0, default_neighbor_id=0, seed=0, call_counter=0, full_nbr_num=100,
                    default_weight=0.0):
        """Collective RandomWalk over the shards (DeepWalk when p = q = 1, node2vec otherwise): -> walks[batch, walk_len],
        Graph.random_walk's draws."""
        batch = int(seeds.shape[0])
        if _is_torch(seeds):
            import torch
            walks = torch.empty((batch, walk_len), dtype=torch.int64, device=seeds.device)
            kind = PTR_DEVICE
        else:
            walks = np.empty((batch, walk_len), np.int64)
            kind = PTR_HOST
        _check(lib().glx_dist_random_walk_ex(self._h, _ptr(seeds)[0] if batch else None, batch, walk_len, p, q, full_nbr_num,
                                             default_weight, default_neighbor_id, seed, call_counter,
                                             _ptr(walks)[0] if batch * walk_len else None, kind,
                                             _stream(kind, self.comm.device)))
        return walks

    def last_sample_rows(self):
        """{'rows', 'from_graph_replica', 'remote'} of the last sample() on this rank."""
        a, b, c = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _check(lib().glx_dist_last_sample_rows(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return {"rows": a.value, "from_graph_replica": b.value, "remote": c.value}

    def hot_ids(self, want):
        """The `want` destination ids with the largest global in-degree (numpy int64, same on every rank)."""
        out = np.empty(max(int(want), 1), np.int64)
        n = ctypes.c_int64(0)
        _check(lib().glx_dist_hot_ids(self._h, int(want), _ptr(out)[0], ctypes.byref(n), _stream(PTR_DEVICE, self.comm.device)))
        return out[:n.value].copy()

    def enable_in_degree(self):
        """Collective: build the shard's InDegreeSampler tables from in-degrees summed over all shards."""
        _check(lib().glx_dist_enable_in_degree(self._h, self.graph._h, _stream(PTR_DEVICE, self.comm.device)))

    def sample(self, sampler, src, k, seed=0, call_counter=0, padding_mode=PAD_CIRCULAR, default_neighbor_id=0,
               out=None, filter_type=FILTER_NONE, filter_field=FILTER_FIELD_NONE, values=None, retry_times=5,
               default_timestamp=-1):
        if isinstance(sampler, str):
            sampler = SAMPLER_IDS[sampler] if sampler in SAMPLER_IDS else EXTRA_SAMPLER_IDS[sampler]
        batch = int(src.shape[0])
        if out is not None:
            nbr, eid = out
        elif _is_torch(src):
            import torch
            nbr = torch.empty((batch, k), dtype=torch.int64, device=src.device)
            eid = torch.empty((batch, k), dtype=torch.int64, device=src.device)
        else:
            nbr = np.empty((batch, k), np.int64)
            eid = np.empty((batch, k), np.int64)
        ps, pn, pe, pv = _ptr(src), _ptr(nbr), _ptr(eid), _ptr(values)
        kind = _kind(ps, pn, pe, pv)
        flt = None
        if values is not None and filter_type != FILTER_NONE:
            flt = ctypes.byref(Filter(filter_type, filter_field, pv[0], retry_times, default_timestamp))
        _check(lib().glx_dist_sample(self._h, sampler, ps[0], batch, k, padding_mode, default_neighbor_id, seed,
                                     call_counter, flt, pn[0], pe[0], kind, _stream(kind, self.comm.device)))
        return nbr, eid

    def aggregate(self, op, node_ids, segment_ids, num_segments, default_attr=0.0, out=None, partial=False):
        """segment_ids=None: num_segments equal segments (a dense sampler response).  partial=True: design R -- owners
        reduce, the requester folds the partial results (glx_dist_aggregate_partial) instead of the halo-row exchange."""
        if isinstance(op, str):
            op = AGGREGATOR_IDS[op]
        n = int(node_ids.shape[0])
        if out is not None:
            emb, cnt = out
        elif _is_torch(node_ids):
            import torch
            emb = torch.empty((num_segments, self.dim), dtype=torch.float32, device=node_ids.device)
            cnt = torch.empty((num_segments,), dtype=torch.int32, device=node_ids.device)
        else:
            emb = np.empty((num_segments, self.dim), np.float32)
            cnt = np.empty((num_segments,), np.int32)
        pi, pg, pe, pc = _ptr(node_ids), _ptr(segment_ids), _ptr(emb), _ptr(cnt)
        kind = _kind(pi, pg, pe, pc)
        fn = lib().glx_dist_aggregate_partial if partial else lib().glx_dist_aggregate
        _check(fn(self._h, op, pi[0], pg[0], n, num_segments, default_attr, pe[0], pc[0], kind, _stream(kind, self.comm.device)))
        return emb, cnt

    def aggregate_begin(self, slot, node_ids, default_attr=0.0):
        """Collective half of aggregate(): resolve the ids and fetch the halo rows into buffer set `slot`
        (torch CUDA ids, on the current stream) -- may run ahead of aggregate_end, beside an earlier reduce."""
        assert _is_torch(node_ids) and node_ids.is_cuda and node_ids.is_contiguous()
        _check(lib().glx_dist_aggregate_begin(self._h, slot, _ptr(node_ids)[0], int(node_ids.shape[0]), default_attr,
                                              _stream(PTR_DEVICE, self.comm.device)))

    def aggregate_end(self, slot, op, segment_ids, num_segments, out):
        """Local half: the segmented reduce over the rows aggregate_begin(slot, ...) prepared."""
        if isinstance(op, str):
            op = AGGREGATOR_IDS[op]
        emb, cnt = out
        _check(lib().glx_dist_aggregate_end(self._h, slot, op, _ptr(segment_ids)[0], num_segments, _ptr(emb)[0],
                                            _ptr(cnt)[0], _stream(PTR_DEVICE, self.comm.device)))
        return emb, cnt

    def aggregate_end_range(self, slot, first_id, num_ids, op, segment_ids, num_segments, out, release=False):
        """The reduce over ids [first_id, first_id + num_ids) of the request begun in `slot` (one begin, several
        aggregating requests: glx_dist_aggregate_end_range); release=True ends the slot's request."""
        if isinstance(op, str):
            op = AGGREGATOR_IDS[op]
        emb, cnt = out
        _check(lib().glx_dist_aggregate_end_range(self._h, slot, int(first_id), int(num_ids), 1 if release else 0, op,
                                                  _ptr(segment_ids)[0], num_segments, _ptr(emb)[0], _ptr(cnt)[0],
                                                  _stream(PTR_DEVICE, self.comm.device)))
        return emb, cnt

    def lookup(self, node_ids, default_attr=0.0):
        n = int(node_ids.shape[0])
        if _is_torch(node_ids):
            import torch
            out = torch.empty((n, self.dim), dtype=torch.float32, device=node_ids.device)
        else:
            out = np.empty((n, self.dim), np.float32)
        pi, po = _ptr(node_ids), _ptr(out)
        kind = _kind(pi, po)
        _check(lib().glx_dist_lookup(self._h, pi[0], n, default_attr, po[0], kind, _stream(kind, self.comm.device)))
        return out

    def stats(self):
        st = DistStats()
        _check(lib().glx_dist_last_stats(self._h, ctypes.byref(st)))
        return st.as_dict()

    def confirm(self):
        """A confirmation point for speculated sample calls (Ledger): one count exchange; raises GlxError(ABORTED)
        on every rank when a speculated message overflowed."""
        _check(lib().glx_dist_confirm(self._h, _stream(PTR_DEVICE, self.comm.device)))


class LedgerStats(ctypes.Structure):
    _fields_ = [("speculated", ctypes.c_int64), ("learned", ctypes.c_int64), ("aborted", ctypes.c_int64),
                ("holding", ctypes.c_int64), ("largest_share", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Ledger:
    """glx_dist_ledger: lets glx_dist_sample skip its count exchange for requests whose shape repeats (fixed-capacity
    messages; whether they fitted is confirmed by the next count exchange of any store attached to the ledger, which
    raises GlxError with code ABORTED on every rank when they did not).  One per rank."""

    def __init__(self, device=0):
        h = ctypes.c_void_p()
        _check(lib().glx_dist_ledger_create(int(device), ctypes.byref(h)))
        self._h = h
        self._stores = []

    def attach(self, *stores):
        for st in stores:
            _check(lib().glx_dist_store_set_ledger(st._h, self._h))
            st._ledger = self  # the ledger outlives the stores attached to it
            self._stores.append(st)
        return self

    def detach(self, *stores):
        for st in stores:
            if getattr(st, "_h", None):  # (a store closed before its ledger has nothing left to detach)
                _check(lib().glx_dist_store_set_ledger(st._h, None))
            st._ledger = None
            self._stores = [x for x in self._stores if x is not st]

    def set_slack(self, slack=1.25, pad_rows=1024):
        _check(lib().glx_dist_ledger_set_slack(self._h, float(slack), int(pad_rows)))

    def stats(self):
        st = LedgerStats()
        _check(lib().glx_dist_ledger_get_stats(self._h, ctypes.byref(st)))
        return st.as_dict()

    def close(self):
        if self._h:
            self.detach(*list(self._stores))
            lib().glx_dist_ledger_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _DevArray:
    """A device buffer owned by a C handle, exposed to torch without a copy (CUDA array interface)."""

    def __init__(self, ptr, shape, typestr, owner):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}
        self._owner = owner  # keeps the plan alive while a tensor view exists


class Plan:
    """A fixed-shape multi-hop sample (+ aggregate) request captured into one hipGraph (glx_plan): the
    launch-bound small-batch path.  run(seeds, call_counter) replays it on torch's current stream; the outputs
    are views of plan-owned device buffers, overwritten by the next run."""

    def __init__(self, graphs, sampler, fanouts, batch, features=None, agg=None, seed=0, padding_mode=PAD_CIRCULAR,
                 default_neighbor_id=0, default_attr=0.0):
        import torch
        if isinstance(sampler, str):
            sampler = SAMPLER_IDS[sampler] if sampler in SAMPLER_IDS else EXTRA_SAMPLER_IDS[sampler]
        L = len(fanouts)
        assert len(graphs) == L and (features is None or len(features) == L)
        self.device = graphs[0].device
        self._keep = (list(graphs), list(features) if features is not None else None)
        gh = (ctypes.c_void_p * L)(*[g._h for g in graphs])
        fo = (ctypes.c_int32 * L)(*[int(f) for f in fanouts])
        fh = (ctypes.c_void_p * L)(*[f._h for f in features]) if features is not None else None
        op = AGGREGATOR_IDS[agg] if isinstance(agg, str) else (agg if agg is not None else 0)
        h = ctypes.c_void_p()
        _check(lib().glx_plan_create(gh, L, sampler, fo, int(batch), padding_mode, default_neighbor_id, seed, fh, op,
                                     default_attr, ctypes.byref(h)))
        self._h = h
        self.batch, self.num_hops = int(batch), L
        self.hops = []
        dev = torch.device("cuda", self.device)
        for hop in range(L):
            pn, pe, pm, pc = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
            rows, fan = ctypes.c_int64(), ctypes.c_int32()
            _check(lib().glx_plan_output(h, hop, ctypes.byref(pn), ctypes.byref(pe), ctypes.byref(pm), ctypes.byref(pc),
                                         ctypes.byref(rows), ctypes.byref(fan)))
            r, k = rows.value, fan.value
            out = {"nbr": torch.as_tensor(_DevArray(pn.value, (r, k), "<i8", self), device=dev),
                   "eid": torch.as_tensor(_DevArray(pe.value, (r, k), "<i8", self), device=dev)}
            if features is not None:
                out["emb"] = torch.as_tensor(_DevArray(pm.value, (r, features[hop].dim), "<f4", self), device=dev)
                out["cnt"] = torch.as_tensor(_DevArray(pc.value, (r,), "<i4", self), device=dev)
            self.hops.append(out)

    def run(self, seeds, call_counter=0):
        assert _is_torch(seeds) and seeds.is_cuda and seeds.is_contiguous() and int(seeds.shape[0]) == self.batch
        _check(lib().glx_plan_run(self._h, _ptr(seeds)[0], call_counter, _stream(PTR_DEVICE, self.device)))
        return self.hops

    def close(self):
        """Frees the plan's device buffers and lets go of the stores it was captured over.  The output tensors keep their
        plan alive through the array interface (a reference cycle that runs through torch's C++ side, which the garbage
        collector cannot see): a caller that wants the memory back calls close() -- dropping the last Python name is not
        enough."""
        if getattr(self, "_h", None):
            try:
                lib().glx_plan_destroy(self._h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None
        self.hops = []
        self._keep = None

    __del__ = close


KERNEL_SAMPLE, KERNEL_AGGREGATE, KERNEL_LOOKUP = 0, 1, 2


i64_t = ctypes.c_int64
NO_KEY = -(1 << 63)  # a dst key that matches no group


class CondTable:
    """glx_cond_table: ids [U], weights [U] | None, cand_keys [ncols, U] int64 (numpy or torch-on-device)."""

    def __init__(self, ids, weights, cand_keys, device=0):
        self.device = device
        self.num_ids = int(ids.shape[0])
        self.num_cols = 0 if cand_keys is None else int(cand_keys.reshape(-1, max(self.num_ids, 1)).shape[0]) if self.num_ids else 0
        pi, pw, pk = _ptr(ids), _ptr(weights), _ptr(cand_keys)
        kind = _kind(pi, pw, pk)
        h = ctypes.c_void_p()
        _check(lib().glx_cond_table_create(device, self.num_ids, pi[0], pw[0], self.num_cols, pk[0], kind, _stream(kind, device),
                                           ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().glx_cond_table_destroy(self._h)
            self._h = None

    __del__ = close

    def sample(self, graph, src, dst, dst_keys, props, count, batch_share=False, unique=False, retry=5,
               default_neighbor_id=0, seed=0, call_counter=0):
        """-> out [batch, count] int64 (numpy in -> numpy out, torch in -> torch out)."""
        batch = int(src.shape[0])
        if _is_torch(src):
            import torch
            out = torch.empty((batch, count), dtype=torch.int64, device=src.device)
        else:
            out = np.empty((batch, count), np.int64)
        props = np.ascontiguousarray(props, np.float32)
        ps, pd, pk, po = _ptr(src), _ptr(dst), _ptr(dst_keys), _ptr(out)
        kind = _kind(ps, pd, pk, po)
        _check(lib().glx_cond_negative_sample(self._h, graph._h if graph is not None else None, ps[0], pd[0], pk[0],
                                              ctypes.c_void_p(props.ctypes.data), batch, count, int(batch_share), int(unique),
                                              retry, default_neighbor_id, seed, call_counter, po[0], kind,
                                              _stream(kind, self.device)))
        return out


def subgraph_induce(nodes, offsets, nbr, eid, device=0):
    """glx_subgraph_induce on FullSampler's response rows of `nodes` -> (row[m] int32, col[m] int32, eid[m] int64);
    numpy in -> numpy out, torch (device) in -> torch out."""
    n = int(nodes.shape[0])
    pn, po, pb, pe = _ptr(nodes), _ptr(offsets), _ptr(nbr), _ptr(eid)
    kind = _kind(pn, po, pb, pe)
    total = i64_t()
    _check(lib().glx_subgraph_induce(device, pn[0], n, po[0], pb[0], pe[0], None, None, None, 0, ctypes.byref(total), kind,
                                     _stream(kind, device)))
    m = int(total.value)
    if _is_torch(nodes):
        import torch
        row = torch.empty(m, dtype=torch.int32, device=nodes.device)
        col = torch.empty(m, dtype=torch.int32, device=nodes.device)
        out = torch.empty(m, dtype=torch.int64, device=nodes.device)
    else:
        row, col, out = np.empty(m, np.int32), np.empty(m, np.int32), np.empty(m, np.int64)
    if m:
        _check(lib().glx_subgraph_induce(device, pn[0], n, po[0], pb[0], pe[0], _ptr(row)[0], _ptr(col)[0], _ptr(out)[0], m,
                                         ctypes.byref(total), kind, _stream(kind, device)))
    return row, col, out


PROBES = {"stream_read": 0, "copy": 1, "triad": 2, "gather32": 3, "gather_rows": 4}


def probe_bandwidth(kind, nbytes, units=0, unit_bytes=0, reps=10, device=0):
    """glx_probe_bandwidth: -> dict(gbps, ms, moved_bytes) of one hand-written streaming / gather kernel."""
    moved, ms = ctypes.c_double(), ctypes.c_double()
    _check(lib().glx_probe_bandwidth(device, PROBES[kind] if isinstance(kind, str) else kind, int(nbytes), int(units),
                                     int(unit_bytes), int(reps), ctypes.byref(moved), ctypes.byref(ms),
                                     _stream(PTR_DEVICE, device)))
    return {"gbps": moved.value / (ms.value * 1e-3) / 1e9, "ms": ms.value, "moved_bytes": moved.value}


def tune(name, value):
    """glx_tune: set a measurement knob of the aggregation launch (agg_unroll, agg_legacy, agg_segs, ...)."""
    _check(lib().glx_tune(name.encode(), int(value)))


def profile_enable(on=True):
    _check(lib().glx_profile_enable(1 if on else 0))


def profile_collect(kind, cap=1 << 16):
    """Durations (ms) of the timed dominant-kernel launches of `kind`, oldest first."""
    buf = np.zeros(cap, np.float32)
    n = ctypes.c_int32(0)
    _check(lib().glx_profile_collect(kind, _ptr(buf)[0], cap, ctypes.byref(n)))
    return buf[:n.value].copy()
