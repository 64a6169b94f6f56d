/* glx -- MI355X-native drop-in for the graph-learn sampling / aggregation hot path.
 *
 * This is the C-ABI boundary (plain pointers and sizes; no C++/torch types).
 * The C++ operators that mirror the reference's registry (graph-learn_amd/host)
 * call it from their Process() bodies; a maintainer of the reference would call
 * it the same way from graphlearn::op::Sampler / Aggregator subclasses (see
 * INTEGRATION.md).  Every entry point names the reference interface it replaces.
 *
 * Conventions
 *   - return value: graphlearn::error::Code (graphlearn/src/include/status.h:29-49),
 *     0 = OK; a message for the last failure on this thread: glx_last_error().
 *   - `ptr_kind` says whether the data pointers of THAT call are host
 *     (GLX_PTR_HOST: the call copies in/out and returns when results are in
 *     host memory) or device pointers on the handle's GPU (GLX_PTR_DEVICE: the
 *     call only enqueues work on `stream` and returns; the caller orders later
 *     use on that stream).
 *   - `stream` is a hipStream_t passed as void*.  NULL means the null stream for
 *     device-pointer calls; host-pointer calls with NULL run on a private
 *     per-(host thread, device) stream so that concurrent callers overlap.
 *   - handles are immutable after creation and may be used concurrently from
 *     any number of host threads (the reference calls Process() from up to 32
 *     pool threads on one operator instance: in_memory_service.cc:64-71).
 *   - no entry point throws or takes ownership of caller memory.
 */
#ifndef GLX_H_
#define GLX_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1: graph / features / samplers / aggregators / partition helpers.  2 (additions only): host registration, shard
 * communicator, distributed store (+ replicas), request plans.  3 (additions only): memory-system probes,
 * induced sub-graph, conditional negative sampling.  4 (additions only): the speculation ledger of the distributed store
 * (glx_dist_ledger_*, glx_dist_confirm, GLX_ABORTED), glx_tune.  5 (additions only): glx_dist_sample_full_filtered,
 * glx_dist_in_degrees, glx_dist_negative_create, glx_dist_negative_sample, glx_dist_random_walk_ex (all added during
 * round 4 under 4), glx_graph_enable_default_weight.  Added under 5 (additions only): half-precision
 * feature tables -- GLX_DTYPE_*, glx_features_create_ex, glx_features_view_ex, glx_features_dtype;
 * glx_graph_edge_weight_packed; frontier dedup -- glx_unique; device-resident label / weight / timestamp / int-attribute
 * columns -- glx_columns_create, glx_columns_lookup, glx_columns_info, glx_columns_destroy; differentiable aggregation --
 * glx_aggregate_arg, glx_aggregate_backward; weighted aggregation -- glx_aggregate_weighted,
 * glx_aggregate_weighted_backward_x, glx_aggregate_weighted_backward_w; ragged segment softmax -- glx_segment_softmax,
 * glx_segment_softmax_backward; pair scores -- glx_pair_dot, glx_pair_dot_backward; trainable embedding tables --
 * glx_rows_coalesce, glx_embedding_update; fused GAT attention -- glx_gat_attention, glx_gat_attention_backward; fused
 * dot-product attention -- glx_dot_attention, glx_dot_attention_backward; exact KNN search -- GLX_KNN_*, glx_knn_search,
 * glx_knn_merge; TGN memory -- glx_tgn_store_update, glx_tgn_message, glx_tgn_message_backward, glx_tgn_memory_write;
 * IVF-Flat index -- glx_knn_ivf_build, glx_knn_ivf_search, glx_knn_ivf_info, glx_knn_ivf_export, glx_knn_ivf_destroy;
 * IVF-PQ index -- glx_knn_ivfpq_build, glx_knn_ivfpq_search, glx_knn_ivfpq_info, glx_knn_ivfpq_export,
 * glx_knn_ivfpq_destroy; float8 feature tables -- GLX_DTYPE_F8E4M3, GLX_DTYPE_F8E5M2, glx_features_convert_host;
 * the bfloat16 training path -- glx_aggregate_backward_ex, glx_aggregate_weighted_ex,
 * glx_aggregate_weighted_backward_x_ex, glx_aggregate_weighted_backward_w_ex, glx_pair_dot_ex,
 * glx_pair_dot_backward_ex; chunked row gradients -- glx_aggregate_backward_chunked,
 * glx_aggregate_weighted_backward_x_chunked. */
#define GLX_ABI_VERSION 5

/* Exported symbols: libglx.so is built with -fvisibility=hidden. */
#if defined(__GNUC__)
#define GLX_API __attribute__((visibility("default")))
#else
#define GLX_API
#endif

/* graphlearn::error::Code values used by this library (status.h:29-49). */
#define GLX_OK 0
#define GLX_INVALID_ARGUMENT 3
#define GLX_RESOURCE_EXHAUSTED 8
#define GLX_ABORTED 10 /* ABI 4: a speculated exchange did not fit (glx_dist_ledger); redo the unconfirmed calls */
#define GLX_OUT_OF_RANGE 11
#define GLX_UNIMPLEMENTED 12
#define GLX_INTERNAL 13
#define GLX_UNAVAILABLE 14

#define GLX_PTR_HOST 0
#define GLX_PTR_DEVICE 1

/* Sampler ids; the registry names they serve are in the comments
 * (REGISTER_OPERATOR in random_sampler.cc:80, random_without_replacement_sampler.cc:79,
 * edge_weight_sampler.cc:128, topk_sampler.cc:72). */
#define GLX_SAMPLER_RANDOM 0                     /* "RandomSampler" */
#define GLX_SAMPLER_RANDOM_WITHOUT_REPLACEMENT 1 /* "RandomWithoutReplacementSampler" */
#define GLX_SAMPLER_EDGE_WEIGHT 2                /* "EdgeWeightSampler" */
#define GLX_SAMPLER_TOPK 3                       /* "TopkSampler" */
#define GLX_SAMPLER_IN_DEGREE 4                  /* "InDegreeSampler" (in_degree_sampler.cc:117); needs
                                                    glx_graph_enable_in_degree() */

/* Aggregator ids ("SumAggregator" ... sum_aggregator.cc:36, mean_aggregator.cc:64,
 * max_aggregator.cc:43, min_aggregator.cc:43, prod_aggregator.cc:43). */
#define GLX_AGG_SUM 0
#define GLX_AGG_MEAN 1
#define GLX_AGG_MAX 2
#define GLX_AGG_MIN 3
#define GLX_AGG_PROD 4

/* GLOBAL_FLAG(PaddingMode) values (constants.h:119-122, config.cc:94). */
#define GLX_PAD_REPLICATE 0
#define GLX_PAD_CIRCULAR 1

typedef struct glx_graph glx_graph;       /* one edge type: device CSR + alias table + id map */
typedef struct glx_features glx_features; /* one node type: device [V, D] float matrix + id map */

/* ---- library ------------------------------------------------------------ */
GLX_API int glx_abi_version(void);
/* Number of visible GPUs; GLX_UNAVAILABLE (and *count = 0) when there is no
 * usable HIP device.  Nothing in this library falls back to the CPU. */
GLX_API int glx_device_count(int* count);
GLX_API const char* glx_last_error(void);

/* Pins (page-locks and maps) a caller-owned host buffer so that the copies of host-pointer calls into / out
 * of it are single DMA transfers instead of bouncing through the runtime's pageable staging -- what the
 * response tensors of the C++ layer are backed by (the role of the reference's RepeatedField storage,
 * service/tensor_impl.h:72-75,196-200, on this path).  Both return GLX_UNAVAILABLE without a GPU runtime;
 * an unregistered buffer works everywhere, only slower.  A result is written directly only when the WHOLE output extent
 * lies inside one range registered HERE; memory pinned by other means is staged.  A buffer that straddles the end of a
 * registered range is the caller's error (the runtime refuses a copy across that boundary: GLX_INTERNAL, "invalid argument").
 * WHERE the memory comes from matters (ROCm 7.0, measured in round 6): register private anonymous mappings of their own
 * -- mmap(MAP_PRIVATE | MAP_ANONYMOUS), 2 MiB aligned, whole 2 MiB granules -- NOT ranges of the malloc heap.  A process
 * that has registered parts of its heap and also holds heap memory marked MADV_HUGEPAGE (numpy marks every array of
 * 4 MiB or more) gets "an illegal memory access" from later PAGEABLE host-to-device copies, anywhere in the process:
 * scripts/r06/repro/hostreg_pageable.hip shows it with the runtime alone (registered ranges cut from the heap: a fault
 * within ~50 rounds of copies; cut from mappings of their own: none in 600), unregistered or not.  The C++ layer's
 * response pool (host/src/base.cc) follows the rule; long-lived pools that never unregister are the intended use.
 * A range inside the process's brk heap is refused with GLX_INVALID_ARGUMENT (GLX_HOST_REGISTER_HEAP=1 lifts the check). */
GLX_API int glx_host_register(void* p, uint64_t bytes);
GLX_API int glx_host_unregister(void* p);

/* ---- graph storage: replaces GraphStorage::GetNeighbors / GetOutEdges /
 * GetEdgeWeight (graph_storage.h:40-57) + CompressedMemoryAdjMatrix
 * (memory_adj_matrix.cc:159-225) + AutoIndex (auto_indexing.cc:21-33). -----
 *
 * Input is the adjacency exactly as the reference exposes it after Build():
 * row r holds neighbours col[row_ptr[r] .. row_ptr[r+1]) and their edge ids
 * eid[..] IN THE REFERENCE'S ROW ORDER (weight-descending for weighted edge
 * types, memory_adj_matrix.cc:105-125).  `weight` is per CSR slot (the
 * reference stores it per edge id: memory_edge_storage.cc:97-103) or NULL for
 * an unweighted type.  `ids` maps row -> raw vertex id, or NULL when raw id v
 * is row v.  row_ptr is 64-bit (the reference's int32 offsets overflow at
 * E >= 2^31: types.h:28).  When weights are given the per-row alias tables of
 * AliasMethod::Build (alias_method.cc:57-107) are built once, on the device.
 */
GLX_API int glx_graph_create(int device, int64_t num_rows, int64_t num_edges, const int64_t* row_ptr,
                     const int64_t* col, const int64_t* eid, const float* weight,
                     const int64_t* ids, int ptr_kind, void* stream, glx_graph** out);
/* Device-side storage build from a raw edge list (the loader's output): replaces
 * LocalGraph::UpdateEdges -> GraphStorage::Add (local_graph.cc:50-64,
 * memory_graph_storage.cc:49-54), MemoryAdjMatrix::Build / Sort
 * (memory_adj_matrix.cc:60-66,105-125) and CompressedMemoryAdjMatrix::Build
 * (:169-189).  src/dst/weight[num_edges] are in insertion order, so edge id i is
 * edge i (memory_edge_storage.cc:53-57); weight may be NULL.  Rows are the distinct
 * source ids (a device hash map replaces AutoIndex).  edge_ids (may be NULL) overrides
 * the ids -- a shard that holds a subset of the edges passes their GLOBAL ids; the
 * array order is still the insertion order.  sort_by_weight != 0 orders
 * every row by weight descending like Build() with IndexOption "sort" does; ties
 * keep insertion order (the reference's std::sort leaves them unspecified).
 * The whole build (two radix sorts, run-length encode, scan, gather, alias
 * tables, id map) runs on the GPU. */
GLX_API int glx_graph_build(int device, int64_t num_edges, const int64_t* src, const int64_t* dst,
                    const float* weight, const int64_t* edge_ids, int sort_by_weight, int ptr_kind,
                    void* stream, glx_graph** out);
/* Same, with the row order spelled out.  GLX_ORDER_TIMESTAMP_ASC orders every row by the
 * edges' timestamps ascending, which is what Build() does for timestamped edge types -- it
 * takes precedence over the weight order (memory_adj_matrix.cc:60-66,129-148); ties keep
 * insertion order.  timestamp (may be NULL for the other orders) is also kept per slot
 * for timestamp filters (glx_sample_filtered). */
#define GLX_ORDER_INSERTION 0
#define GLX_ORDER_WEIGHT_DESC 1
#define GLX_ORDER_TIMESTAMP_ASC 2
GLX_API int glx_graph_build_ordered(int device, int64_t num_edges, const int64_t* src, const int64_t* dst,
                            const float* weight, const int64_t* edge_ids, const int64_t* timestamp, int order,
                            int ptr_kind, void* stream, glx_graph** out);
GLX_API void glx_graph_destroy(glx_graph* g);
GLX_API int glx_graph_info(const glx_graph* g, int64_t* num_rows, int64_t* num_edges, int* weighted,
                   int* has_id_map, int* device);
/* *packed = 1 when EdgeWeightSampler (circular padding) draws from the packed per-slot records {prob, own (nbr, eid),
 * alias partner's (nbr, eid)}: built for a weighted graph whose edge ids all fit an int32, unless GLX_EW_PACKED was "0"
 * when the graph was created.  0: it draws from the alias tables and the adjacency (same answers).  Added under 5. */
GLX_API int glx_graph_edge_weight_packed(const glx_graph* g, int* packed);
/* *bytes = the size of those records: 20, 32 or 0 (none).  A weighted graph keeps ONE table, chosen when it is built:
 *   20 -- {float prob, int32 eid_self, eid_alias, nbr_self, nbr_alias}, three to a 64-byte sector (slot g at byte
 *         (g / 3) * 64 + (g % 3) * 20): every edge id and every neighbour id fits an int32 (negative ids included)
 *         and num_edges <= 2^31;
 *   32 -- the same with int64 neighbour ids: the edge ids fit an int32;
 *    0 -- neither: the alias tables and the adjacency serve the draws.
 * GLX_EW_PACKED at the build: "0" keeps none, "32" keeps the 32-byte records where the rule would keep either,
 * anything else (or unset) is the rule above.  The answers are the same bit for bit under all three. */
GLX_API int glx_graph_edge_weight_record_bytes(const glx_graph* g, int* bytes);
/* *form = the row directory the graph keeps for its samplers, *bytes (optional) = its size.  A graph whose rows are
 * named by raw ids (every glx_graph_build graph, and glx_graph_create with ids) answers "id -> (first slot, degree)"
 * from one table laid out when it is built, in one aligned load per request row:
 *   1 (direct)   -- {uint32 start, uint32 deg} at index id for ids in [0, max_id], start = UINT32_MAX where the id is no
 *                   row: the smallest id is >= 0 and (max_id + 1) * 8 bytes are no more than the hashed form's;
 *   2 (hashed16) -- {int64 key, uint32 start, uint32 deg} in the slots of the id map (2 * num_rows rounded up to a power
 *                   of two, at least 64; 16 bytes each), INT64_MIN marking a free slot;
 *   0 (none)     -- dense ids (no id map), no rows, or num_edges >= 2^32 - 1: the id map and row_ptr answer.
 * GLX_ROW_DIR at the build: "0" keeps none, "hash" keeps the hashed form where the rule would keep either, anything else
 * (or unset) is the rule above.  The answers are the same bit for bit under all three. */
GLX_API int glx_graph_row_dir(const glx_graph* g, int* form, int64_t* bytes);
/* EdgeWeightSampler on an UNWEIGHTED edge type: the reference reads GLOBAL_FLAG(DefaultWeight) for every edge
 * (MemoryEdgeStorage::GetWeight, memory_edge_storage.cc:97-103: an id beyond the empty weight array) and builds its
 * alias row from that (edge_weight_sampler.cc:78-92) -- with the default 0.0 every prob is 0/0 = NaN, no slot takes its
 * alias and a draw is idx = (int)(float)uniform[0, deg - 1) (alias_method.cc:117-121).  This gives the graph that
 * constant weight per slot and the alias tables AliasMethod::Build makes of it (NaN rows included, bit for bit); it
 * MUTATES the handle like glx_graph_enable_in_degree: call it once, before sampling from other threads.  A graph that
 * has weights is left alone.  (ABI 5) */
GLX_API int glx_graph_enable_default_weight(glx_graph* g, float default_weight, void* stream);
/* Copy the device alias table out (parity checks against alias_method.cc:57-107). */
GLX_API int glx_graph_export_alias(const glx_graph* g, float* prob, int32_t* alias, int ptr_kind,
                           void* stream);
/* Degrees of a batch of raw ids (0 for unknown ids), as GetNeighbors().Size(). */
GLX_API int glx_graph_degrees(const glx_graph* g, const int64_t* src, int64_t n, int64_t* deg_out,
                      int ptr_kind, void* stream);
/* In-degrees of a batch of raw destination ids (0 for ids no edge points to), as
 * GraphStorage::GetInDegree (topo_statics.cc:62-69).  Needs glx_graph_enable_in_degree(g). */
GLX_API int glx_graph_in_degrees(const glx_graph* g, const int64_t* ids, int64_t n, int64_t* deg_out,
                         int ptr_kind, void* stream);

/* ---- neighbour sampling: replaces Sampler::Sample of the four samplers
 * (random_sampler.cc:33-76, random_without_replacement_sampler.cc:31-75,
 * edge_weight_sampler.cc:31-92, topk_sampler.cc:29-68) incl. the padders
 * (padder/circular_padder.h:36-66, padder/replicate_padder.h:37-56) and
 * SamplingResponse::FillWith for unknown / empty rows. --------------------
 *
 * src[batch] raw ids -> nbr_out[batch*k], eid_out[batch*k], row-major dense,
 * the layout of SamplingResponse kNodeIds / kEdgeIds (sampling_request.cc:226-251).
 * `padding_mode` and `default_neighbor_id` are the reference's global flags,
 * passed explicitly.  (`seed`, `call_counter`) select the random stream (the
 * seeding contract in DESIGN.md): the same pair gives the same output,
 * bit-for-bit, on every run and every GPU count.  Requests with a Filter go through
 * glx_sample_filtered.
 */
GLX_API int glx_sample(const glx_graph* g, int sampler, const int64_t* src, int32_t batch, int32_t k,
               int padding_mode, int64_t default_neighbor_id, uint64_t seed,
               uint64_t call_counter, int64_t* nbr_out, int64_t* eid_out, int ptr_kind,
               void* stream);

/* ---- further samplers of the registry -------------
 * InDegreeSampler (in_degree_sampler.cc:33-114) is EdgeWeightSampler with the
 * neighbour's in-degree inside this edge type as the weight (GraphStorage::
 * GetInDegree, topo_statics.cc:33-69), rebuilt per row per request in the
 * reference.  glx_graph_enable_in_degree counts the in-degrees and builds that
 * second set of alias tables once, on the device; it MUTATES the handle: call it
 * right after creation, before the handle is shared between threads. */
GLX_API int glx_graph_enable_in_degree(glx_graph* g, void* stream);

/* FullSampler (full_sampler.cc:28-97): every row returns its first
 * min(max_limit, deg) neighbours in storage order (max_limit <= 0: all) as a
 * sparse response -- SamplingResponse's segments + values (sampling_request.cc:
 * 198-224).  Two calls, like the reference's two passes:
 *   glx_sample_full_sizes  -> degrees_out[batch] (the segments) and
 *                             offsets_out[batch+1] (exclusive prefix sum; the last
 *                             entry is the total number of values);
 *   glx_sample_full        -> nbr_out / eid_out[offsets[batch]], row i at offsets[i]
 *                             (both may be NULL for an empty response, offsets[batch] == 0;
 *                             glx_sample_full_filtered likewise). */
GLX_API int glx_sample_full_sizes(const glx_graph* g, const int64_t* src, int32_t batch, int32_t max_limit,
                          int32_t* degrees_out, int64_t* offsets_out, int ptr_kind, void* stream);
GLX_API int glx_sample_full(const glx_graph* g, const int64_t* src, int32_t batch, int32_t max_limit,
                    const int64_t* offsets, int64_t* nbr_out, int64_t* eid_out, int ptr_kind,
                    void* stream);

/* Same as glx_sample, but request row i draws from the random stream of row
 * rng_rows[i] instead of row i (rng_rows == NULL: identical to glx_sample).  A
 * shard that serves a slice of a partitioned request (DistributeRunner::Run,
 * op_runner.h:60-84) passes the rows' indices in the ORIGINAL request -- the
 * Sticker values of hash_partitioner.h:69 -- so the stitched result is
 * bit-identical to the unpartitioned one for every shard count. */
GLX_API int glx_sample_ex(const glx_graph* g, int sampler, const int64_t* src, const int64_t* rng_rows,
                  int32_t batch, int32_t k, int padding_mode, int64_t default_neighbor_id,
                  uint64_t seed, uint64_t call_counter, int64_t* nbr_out, int64_t* eid_out,
                  int ptr_kind, void* stream);

/* Multi-hop driver: replaces the host-side hop loop of NeighborSampler.get
 * (graphlearn/python/sampler/neighbor_sampler.py:93-127) / a chain of sampling
 * DAG nodes (core/runner/dag_node_runner.cc:32-109).  Hop h samples fanouts[h]
 * neighbours of every vertex of hop h-1 (hop 0 = `seeds`) from graphs[h] -- one
 * edge type per hop, i.e. the meta-path -- with random stream (seed,
 * call_counter + h).  Frontiers stay on the device between hops; hop h's
 * batch * fanouts[0] * ... * fanouts[h] slots are written to nbr_out[h] /
 * eid_out[h] (eid_out, or single entries of it, may be NULL).  Equivalent to
 * num_hops glx_sample calls feeding each other. */
GLX_API int glx_sample_hops(const glx_graph* const* graphs, int32_t num_hops, int sampler,
                    const int64_t* seeds, int32_t batch, const int32_t* fanouts, int padding_mode,
                    int64_t default_neighbor_id, uint64_t seed, uint64_t call_counter,
                    int64_t* const* nbr_out, int64_t* const* eid_out, int ptr_kind, void* stream);

/* ---- sampling filters: replaces op::Filter (core/operator/sampler/filter.h:30-125,
 * filter.cc:69-229) as the samplers use it (random_sampler.cc:52-71, topk_sampler.cc:52-61,
 * random_without_replacement_sampler.cc:56-68, edge_weight_sampler.cc:55-66,94-112,
 * in_degree_sampler.cc:54-65,94-113, full_sampler.cc:66-84). ----------------------------
 * type / field carry the reference's enum values (include/constants.h:135-145).  values[batch]
 * is the filter tensor AFTER Filter::FillValues: one value per request row, in the same
 * memory kind as src.  A neighbour "hits" when its field (ID = the neighbour id, TIMESTAMP =
 * the edge's timestamp, default_timestamp when the graph has none) == / > the row's value,
 * and hits are what sampling avoids:
 *   RandomSampler   a row whose neighbours all hit is default-filled; otherwise every slot
 *                   redraws a hit up to retry_times times and then keeps it (attempt a of
 *                   slot j is draw j + a * k of the row's stream);
 *   the others      sample from the reserved positions Filter::ActOn leaves, in ITS order:
 *                   survivors keep their place, holes left by hits are refilled from the
 *                   right end, rightmost survivor first (filter.cc:83-94); TIMESTAMP +
 *                   LARGER_THAN instead keeps the prefix below values[0] -- the value of
 *                   request row 0, for every row (filter.h:107-111) -- in descending order,
 *                   and keeps nothing of a single-neighbour row (filter.cc:208-210).
 *                   EdgeWeight / InDegree rebuild the alias table over the reserved
 *                   neighbours' weights per row, like the reference; padding as before.
 * glx_sample_full_filtered: the row sizes stay those of glx_sample_full_sizes (the
 *   UNFILTERED min(limit, deg), full_sampler.cc:55-62) and the reserved neighbours are padded
 *   up to that size; a row whose neighbours all hit yields default ids (the reference's
 *   FillWith(dim2) breaks the ragged layout there).
 * filter == NULL or type == GLX_FILTER_NONE: identical to the unfiltered entry points. */
#define GLX_FILTER_NONE 0
#define GLX_FILTER_EQUAL 1
#define GLX_FILTER_LARGER_THAN 2
#define GLX_FILTER_FIELD_NONE 0
#define GLX_FILTER_FIELD_ID 1
#define GLX_FILTER_FIELD_TIMESTAMP 2
typedef struct glx_filter {
  int32_t type;
  int32_t field;
  const int64_t* values;
  int32_t retry_times;       /* GLOBAL_FLAG(SamplingRetryTimes), config.cc:108; RandomSampler only */
  int64_t default_timestamp; /* GLOBAL_FLAG(DefaultTimestamp), memory_edge_storage.cc:113-119 */
} glx_filter;
/* Per-slot timestamps for a handle made by glx_graph_create: ts_slot[num_edges] in the
 * order of `col`.  MUTATES the handle, like glx_graph_enable_in_degree. */
GLX_API int glx_graph_set_timestamps(glx_graph* g, const int64_t* ts_slot, int ptr_kind, void* stream);
GLX_API int glx_sample_filtered(const glx_graph* g, int sampler, const int64_t* src, const int64_t* rng_rows,
                                int32_t batch, int32_t k, int padding_mode, int64_t default_neighbor_id,
                                uint64_t seed, uint64_t call_counter, const glx_filter* filter,
                                int64_t* nbr_out, int64_t* eid_out, int ptr_kind, void* stream);
GLX_API int glx_sample_full_filtered(const glx_graph* g, const int64_t* src, int32_t batch, int32_t max_limit,
                                     const int64_t* offsets, int padding_mode, int64_t default_neighbor_id,
                                     const glx_filter* filter, int64_t* nbr_out, int64_t* eid_out, int ptr_kind,
                                     void* stream);

/* ---- temporal neighbour sampling: "the neighbours of v over edges that happened before t", with a cutoff of its own
 * for every request row.  An addition of this engine (added under 5).  It stands in for the sample the reference's TGN
 * loader takes per event (examples/pytorch/tgn/temporal_batch_loader.py:70-80: a topk sample of the whole interaction
 * graph, which ignores time), and answers per row what the reference's timestamp filter answers for request row 0's
 * value only (core/operator/sampler/filter.cc:74-82), over the timestamp-ascending rows that Build() lays out for a
 * timestamped edge type (core/graph/storage/memory_adj_matrix.cc:129-148). -------------------------------------------
 *
 * Request row i (raw id src[i], cutoff t = cutoff[i]): c = the number of slots of the row whose timestamp is < t
 * (<= t when inclusive != 0).  Rows are timestamp-ascending with ties in insertion order, so these are the row's first
 * c slots; an unknown id has c = 0.  INT64_MAX with `inclusive` selects the whole row, INT64_MIN nothing.
 *   GLX_TEMPORAL_RECENT   slot j < min(k, c) of the answer is CSR slot c - 1 - j (latest first), the other slots are
 *                         default-filled: (default_neighbor_id, -1, default_timestamp); cnt_out[i] = min(k, c).
 *   GLX_TEMPORAL_UNIFORM  c > 0: slot j is CSR slot bounded(draw j of row stream rr, c) under (seed, call_counter),
 *                         rr = rng_rows ? rng_rows[i] : i -- the draw of RandomSampler (random_sampler.cc:61-63) with
 *                         the prefix length in place of the degree -- and cnt_out[i] = k.  c == 0: the row is
 *                         default-filled and cnt_out[i] = 0.
 * nbr_out / eid_out / ts_out are [batch, k], row-major and dense, every element written; eid_out, ts_out and cnt_out
 * may each be NULL.  There are no padding modes: a temporal consumer needs the mask.  batch == 0 is a no-op; k >= 1.
 * The graph must keep per-slot timestamps (glx_graph_build_ordered with GLX_ORDER_TIMESTAMP_ASC, or
 * glx_graph_set_timestamps on a glx_graph_create handle -- whose rows the CALLER keeps ascending; if they are not,
 * the answer is unspecified but every load stays inside the row).  The same bits on every call; no atomics.
 *
 * glx_sample_temporal_hops: request row r of hop h >= 1 is slot r of hop h - 1 -- its id is that slot's neighbour and
 * its cutoff that slot's edge timestamp (a neighbour's history before the interaction that reached it) -- and draws
 * from graphs[h] with stream (seed, call_counter + h).  A default-filled parent slot yields a default-filled row with
 * cnt = 0 whatever default_neighbor_id is.  Frontiers stay on the device; the result equals num_hops single calls
 * chained by that rule.  eid_out / ts_out / cnt_out, or single entries of them, may be NULL -- except that with device
 * pointers the outputs ARE the frontiers, so every hop but the last needs its ts_out and cnt_out.  num_hops <= 8. */
#define GLX_TEMPORAL_RECENT 0
#define GLX_TEMPORAL_UNIFORM 1
GLX_API int glx_graph_has_timestamps(const glx_graph* g, int* has);
GLX_API int glx_sample_temporal(const glx_graph* g, int strategy, const int64_t* src, const int64_t* cutoff,
                                const int64_t* rng_rows, int32_t batch, int32_t k, int inclusive,
                                int64_t default_neighbor_id, int64_t default_timestamp, uint64_t seed,
                                uint64_t call_counter, int64_t* nbr_out, int64_t* eid_out, int64_t* ts_out,
                                int32_t* cnt_out, int ptr_kind, void* stream);
GLX_API int glx_sample_temporal_hops(const glx_graph* const* graphs, int32_t num_hops, int strategy,
                                     const int64_t* seeds, const int64_t* cutoff, int32_t batch,
                                     const int32_t* fanouts, int inclusive, int64_t default_neighbor_id,
                                     int64_t default_timestamp, uint64_t seed, uint64_t call_counter,
                                     int64_t* const* nbr_out, int64_t* const* eid_out, int64_t* const* ts_out,
                                     int32_t* const* cnt_out, int ptr_kind, void* stream);

/* ---- random walks: replaces the "RandomWalk" operator (core/operator/random_walk/
 * random_walk.cc:30-276) -- DeepWalk (:168-190) when p = q = 1 within 32 FLT_EPSILON
 * (RandomWalkRequest::IsDeepWalk, random_walk_request.cc:152-160), node2vec otherwise
 * (WeightedRandomWalk / WeightedRandomWalkKernel, :192-272). ----------------------------
 * walks_out[batch * walk_len], row i = the walk_len vertices visited from seeds[i] (the
 * response layout, :121-127).  A vertex without out-edges yields default_neighbor_id, and
 * the walk goes on from THAT id, like the reference.  node2vec looks at the first
 * min(deg, full_nbr_num) neighbours only (GLOBAL_FLAG(DefaultFullNbrNum), <= 2048 here),
 * weighs an edge by 1/(p + 1e-6) when it returns to the parent, by 1 when it leads to one of
 * the parent's first full_nbr_num neighbours, by 1/(q + 1e-6) otherwise, and draws once from
 * the alias table of those weights; the first step's parent is the seed itself, without
 * neighbours (random_walk_request.cc:120-131).  default_weight stands in for the edge
 * weights of an unweighted graph (GLOBAL_FLAG(DefaultWeight)).  Step t of walker i uses draw 0
 * of the stream (seed, call_counter + t, i).  The reference does not advance its cursor
 * into the parents' neighbour lists past a walker that is stuck (:214-226), which shifts the
 * windows of all later walkers of the batch: reproduced (round 4) -- walks equal the reference's
 * also on graphs with dead ends. */
GLX_API int glx_random_walk(const glx_graph* g, const int64_t* seeds, int32_t batch, int32_t walk_len, float p,
                            float q, int32_t full_nbr_num, float default_weight, int64_t default_neighbor_id,
                            uint64_t seed, uint64_t call_counter, int64_t* walks_out, int ptr_kind, void* stream);

/* ---- node features: replaces NodeStorage::GetAttribute()->GetFloats()
 * (node_storage.h:51-54, compressed_memory_node_storage.cc:149-176). -------
 * X is [num_rows, dim] row-major float32 (SideInfo.f_num == dim). */
GLX_API int glx_features_create(int device, int64_t num_rows, int32_t dim, const float* X,
                        const int64_t* ids, int ptr_kind, void* stream, glx_features** out);
/* Non-owning view of a device-resident [num_rows, dim] matrix with the dense id
 * map (id v is row v): lets glx_aggregate reduce rows that arrived from other
 * shards (the halo exchange) without a copy.  X must outlive the handle. */
GLX_API int glx_features_view(int device, int64_t num_rows, int32_t dim, const float* X_device,
                      glx_features** out);
GLX_API void glx_features_destroy(glx_features* f);
GLX_API int glx_features_info(const glx_features* f, int64_t* num_rows, int32_t* dim, int* has_id_map,
                      int* device);
/* Storage types of a feature table.  Aggregation, lookup and the KNN searches read the stored elements, upcast them
 * to float32 (exact) and accumulate and write float32 in the same order as for a float32 table: a half or float8
 * table's results equal those of the float32 table holding the upcast values, bit for bit.
 * float8 (OCP 8-bit floating point, one byte per element: a quarter of the float32 bytes; no FNUZ encodings, no
 * per-row or per-column scale -- the stored byte IS the value):
 *   conversion  float32 -> float8 rounds to nearest even in integer arithmetic, bit-identical to
 *               torch.Tensor.to(torch.float8_e4m3fn / torch.float8_e5m2) of a contiguous CPU tensor.
 *               e4m3fn has NO infinity: OVERFLOW BECOMES NaN, NOT THE LARGEST NUMBER.  |x| up to 464 (the tie, to
 *               even) is 448 (0x7E); everything above, +-inf and every NaN is sign | 0x7F.  Features outside
 *               [-448, 448] must be normalised before they are stored as e4m3.  Below, 2^-10 (half the smallest
 *               subnormal, a tie) is zero and the sign of a zero is kept.
 *               e5m2: up to 57344 is finite (0x7B); 61440 (the tie) and above is sign | 0x7C (inf); NaN is sign | 0x7F.
 *   upcast      exact: every non-NaN code gives the float32 of torch's .float(); a NaN code (e4m3 0x7F, 0xFF; e5m2
 *               0x7D-0x7F, 0xFD-0xFF) gives a NaN whose sign and payload are unspecified.
 *   serves      glx_lookup, glx_aggregate (every operator), glx_aggregate_arg, glx_plan, the exact / IVF-Flat / IVF-PQ
 *               KNN (queries stay float32).  Refuses, naming the dtype: glx_dist_store_create and the hot-row replica;
 *               the training-path entry points take float32 matrices only. */
#define GLX_DTYPE_F32 0
#define GLX_DTYPE_BF16 1
#define GLX_DTYPE_F16 2
#define GLX_DTYPE_F8E4M3 8 /* OCP float8_e4m3fn */
#define GLX_DTYPE_F8E5M2 9 /* OCP float8_e5m2 */
/* glx_features_create with a storage type.  X holds [num_rows, dim] elements of x_dtype.  x_dtype == store_dtype
 * copies them as they are; x_dtype == GLX_DTYPE_F32 with a half or float8 store_dtype converts on the device while
 * the rows are placed (float8: the rule above; half): round to nearest even, overflow to +-inf, bit-identical to torch.Tensor.to() of a contiguous CPU
 * tensor for every input, NaN included (bfloat16: 0xFFFF for every NaN; float16: sign | 0x7E00 | payload >> 13).
 * Every other pair is GLX_INVALID_ARGUMENT.
 * glx_features_create(...) is glx_features_create_ex(..., GLX_DTYPE_F32, GLX_DTYPE_F32, ...). */
GLX_API int glx_features_create_ex(int device, int64_t num_rows, int32_t dim, const void* X, int x_dtype,
                                   int store_dtype, const int64_t* ids, int ptr_kind, void* stream, glx_features** out);
/* glx_features_view of a device-resident [num_rows, dim] matrix of `dtype` elements. */
GLX_API int glx_features_view_ex(int device, int64_t num_rows, int32_t dim, const void* X_device, int dtype,
                                 glx_features** out);
GLX_API int glx_features_dtype(const glx_features* f, int* dtype);
/* The upload's conversion on the host, without a GPU: dst[i] = src[i] converted to store_dtype for i < n, by the very
 * functions the device runs while it places the rows of glx_features_create_ex -- so the rounding rule can be checked
 * against torch.Tensor.to() anywhere.  store_dtype: GLX_DTYPE_BF16 / _F16 (dst: n x 2 bytes), _F8E4M3 / _F8E5M2 (n
 * bytes), _F32 (copies n x 4 bytes).  An addition of this engine: it stands in for the float -> storage step of
 * NodeStorage::Add (compressed_memory_node_storage.cc:99-101), which keeps float32.  Pure host code, no HIP call. */
GLX_API int glx_features_convert_host(const float* src, int64_t n, int store_dtype, void* dst);

/* ---- exact KNN search: replaces the KnnOperator on the reference's flat index -- FlatKnnIndex::Search
 * (contrib/knn/flat_index.cc:26-55), KnnRequest / KnnResponse and KnnResponse::Merge (contrib/knn/knn_request.cc:26-50,
 * 186-202) and the index build (contrib/knn/builder.cc:23-52) -- without faiss: the flat index IS the glx_features table
 * as it lies in device memory, no second copy.  ivfflat / ivfpq / gpu_* index types are answered exactly by this search.
 * For a query q (dim float32 values) and a stored row x of a float32, bfloat16, float16 or float8 table:
 *   upcast   a half or float8 element is upcast exactly to float32 first.
 *   ip       = +0.0f, then ip = fmaf(q[c], x[c], ip) for c = 0 .. dim-1 ascending: ONE chain over all columns, one
 *            rounding per step (the numerics of v_mfma_f32_32x32x2_f32, of v_mfma_f32_16x16x4_f32 and of a VALU fmaf
 *            loop alike; no split-K, no second accumulator over the columns).
 *   GLX_KNN_IP  dist = ip; larger is better.
 *   GLX_KNN_L2  qn, xn: the same chain of the vector with itself; d = fmaf(-2.0f, ip, fadd_rn(qn, xn));
 *            dist = d < 0 ? +0.0f : d (a NaN stays a NaN): the squared distance by expansion, as faiss's flat index
 *            computes it for batches; smaller is better.  xn is computed once per owned table, on the first L2
 *            search (stream-ordered, guarded for concurrent callers), and kept with the glx_features object; per
 *            search for a view (glx_features_view*), whose rows are the caller's to rewrite between calls.
 *   order    a better dist first; equal dist (float equality, +0.0f == -0.0f): the smaller storage row (insertion order)
 *            first; a NaN dist is worse than every number, NaNs among themselves by row.  Which NaN a NaN dist is, is
 *            the hardware's.
 *   output   row i of ids_out / dist_out ([num_queries, k]) holds the k best rows under that order, best first; ids_out
 *            holds node ids -- the id the row was created with (ids_[row], flat_index.cc:52-54), the row number for a
 *            table without an id map.  With k > num_rows the remaining slots are id = -1, dist = -inf (IP) / +inf (L2):
 *            faiss's padding, without the reference's ids_[-1] read.
 * Every element of both outputs is written; the same inputs give the same bits on every call; no float atomics; the
 * table's stride and swizzle are honoured.  Limits (else GLX_INVALID_ARGUMENT): 1 <= k <= 1024; num_queries >= 0 (0 is
 * a no-op success); num_rows < 2^31; num_queries * k < 2^31; one GPU; not under graph capture.
 * glx_tune: "knn_chunk_rows" (GLX_KNN_CHUNK_ROWS: table rows per chunk), "knn_query_block" (GLX_KNN_QUERY_BLOCK: queries
 * per pass over the table); results are bit-identical under every setting.
 * glx_knn_merge is KnnResponse::Merge: ids / dist are [num_parts, num_queries, k]; the output is the k best of the
 * num_parts * k entries of each query under the same order on dist, ties to the lower part, then to the earlier
 * position in the part; id = -1 entries are worst (absent).  Merging the searches of consecutive row ranges of one
 * table reproduces the whole-table search bit for bit (the reference's heap leaves the tie order to chance).
 * num_parts >= 1, num_parts * k < 2^31. */
#define GLX_KNN_L2 0 /* the reference's KnnMetric values: contrib/knn/config.h:21-23 with flat_index.cc:27-28 */
#define GLX_KNN_IP 1
GLX_API int glx_knn_search(const glx_features* f, int metric, const float* queries, int32_t num_queries, int32_t k,
                           int64_t* ids_out, float* dist_out, int ptr_kind, void* stream);
GLX_API int glx_knn_merge(int device, int metric, int32_t num_parts, const int64_t* ids, const float* dist,
                          int32_t num_queries, int32_t k, int64_t* ids_out, float* dist_out, int ptr_kind,
                          void* stream);

/* ---- IVF-Flat index: probed KNN search, the reference's IndexOption(index_type = "ivfflat", nlist, nprobe) --
 * IVFFlatKnnIndex (contrib/knn/ivfflat_index.cc:25-55) as the index factory makes it (contrib/knn/index_factory.cc:32-34)
 * -- without faiss and without a second copy of the table.  A glx_knn_ivf belongs to ONE glx_features table of N rows
 * (float32 / bfloat16 / float16, owned or a view, id-mapped, swizzled: whatever glx_knn_search serves), which must
 * outlive it.  It holds centroids [nlist, dim] float32, list_ptr [nlist + 1] and list_rows [N]: the storage rows of every
 * list, ascending within a list, 4 bytes each; every row is in exactly one list.  Scores always come from the table
 * itself: a returned dist is the contract distance of that row as the table holds it at the call (an index over a view
 * whose rows changed since the build has stale lists, never stale distances).
 * Build (deterministic: no RNG, no float atomic; two builds give the same bits):
 *   sample   T = train_rows clamped to [nlist, N]; train_rows = 0 means min(N, 256 * nlist).  Sample element t is
 *            storage row floor(t * N / T), upcast exactly to float32.
 *   start    centroids_init [nlist, dim] float32 (host or device by ptr_kind) when given, else sample element
 *            floor(i * T / nlist) for centroid i.
 *   assign   a row goes to its first centroid under glx_knn_search's contract with GLX_KNN_L2, k = 1, the row as the
 *            query and the centroids as the table: the nearest, a tie to the lower centroid, NaN distances last by
 *            centroid.
 *   update   niter (>= 0) Lloyd iterations, each an assign of the sample followed by: a centroid with n >= 1 sample
 *            rows becomes acc / (float)n where acc = +0.0f and then acc = fadd_rn(acc, row) in ascending storage row
 *            (the bits of glx_aggregate's MeanAggregator over those rows); a centroid with no row keeps its value.
 *   lists    all N rows are assigned against the final centroids; list_rows is the stable sort of the rows by list.
 *            niter = 0 with centroids_init is "assign only".
 *   limits   1 <= nlist <= min(N, 65536), niter >= 0, train_rows >= 0; synchronises `stream` before it returns.
 * Search: the probe set of a query is every list when nprobe == nlist (no coarse step), else the lists that
 * glx_knn_search names for the query over the centroids with k = nprobe under the search's own metric, in that order
 * (1 <= nprobe <= 1024 then).  The result is the k best rows among the rows of the probed lists under glx_knn_search's
 * contract word for word -- the same ip chain, the same L2 formula with the same qn / xn, a better dist first, then the
 * smaller storage row, NaN last by row, ids by the table's row -> id rule, slots beyond the number of candidates
 * id = -1 and dist = -inf (IP) / +inf (L2).  Hence nprobe == nlist equals glx_knn_search bit for bit, and because the
 * probe sets are nested in nprobe the set of true top-k rows a search finds never shrinks as nprobe grows.
 * Limits (else GLX_INVALID_ARGUMENT): 1 <= k <= 1024; 1 <= nprobe <= nlist; num_queries >= 0 (0 is a no-op success);
 * num_queries * k < 2^31 and num_queries * nprobe < 2^31; float32 queries; one GPU; not under graph capture.  No float
 * atomics and no counters: the same inputs give the same bits on every call.  glx_tune "knn_query_block" may shrink
 * the queries served per pass (never grow them past the 256 MiB workspace budget); the bits do not depend on it.
 * glx_knn_ivf_info: any output may be NULL; longest_list in rows; device_bytes of centroids + list_ptr + list_rows.
 * glx_knn_ivf_export: centroids_out [nlist, dim] float32, list_ptr_out [nlist + 1] int64, list_rows_out [N] int64, to
 * host or device by ptr_kind; any of them may be NULL. */
typedef struct glx_knn_ivf glx_knn_ivf;
GLX_API int glx_knn_ivf_build(const glx_features* f, int32_t nlist, int32_t niter, int64_t train_rows,
                              const float* centroids_init, int ptr_kind, void* stream, glx_knn_ivf** out);
GLX_API int glx_knn_ivf_search(const glx_knn_ivf* index, int metric, const float* queries, int32_t num_queries, int32_t k,
                               int32_t nprobe, int64_t* ids_out, float* dist_out, int ptr_kind, void* stream);
GLX_API int glx_knn_ivf_info(const glx_knn_ivf* index, int32_t* nlist, int32_t* dim, int64_t* num_rows,
                             int64_t* longest_list, int64_t* device_bytes);
GLX_API int glx_knn_ivf_export(const glx_knn_ivf* index, float* centroids_out, int64_t* list_ptr_out,
                               int64_t* list_rows_out, int ptr_kind, void* stream);
GLX_API void glx_knn_ivf_destroy(glx_knn_ivf* index);

/* ---- IVF-PQ index: coded scan and exact re-rank, the reference's IndexOption(index_type = "ivfpq", nlist, nprobe, m) --
 * IVFPQKnnIndex (contrib/knn/ivfpq_index.cc:25-56: faiss::IndexIVFPQ with 8 bits per sub-quantiser) as the index factory
 * makes it (contrib/knn/index_factory.cc:35-37; the gpu_ivfpq form: index_factory.cc:43-45, gpu_ivfpq_index.cc:30-60)
 * -- without faiss and without a second copy of the table.  A glx_knn_ivfpq sits on ONE glx_knn_ivf, which supplies
 * the coarse centroids and the lists and must outlive it (and so must that index's table).  It adds m codebooks and
 * one m-byte code per row.  "The contract" below is glx_knn_search's: the one ascending fmaf chain ip, L2 as
 * max(0, fmaf(-2, ip, qn + xn)) with a NaN kept, and the order better dist first, then the smaller row, NaN last by row.
 *   shape    1 <= m <= 64, dim % m == 0, dsub = dim / m; every sub-quantiser has 256 codewords (8 bits, fixed);
 *            num_rows >= 256.  Codebooks [m, 256, dsub] float32; codes [N, m] uint8 in LIST order: position p belongs
 *            to storage row list_rows[p] of the IVF index.
 *   residual a row x in list l has r[c] = fsub_rn(x[c], centroid_l[c]), a half element upcast exactly first.
 *   train    (deterministic) T = train_rows clamped to [256, N]; train_rows = 0 means min(N, 65536).  Sample element t
 *            is storage row floor(t * N / T) (glx_knn_ivf_build's rule).  R_j is the [T, dsub] float32 matrix of the
 *            sample's residual columns j * dsub .. (j + 1) * dsub - 1.  Codebook j is, bit for bit, the centroids that
 *            glx_knn_ivf_build returns for a float32 table holding R_j with nlist = 256, the same niter and
 *            train_rows = T: initial codeword i is R_j[floor(i * T / 256)], assignment is the contract's L2 search with
 *            k = 1 (ties to the lower codeword), the update is the sequential float32 mean in ascending sample order,
 *            an empty codeword keeps its value.  codebooks_init [m, 256, dsub] (host or device by ptr_kind) replaces
 *            the initial codewords; codebooks_init with niter = 0 is "encode only".
 *   encode   code j of each of the N rows is its first codeword under the contract with GLX_KNN_L2 and k = 1, the row's
 *            residual sub-vector j as the query and codebook j as the table.
 *   adc      the score of query q against list position p of probed list l.
 *            GLX_KNN_IP: adc = ip(q, centroid_l), the contract chain over all dim columns, then
 *            adc = fadd_rn(adc, lut[j][code[p][j]]) for j = 0 .. m-1 ascending; lut[j][c] is the contract ip of q's
 *            sub-vector j with codeword c.
 *            GLX_KNN_L2: rq[c] = fsub_rn(q[c], centroid_l[c]); adc = +0.0f, then the same ascending fadd_rn chain;
 *            lut[j][c] is the contract L2 distance (expansion form, clamped at +0.0f, NaN kept) of rq's sub-vector j
 *            to codeword c, the query-side norm the chain of that sub-vector with itself, the codeword norm the chain
 *            of the codeword with itself (computed once at build).
 *            ADC order: the contract's order applied to adc -- a better adc first, then the smaller storage row, NaN
 *            last by row.
 *   search   the probe sets are exactly glx_knn_ivf_search's (every list when nprobe == nlist, else the coarse search
 *            with k = nprobe under the search's own metric).
 *            refine = 0: the k best candidates by ADC order; dist_out holds adc (which NaN a NaN adc is, is unspecified);
 *            ids by the table's row -> id rule; padding id = -1 with dist = -inf (IP) / +inf (L2).
 *            k <= refine <= 1024: the R = refine best candidates by ADC order are re-scored from the TABLE with the
 *            contract distance (the same qn / xn as glx_knn_ivf_search, xn per search for a view) and the k best of
 *            those under glx_knn_search's order are returned with the same padding: every returned dist is the exact
 *            search's dist of that row, bit for bit.  When the probed lists hold at most R rows the answer equals
 *            glx_knn_ivf_search bit for bit, and with nprobe == nlist on top of that glx_knn_search.  The R best sets
 *            are nested in R, so the set of true top-k rows found never shrinks as refine grows at a fixed nprobe.
 *   limits   (else GLX_INVALID_ARGUMENT) 1 <= k <= 1024; refine == 0 or k <= refine <= 1024; nprobe as
 *            glx_knn_ivf_search; num_queries >= 0 (0 is a no-op success); num_queries * max(k, refine) < 2^31; float32
 *            queries; one GPU; not under graph capture.  glx_knn_ivfpq_build synchronises `stream` before it returns.
 *   stale    codes, like lists, do not follow rows rewritten under a view; distances returned with refine > 0 are
 *            still never stale.
 * No RNG, no float atomics, no counters: the same inputs give the same bits on every call.  glx_tune "knn_query_block"
 * may shrink the queries served per pass (the workspace stays under the flat search's 256 MiB budget); the bits do not
 * depend on it.
 * glx_knn_ivfpq_info: any output may be NULL; device_bytes of what the index holds on the device: the codebooks (kept
 * twice, row-major and codeword-minor) + the codeword norms + the codes.
 * glx_knn_ivfpq_export: codebooks_out [m, 256, dsub] float32, codes_out [N, m] uint8, to host or device by ptr_kind;
 * either may be NULL. */
typedef struct glx_knn_ivfpq glx_knn_ivfpq;
GLX_API int glx_knn_ivfpq_build(const glx_knn_ivf* ivf, int32_t m, int32_t niter, int64_t train_rows,
                                const float* codebooks_init, int ptr_kind, void* stream, glx_knn_ivfpq** out);
GLX_API int glx_knn_ivfpq_search(const glx_knn_ivfpq* index, int metric, const float* queries, int32_t num_queries,
                                 int32_t k, int32_t nprobe, int32_t refine, int64_t* ids_out, float* dist_out,
                                 int ptr_kind, void* stream);
GLX_API int glx_knn_ivfpq_info(const glx_knn_ivfpq* index, int32_t* m, int32_t* dsub, int64_t* num_rows,
                               int64_t* device_bytes);
GLX_API int glx_knn_ivfpq_export(const glx_knn_ivfpq* index, float* codebooks_out, uint8_t* codes_out, int ptr_kind,
                                 void* stream);
GLX_API void glx_knn_ivfpq_destroy(glx_knn_ivfpq* index);

/* ---- aggregation: replaces Aggregator::Aggregate (aggregator.cc:25-59) with
 * Sum/Mean/Max/Min/Prod Init/Agg/Final (sum_aggregator.cc:25-33,
 * mean_aggregator.cc:26-61, max_aggregator.cc:26-40, min_aggregator.cc,
 * prod_aggregator.cc). ---------------------------------------------------
 * node_ids[num_ids], segment_ids[num_ids] (consumed with the reference's
 * cursor rule, aggregating_request.cc:86-105) -> emb_out[num_segments*dim],
 * cnt_out[num_segments].  Unknown ids contribute a row of `default_attr`;
 * empty segments are `default_attr` (GLOBAL_FLAG(DefaultFloatAttribute)).
 * Each output element is accumulated in the reference's left-to-right order,
 * so results are bit-identical to the reference for every op.  segment_ids == NULL
 * means num_segments equal segments of num_ids / num_segments consecutive ids -- the
 * layout of a dense sampler response (segment i = the neighbours of request row i):
 * the segment bookkeeping kernels and the read of the segment ids are skipped.  Device-pointer
 * callers get the float4 path when dim % 4 == 0 and emb_out (and a view's X) are
 * 16-byte aligned; any other alignment silently takes the scalar path. */
GLX_API int glx_aggregate(const glx_features* f, int op, const int64_t* node_ids,
                  const int32_t* segment_ids, int32_t num_ids, int32_t num_segments,
                  float default_attr, float* emb_out, int32_t* cnt_out, int ptr_kind,
                  void* stream);

/* ---- differentiable aggregation: the gradient of glx_aggregate with respect to the table rows.  The reference's
 * model layers sit on differentiable segment reductions (python/nn/tf/layers/sage_conv.py:69-73: unsorted_segment_sum /
 * unsorted_segment_mean; gcn_conv.py:73); its operator API (aggregator.cc:25-59) has no backward to mirror. -----------
 * glx_aggregate_arg: glx_aggregate for GLX_AGG_MAX / GLX_AGG_MIN (any other op: GLX_INVALID_ARGUMENT) that also
 * records where each extreme came from.  emb_out and cnt_out equal glx_aggregate's bit for bit, for every storage type
 * and id map of `f`.  arg_out[num_segments * dim]: the request position whose element the fold's select (Max:
 * (l < r) ? r : l, max_aggregator.cc:26-40) last moved into the accumulator -- the FIRST position that attains the
 * extreme -- or -1 when nothing replaced the start value (every element <= -37 for Max, an empty segment, a NaN the
 * comparison never selects).  A default-filled position (unknown id) can be the argument. */
GLX_API int glx_aggregate_arg(const glx_features* f, int op, const int64_t* node_ids, const int32_t* segment_ids,
                              int32_t num_ids, int32_t num_segments, float default_attr, float* emb_out,
                              int32_t* cnt_out, int32_t* arg_out, int ptr_kind, void* stream);
/* glx_aggregate_backward: grad_x[num_rows * dim] from grad_out[num_segments * dim], for Sum / Mean / Max / Min over a
 * float32 table with dense ids (GLX_AGG_PROD: GLX_INVALID_ARGUMENT -- its gradient divides by the element).
 *   rows[num_ids]       the request's ids, i.e. row indices into the [num_rows, dim] table
 *   cnt[num_segments]   the counts the forward returned: segment s is positions [sum(cnt[:s]), sum(cnt[:s]) + cnt[s]),
 *                       what the forward's cursor consumed (aggregating_request.cc:86-105); positions from sum(cnt) on
 *                       give nothing.  NULL: the implied layout, num_segments segments of num_ids / num_segments
 *                       positions (a remainder gives nothing)
 *   arg                 Max / Min: what glx_aggregate_arg recorded (NULL: GLX_INVALID_ARGUMENT); ignored otherwise
 * A position whose row is outside [0, num_rows) contributed the default row and gives nothing.  grad_x[r, c] starts at
 * +0.0f and adds one float32 term per consumed position p with rows[p] == r, in ascending p: grad_out[s(p), c] (Sum),
 * grad_out[s(p), c] / float(cnt[s(p)]) (Mean), grad_out[s(p), c] when arg[s(p), c] == p (Max / Min).  EVERY row of
 * grad_x is written (rows nobody references: zeros); the call overwrites and never accumulates.  No float atomics: the
 * result is a function of the inputs alone, bit for bit (a stable sort by row, then one lane group per row).
 * A device-pointer call only enqueues work; the workspace comes from the calling thread's per-(device, stream) cache. */
GLX_API int glx_aggregate_backward(int device, int op, const int64_t* rows, const int32_t* cnt, const int32_t* arg,
                                   int32_t num_ids, int32_t num_segments, int64_t num_rows, int32_t dim,
                                   const float* grad_out, float* grad_x, int ptr_kind, void* stream);

/* ---- weighted aggregation: a per-position, optionally multi-head, weighted Sum / Mean over segments of gathered rows,
 * with both gradients.  The reduce under the reference's GCN layer (python/nn/tf/layers/gcn_conv.py:52-73: every
 * neighbour row scaled by an edge coefficient before the segment sum) and its GAT layers (gat_conv.py:96-110,
 * ego_gat_conv.py:98-103: a learned attention coefficient per neighbour and head). ------------------------------------
 * Common to the three entry points:
 *   x[num_rows * dim]      float32, row-major; rows are dense indices into it
 *   rows[num_ids]          int64; a position whose row is outside [0, num_rows) reads a row of default_attr
 *   w[num_ids * heads]     float32; heads >= 1, dim % heads == 0, C = dim / heads; column c belongs to head c / C
 *   cnt[num_segments]      segment s is positions [sum(cnt[:s]), sum(cnt[:s]) + cnt[s]) of the counts clamped at 0;
 *                          positions from sum(cnt) on are not consumed.  Counts that promise more than num_ids
 *                          positions are cut at num_ids: count(s) below is the number of positions segment s really
 *                          has (cnt[s] for a well-formed request), and a segment cut to nothing is empty.  NULL: the
 *                          implied layout, num_segments segments of num_ids / num_segments positions (a remainder is
 *                          not consumed)
 *   op                     GLX_AGG_SUM or GLX_AGG_MEAN; Max / Min / Prod: GLX_INVALID_ARGUMENT, the message names the op
 * Arguments are checked before any device use; num_rows < 2^31, num_ids * heads and num_segments * dim <= INT32_MAX.
 * A device-pointer call only enqueues work; the workspace comes from the calling thread's per-(device, stream) cache.
 * No float atomics anywhere.
 *
 * glx_aggregate_weighted (bit-exact contract): for segment s and column c the accumulator starts where glx_aggregate's
 * Sum starts (+0.0f); for each consumed position p of s in ascending order
 *     acc = fadd_rn(acc, fmul_rn(w[p, head(c)], xrow(p)[c]))
 * -- two roundings, never contracted into an FMA under any build flag.  Mean then divides by float(count(s)) exactly as
 * glx_aggregate's Mean
 * does; an empty segment is default_attr.  With every weight 1.0f and heads == 1 emb_out equals glx_aggregate on a
 * glx_features_view of x bit for bit (Sum and Mean; signed zeros and non-finite rows included). */
GLX_API int glx_aggregate_weighted(int device, int op, const float* x, int64_t num_rows, int32_t dim,
                                   const int64_t* rows, const float* w, int32_t heads, const int32_t* cnt,
                                   int32_t num_ids, int32_t num_segments, float default_attr, float* emb_out,
                                   int ptr_kind, void* stream);
/* glx_aggregate_weighted_backward_x (bit-exact contract): glx_aggregate_backward's contract with one more factor.
 * grad_x[r, c] starts at +0.0f and, for each consumed position p with rows[p] == r in ascending p, becomes
 *     fadd_rn(grad_x[r, c], fmul_rn(w[p, head(c)], t)),  t = grad_out[s(p), c] (Sum), grad_out[s(p), c] / float(count(s(p))) (Mean).
 * EVERY row of grad_x[num_rows * dim] is written; the call overwrites.  (A stable sort by row shared with
 * glx_aggregate_backward, then one lane group per row.) */
GLX_API int glx_aggregate_weighted_backward_x(int device, int op, const int64_t* rows, const float* w, int32_t heads,
                                              const int32_t* cnt, int32_t num_ids, int32_t num_segments,
                                              int64_t num_rows, int32_t dim, const float* grad_out, float* grad_x,
                                              int ptr_kind, void* stream);
/* glx_aggregate_weighted_backward_w (tolerance contract): grad_w[p, h] = sum over the columns c of head h of
 * grad_out[s(p), c] * xrow(p)[c], divided by float(count(s(p))) for Mean; a position that was not consumed gets +0.0f;
 * EVERY element of grad_w[num_ids * heads] is written.  One lane group per position with a fixed lane-to-column mapping
 * and a fixed cross-lane tree: the same inputs give the same bits on every run.  The ORDER of the sum over the columns
 * is the mapping's and not part of the contract; for any order of a C-term float32 dot product
 *     |grad_w - exact| <= C * 2^-23 * sum_c |grad_out * x| + 2^-126. */
GLX_API int glx_aggregate_weighted_backward_w(int device, int op, const float* x, int64_t num_rows, int32_t dim,
                                              const int64_t* rows, int32_t heads, const int32_t* cnt, int32_t num_ids,
                                              int32_t num_segments, float default_attr, const float* grad_out,
                                              float* grad_w, int ptr_kind, void* stream);

/* ---- ragged segment softmax: attention logits normalised over the segments of a counts= request, with its gradient.
 * The reference's GAT layer calls unsorted_segment_softmax (python/nn/tf/utils/softmax.py:24-50) and then
 * unsorted_segment_sum(nbr * alpha) (gat_conv.py:101-112); the second half is glx_aggregate_weighted. ----------------
 * Common to the two entry points:
 *   e, alpha, grad_alpha, alpha_out, grad_e   [num_ids * heads] float32, row-major [num_ids, heads]; heads >= 1
 *   cnt[num_segments]      glx_aggregate_weighted's layout: counts clamped at 0, segment s is positions
 *                          [sum(cnt[:s]), sum(cnt[:s]) + cnt[s]) cut at num_ids, positions from sum(cnt) on are not
 *                          consumed; NULL: the implied layout of num_ids / num_segments positions per segment (a
 *                          remainder is not consumed).  k = count(s) below is what segment s really has.
 * Arguments are checked before any device use; num_ids * heads <= INT32_MAX.  A device-pointer call only enqueues
 * work; the workspace comes from the calling thread's per-(device, stream) cache.  EVERY element of the output is
 * written: a position that is not consumed gets +0.0f (an empty segment has no position of its own).  No atomics: one
 * lane group (a whole workgroup for a long segment) reduces each (segment, head) with a fixed mapping and tree, so the
 * same inputs give the same bits on every call; the ORDER of the sums is the mapping's and not part of the contract.
 *
 * glx_segment_softmax: independently for each (segment s, head h), m = max_p e[p, h] and
 *     alpha[p, h] = expf(e[p, h] - m) / sum_q expf(e[q, h] - m)
 * with the accurate expf, a correctly rounded division and no epsilon.  Exact: k == 1 with a finite logit is 1.0f; k
 * equal finite logits are 1.0f / (float)k; a -inf logit among finite ones is +0.0f; the whole (s, h) column is NaN when
 * a logit of it is NaN or +inf or all of them are -inf (torch.softmax's answers); only e - m enters, so a shift of a
 * segment's logits that is exact in float32 changes no bit.  Otherwise, against the float64 value of the float32 inputs,
 * with d_p = e_p - m and E the ulp error of expf:
 *     |alpha - exact| <= exact * (2 |d_p| + 2 k + 4 E + 4) * 2^-24 + 2^-126. */
GLX_API int glx_segment_softmax(int device, const float* e, int32_t heads, const int32_t* cnt, int32_t num_ids,
                                int32_t num_segments, float* alpha_out, int ptr_kind, void* stream);
/* glx_segment_softmax_backward: from the forward's own output alpha and grad_alpha (no exp), for each consumed (p, h)
 *     grad_e[p, h] = alpha[p, h] * (grad_alpha[p, h] - sum_q alpha[q, h] * grad_alpha[q, h]),  q over the segment.
 * Non-finite inputs give the IEEE result of the formula.  Against the float64 value of the float32 inputs:
 *     |grad_e - exact| <= |alpha_p| * (k + 2) * 2^-23 * (|g_p| + sum_q |alpha_q g_q|) + 2^-126. */
GLX_API int glx_segment_softmax_backward(int device, const float* alpha, const float* grad_alpha, int32_t heads,
                                         const int32_t* cnt, int32_t num_ids, int32_t num_segments, float* grad_e,
                                         int ptr_kind, void* stream);

/* ---- fused GAT attention: logit, leaky_relu, softmax over the segments of a counts= request and dropout on the
 * coefficients in one kernel, with its gradients.  The attention step of the reference's GATConv
 * (python/nn/tf/layers/gat_conv.py:96-104: leaky_relu(self_e + nbr_e), unsorted_segment_softmax,
 * python/nn/tf/utils/softmax.py:24-50, tf.nn.dropout on the coefficients). ------------------------------------------
 * Common to the two entry points:
 *   s[num_segments * heads]   float32, row-major: the segment-side half of the logit (attn_src of each seed)
 *   t[num_rows * heads]       float32, row-major: the neighbour-side half, one row per node; num_rows < 2^31
 *   rows[num_ids]             int64 rows of t; a value outside [0, num_rows) reads default_attr and gets no gradient
 *   cnt[num_segments]         glx_segment_softmax's layout (clamped prefix sums cut at num_ids); NULL: the implied
 *                             layout of num_ids / num_segments positions per segment, num_ids % num_segments == 0
 *   negative_slope            finite and >= 0;  0 <= drop_p < 1;  heads >= 1;  num_ids * heads and
 *                             num_segments * heads <= INT32_MAX
 * Arguments are checked before any device use.  EVERY element of every output is written; a position that is not
 * consumed gets +0.0f.  No float atomics: one lane group (a workgroup for a long segment) reduces each (segment,
 * head) with a fixed mapping and tree -- the same inputs give the same bits on every call; the ORDER of the sums is
 * the mapping's and not part of the contract.
 *
 * glx_gat_attention: for a consumed position p of segment sg and head h
 *     tv = t[rows[p], h] (default_attr for a row out of range);  pre = fadd_rn(s[sg, h], tv);
 *     e  = pre > 0 ? pre : fmul_rn(pre, negative_slope)          -- torch's leaky_relu(a + b), never contracted
 *     soft = glx_segment_softmax of these e: its bound and its exact rules (k == 1 is 1.0f, k equal logits are
 *            1.0f / (float)k, -inf among finite logits is +0.0f, a NaN or +inf logit or only -inf ones make the
 *            column NaN).  default_attr = -inf is the masking idiom: a padded neighbour (row -1) gets exactly +0.0f.
 *     word = Philox4x32-10(counter = (i >> 2, 0, call lo, call hi), key = (seed lo, seed hi)).w[i & 3],  i = p * heads + h
 *     keep = word >= T,  T = (uint32_t)floor((double)drop_p * 2^32);  scale = 1.0f / (1.0f - drop_p)
 *     alpha = keep ? fmul_rn(soft, scale) : +0.0f;  drop_p == 0: alpha == soft bit for bit and no Philox is evaluated
 * soft_out (the softmax before dropout, what the backward needs) may be NULL iff drop_p == 0. */
GLX_API int glx_gat_attention(int device, const float* s, const float* t, int64_t num_rows, const int64_t* rows,
                              int32_t heads, const int32_t* cnt, int32_t num_ids, int32_t num_segments,
                              float negative_slope, float default_attr, float drop_p, uint64_t seed, uint64_t call,
                              float* soft_out, float* alpha_out, int ptr_kind, void* stream);
/* glx_gat_attention_backward: the mask is recomputed from (seed, call), not stored:
 *     ga = keep ? fmul_rn(grad_alpha, scale) : +0.0f;  d = soft * (ga - sum_q soft_q * ga_q)  (glx_segment_softmax_backward's
 *     bound);  grad_e = pre > 0 ? d : fmul_rn(d, negative_slope), pre recomputed from s, t and rows
 *     grad_s[sg, h] = the sum of the segment's grad_e, by the same lane group in a fixed tree: within
 *                     k * 2^-24 * sum |terms| of the exact sum of the grad_e written; an empty segment is +0.0f
 *     grad_t[r, h]  = +0.0f plus grad_e[p, h] over the consumed, in-range p with rows[p] == r in ascending p: the bits of
 *                     glx_aggregate_backward(Sum) of grad_e with one position per segment; every row is written
 * grad_e_out is required; grad_s_out and grad_t_out may each be NULL (not computed). */
GLX_API int glx_gat_attention_backward(int device, const float* soft, const float* grad_alpha, const float* s,
                                       const float* t, int64_t num_rows, const int64_t* rows, int32_t heads,
                                       const int32_t* cnt, int32_t num_ids, int32_t num_segments, float negative_slope,
                                       float default_attr, float drop_p, uint64_t seed, uint64_t call,
                                       float* grad_e_out, float* grad_s_out, float* grad_t_out, int ptr_kind,
                                       void* stream);

/* ---- fused dot-product attention: the scaled dot-product ("transformer") attention of a node over its neighbours,
 * with an edge term added to the key and to the value, and its gradients.  The layer of the reference's GPU PyTorch
 * model, TransformerConv(in, out // 2, heads=2, dropout=0.1, edge_dim=...) (examples/pytorch/tgn/train_and_eval.py:38-50).
 * Common to the two entry points:
 *   q[num_segments * dim]     float32, row-major: the query, one row per segment
 *   k, v[num_rows * dim]      float32, row-major, dense rows: the key and the value of every node; they may be one
 *                             pointer; num_rows < 2^31
 *   rows[num_ids]             int64 rows of k and v; a value outside [0, num_rows) reads a row of default_attr in both
 *                             tables and receives no gradient
 *   edge[num_ids * dim]       float32 or NULL: the edge term of every position, added to its key and to its value
 *   heads >= 1, dim % heads == 0, C = dim / heads: column c belongs to head c / C
 *   cnt[num_segments]         glx_aggregate_weighted's layout (clamped prefix sums cut at num_ids); NULL: the implied
 *                             layout of num_ids / num_segments positions per segment, num_ids % num_segments == 0
 *   scale finite;  0 <= drop_p < 1;  num_ids * heads and num_segments * dim <= INT32_MAX
 * Arguments are checked before any device use; a device-pointer call only enqueues work (the workspace is the thread's
 * per-(device, stream) lease).  EVERY element of every output that is asked for is written; a position that is not
 * consumed gets +0.0f.  No float atomics: one lane group owns each segment, of any length (a hub segment is walked by
 * its one group), with a fixed mapping and fixed trees -- the same inputs give the same bits on every call.
 *
 * glx_dot_attention: for a consumed position p of segment sg, head h and a column c of it
 *     kk(p)[c] = krow(p)[c], or fadd_rn(krow(p)[c], edge[p, c]) when edge is given; vv(p)[c] the same from v
 *     dot[p, h] = sum_c q[sg, c] * kk(p)[c]     -- glx_pair_dot's tolerance contract: the order is the mapping's,
 *                 |dot - exact| <= C * 2^-23 * sum |terms| + 2^-126 against the float64 value of the float32 kk
 *     e    = fmul_rn(dot, scale)
 *     soft = glx_segment_softmax of these e: its bound and its exact rules (k == 1 is 1.0f, k equal logits are
 *            1.0f / (float)k, -inf among finite logits is +0.0f, a NaN or +inf logit or only -inf ones make the column NaN)
 *     alpha = glx_gat_attention's dropout of soft, word for word: element i = p * heads + h, the same counter, key,
 *             threshold T and scale 1.0f / (1.0f - drop_p); drop_p == 0: alpha == soft and no Philox is evaluated
 *     out[sg, c] = +0.0f, then for each consumed p in ascending order fadd_rn(out, fmul_rn(alpha[p, h], vv(p)[c])):
 *             bit-exact, never contracted.  An empty segment is +0.0f in every column (not default_attr).
 * logit_out (may be NULL) receives e, soft_out (required) soft; out is [num_segments * dim]. */
GLX_API int glx_dot_attention(int device, const float* q, const float* k, const float* v, int64_t num_rows, int32_t dim,
                              int32_t heads, const int64_t* rows, const float* edge, const int32_t* cnt,
                              int32_t num_ids, int32_t num_segments, float scale, float default_attr, float drop_p,
                              uint64_t seed, uint64_t call, float* logit_out, float* soft_out, float* out, int ptr_kind,
                              void* stream);
/* glx_dot_attention_backward: alpha and the mask are recomputed from soft (the forward's soft_out), seed and call:
 *     ga_raw[p, h] = sum_c grad_out[sg, c] * vv(p)[c]   -- glx_aggregate_weighted_backward_w's tolerance contract
 *     ga = keep ? fmul_rn(ga_raw, 1.0f / (1.0f - drop_p)) : +0.0f;  d = soft * (ga - sum_q soft_q * ga_q)
 *     grad_e = fmul_rn(d, scale)                         -- glx_segment_softmax_backward's bound at |ga| + its error,
 *                                                           plus the propagated error of ga, times |scale|
 *     grad_q[sg, c]   = +0.0f, then in ascending p fadd_rn(., fmul_rn(grad_e[p, h], kk(p)[c])): bit-exact from grad_e
 *     grad_edge[p, c] = fadd_rn(fmul_rn(grad_e[p, h], q[sg, c]), fmul_rn(alpha[p, h], grad_out[sg, c])): bit-exact
 *     grad_k = the bits of glx_aggregate_weighted_backward_x(Sum, rows, w = grad_e, grad_out = q); grad_v the same
 *              with w = alpha and grad_out = grad_out; every row is written
 * grad_e_out is required; grad_q_out, grad_k_out, grad_v_out and grad_edge_out (which needs edge) may each be NULL
 * (not computed). */
GLX_API int glx_dot_attention_backward(int device, const float* q, const float* k, const float* v, int64_t num_rows,
                                       int32_t dim, int32_t heads, const int64_t* rows, const float* edge,
                                       const int32_t* cnt, int32_t num_ids, int32_t num_segments, float scale,
                                       float default_attr, float drop_p, uint64_t seed, uint64_t call, const float* soft,
                                       const float* grad_out, float* grad_e_out, float* grad_q_out, float* grad_k_out,
                                       float* grad_v_out, float* grad_edge_out, int ptr_kind, void* stream);
/* The CHUNKED order of dot-product attention (K5-dot-attn-chunked): opt-in, for requests with hub segments -- a
 * FullSampler hop over power-law seeds -- which the entry points above leave to one lane group each.  The two entry
 * points take exactly the arguments of glx_dot_attention / glx_dot_attention_backward, make the same checks in the same
 * order before any device use, and accept host or device pointers; the entry points above are untouched.
 * Segment sg consumes positions [s0, s1), L = s1 - s0.  L <= GLX_COALESCE_CHUNK (256) is SHORT, otherwise LONG; chunk j
 * of a long segment holds positions [s0 + 256 j, min(s0 + 256 (j + 1), s1)).
 *     logit_out   the default entry point's bits at every position (a position's dot product depends on the
 *                 (dim, heads, alignment) plan alone, not on which lane group evaluates it)
 *     short segments: the default entry point's bits in every output (soft_out, out, grad_e, grad_q, grad_edge)
 *     soft_out of a long segment: the same definition, exact rules and bound (glx_segment_softmax's), computed by one
 *                 workgroup per segment in a fixed tree over its 256 threads: bits that may differ from the default's
 *                 and are the same on every call; likewise the softmax gradient inside grad_e
 *     dropout     word for word the default's: element i = p * heads + h, the same counter, key and threshold
 *     out[sg, c]  partial_j[c] = +0.0f, then fadd_rn(., fmul_rn(alpha[p, h], vv(p)[c])) over chunk j in ascending p;
 *                 out[sg, c] = +0.0f, then one fadd_rn per partial in ascending j: bit-exact from alpha, never an FMA
 *     grad_q      the same two-level order over fmul_rn(grad_e[p, h], kk(p)[c]): bit-exact from grad_e
 *     grad_edge   the per-position formula, unchanged
 *     grad_k, grad_v   the bits of glx_aggregate_weighted_backward_x_chunked(Sum) with (w, grad_out) = (grad_e, q) /
 *                 (alpha, grad_out), on one transpose: rows named more than 256 times are chunked as well
 * EVERY element of every output that is asked for is written, an unconsumed position and an empty segment +0.0f; no
 * float atomics; the same inputs give the same bits on every call.  The chunk directory over the segments is built on
 * the device (one scan, one search per work item): the number of long segments and of chunks never reaches the host,
 * and a device-pointer call never synchronises.  A long segment of L positions has fewer than L / 128 chunks, so the
 * partial sums take at most (num_ids / 128 + 1) * dim floats of the calling thread's workspace per direction, beside
 * the [num_ids, heads] alpha under dropout and, going back, the transpose and the row gradient's own partial sums.
 * grad_q_out, grad_k_out, grad_v_out and grad_edge_out may each be NULL, as above. */
GLX_API int glx_dot_attention_chunked(int device, const float* q, const float* k, const float* v, int64_t num_rows,
                                      int32_t dim, int32_t heads, const int64_t* rows, const float* edge,
                                      const int32_t* cnt, int32_t num_ids, int32_t num_segments, float scale,
                                      float default_attr, float drop_p, uint64_t seed, uint64_t call, float* logit_out,
                                      float* soft_out, float* out, int ptr_kind, void* stream);
GLX_API int glx_dot_attention_backward_chunked(int device, const float* q, const float* k, const float* v,
                                               int64_t num_rows, int32_t dim, int32_t heads, const int64_t* rows,
                                               const float* edge, const int32_t* cnt, int32_t num_ids,
                                               int32_t num_segments, float scale, float default_attr, float drop_p,
                                               uint64_t seed, uint64_t call, const float* soft, const float* grad_out,
                                               float* grad_e_out, float* grad_q_out, float* grad_k_out,
                                               float* grad_v_out, float* grad_edge_out, int ptr_kind, void* stream);

/* ---- pair scores: the per-pair, optionally multi-head, dot product of two gathered rows, with its gradients with
 * respect to both tables.  The reference's unsupervised models score an edge as the dot product of its two endpoint
 * embeddings, against sampled negatives (examples/tf/sage/train.py:56-57, examples/tf/bipartite_sage/train.py:59-60,
 * examples/tf/ultra_gcn/ultra_gcn.py:92-95, python/nn/tf/loss.py:58). -------------------------------------------------
 * Common to the two entry points:
 *   xa[num_rows_a * dim], xb[num_rows_b * dim]   float32, row-major; they may be the same pointer
 *   heads >= 1, dim % heads == 0, C = dim / heads; column c belongs to head c / C
 *   repeat >= 1, num_pairs % repeat == 0
 *   ia[num_pairs / repeat], ib[num_pairs]        int64; pair p joins row ia[p / repeat] of xa with row ib[p] of xb:
 *                          repeat = 1 scores positive edges, repeat = K a [B, K] negative-sampler response against its B
 *                          sources, without a copy of each source K times.  An index outside its table reads a row of
 *                          default_attr
 * Arguments are checked before any device use; num_rows_* < 2^31, num_pairs * heads <= INT32_MAX.  A device-pointer
 * call only enqueues work; the workspace comes from the calling thread's per-(device, stream) cache.  No float atomics
 * anywhere.
 *
 * glx_pair_dot (tolerance contract, that of glx_aggregate_weighted_backward_w): out[p, h] = sum over the columns c of
 * head h of xa_row(p)[c] * xb_row(p)[c]; EVERY element of out[num_pairs * heads] is written.  One lane group per pair
 * with a lane-to-column mapping and a cross-lane tree fixed by (dim, heads, alignment) alone: the same inputs give the
 * same bits on every call.  The ORDER of the sum over the columns is the mapping's and not part of the contract; for any
 * order of a C-term float32 dot product, against the float64 value of the float32 inputs,
 *     |out - exact| <= C * 2^-23 * sum_c |a * b| + 2^-126;
 * non-finite inputs give the IEEE result. */
GLX_API int glx_pair_dot(int device, const float* xa, int64_t num_rows_a, const float* xb, int64_t num_rows_b,
                         int32_t dim, int32_t heads, const int64_t* ia, const int64_t* ib, int32_t num_pairs,
                         int32_t repeat, float default_attr, float* out, int ptr_kind, void* stream);
/* glx_pair_dot_backward (bit-exact contract, that of glx_aggregate_weighted_backward_x): the gradient of the table on
 * `side` (0: xa, 1: xb) from g[num_pairs * heads], the gradient of out.  grad_self[r, c] starts at +0.0f and, for each
 * pair p whose own index (side 0: ia[p / repeat], side 1: ib[p]) is r, in ascending p, becomes
 *     fadd_rn(grad_self[r, c], fmul_rn(g[p, head(c)], other_row(p)[c]))
 * -- two roundings, never contracted into an FMA under any build flag; other_row(p) is row ib[p] (side 0) or
 * ia[p / repeat] (side 1) of x_other[num_rows_other * dim], a row of default_attr when that index is outside the table.
 * An own index outside [0, num_rows_self) receives nothing.  EVERY row of grad_self[num_rows_self * dim] is written; the
 * call overwrites.  (The stable sort by row of glx_aggregate_backward over the own index array -- for side 0 its
 * num_pairs / repeat entries only -- then one lane group per row.) */
GLX_API int glx_pair_dot_backward(int device, int side, const int64_t* ia, const int64_t* ib, int32_t num_pairs,
                                  int32_t repeat, const float* g, int32_t heads, const float* x_other,
                                  int64_t num_rows_other, int32_t dim, int64_t num_rows_self, float default_attr,
                                  float* grad_self, int ptr_kind, void* stream);

/* ---- the bfloat16 training path (added under 5): the six entry points above that take or return a [rows, dim] matrix
 * of the model, with that matrix in float32 or bfloat16.  They stand where their float32 siblings stand: the
 * differentiable segment reductions under the reference's layers (python/nn/tf/layers/sage_conv.py:69-73,
 * gcn_conv.py:52-73, gat_conv.py:96-110, ego_gat_conv.py:98-103) and the pair scores of its unsupervised models
 * (examples/tf/sage/train.py:56-57, python/nn/tf/loss.py:58), for a model that runs under bfloat16 autocast. ----------
 * Each _ex entry point is its sibling's signature with the table pointer turned into const void* / void* plus a dtype
 * argument: GLX_DTYPE_F32 or GLX_DTYPE_BF16.  GLX_DTYPE_F16 and the two float8 ids are GLX_INVALID_ARGUMENT -- bfloat16
 * is the half type that has a gradient contract: float16 gradients need loss scaling, a contract of its own -- and so
 * is any other id; the dtype is checked before anything else, so the answer needs no device.  With GLX_DTYPE_F32 an _ex
 * entry point IS its sibling: the six siblings are calls of it, the same kernels, launch shapes and bits.
 *
 * Reads (x, xa / xb, x_other in bfloat16): every element is upcast to float32 as it is loaded -- exact -- and everything
 * downstream is the float32 kernel's arithmetic in the float32 kernel's order.  Every output that is float32 in the
 * sibling stays float32 (emb_out, out, grad_w) and is BIT-IDENTICAL to what the sibling returns for the float32 matrix
 * of the upcast values: the ascending-position folds (glx_aggregate_weighted_ex) and the fixed trees
 * (glx_pair_dot_ex, glx_aggregate_weighted_backward_w_ex) alike.  The trees depend on the lane-to-column mapping, so a
 * bfloat16 call keeps the mapping the float32 call picks for the same (dim, heads): a lane still owns 4 columns, loaded
 * as four bfloat16 in one 8-byte access, and the alignment the 4-column path asks of a bfloat16 matrix is 4 elements =
 * 8 bytes (16 for float32).  A matrix with dim % 4 == 0 whose base is 16-byte aligned therefore takes the same path in
 * both types.  default_attr stays a float32 fill and is not rounded.
 *
 * Row gradients (grad_x, grad_self in bfloat16): let G[r, c] be exactly the float32 value the sibling writes for the
 * same arguments.  The stored element is that value rounded ONCE, to nearest even, by the integer-arithmetic converter
 * the uploads use -- glx_features_convert_host(.., GLX_DTYPE_BF16, ..) is the same code on the host.  So a NaN is
 * stored as 0xFFFF, a value of magnitude 0x7F7F8000 or more as +-inf, bfloat16 subnormals are kept, and so is the sign
 * of zero.  Accumulation never happens in bfloat16; each element is within 2^-9 relative of the float32 gradient (8
 * significand bits).  Every row is still written, rows nobody references are +0.0 (all bits clear), nothing is
 * written outside the num_rows * dim ELEMENTS of the buffer, element offsets are 64-bit, no float atomics, the same
 * bits on every call.  Host buffers hold the 16-bit codes.
 *
 * What stays float32 in every case: w, g, grad_out, the logits and coefficients of glx_segment_softmax /
 * glx_gat_attention / glx_dot_attention ([n, heads] arrays, a few bytes a row), glx_rows_coalesce /
 * glx_embedding_update, the TGN entry points and the distributed store. */
GLX_API int glx_aggregate_backward_ex(int device, int op, const int64_t* rows, const int32_t* cnt, const int32_t* arg,
                                      int32_t num_ids, int32_t num_segments, int64_t num_rows, int32_t dim,
                                      const float* grad_out, void* grad_x, int grad_x_dtype, int ptr_kind,
                                      void* stream);
GLX_API int glx_aggregate_weighted_ex(int device, int op, const void* x, int x_dtype, int64_t num_rows, int32_t dim,
                                      const int64_t* rows, const float* w, int32_t heads, const int32_t* cnt,
                                      int32_t num_ids, int32_t num_segments, float default_attr, float* emb_out,
                                      int ptr_kind, void* stream);
GLX_API int glx_aggregate_weighted_backward_x_ex(int device, int op, const int64_t* rows, const float* w, int32_t heads,
                                                 const int32_t* cnt, int32_t num_ids, int32_t num_segments,
                                                 int64_t num_rows, int32_t dim, const float* grad_out, void* grad_x,
                                                 int grad_x_dtype, int ptr_kind, void* stream);
GLX_API int glx_aggregate_weighted_backward_w_ex(int device, int op, const void* x, int x_dtype, int64_t num_rows,
                                                 int32_t dim, const int64_t* rows, int32_t heads, const int32_t* cnt,
                                                 int32_t num_ids, int32_t num_segments, float default_attr,
                                                 const float* grad_out, float* grad_w, int ptr_kind, void* stream);
/* one x_dtype for both tables */
GLX_API int glx_pair_dot_ex(int device, const void* xa, int64_t num_rows_a, const void* xb, int64_t num_rows_b,
                            int x_dtype, int32_t dim, int32_t heads, const int64_t* ia, const int64_t* ib,
                            int32_t num_pairs, int32_t repeat, float default_attr, float* out, int ptr_kind,
                            void* stream);
/* x_other and grad_self both hold x_dtype elements */
GLX_API int glx_pair_dot_backward_ex(int device, int side, const int64_t* ia, const int64_t* ib, int32_t num_pairs,
                                     int32_t repeat, const float* g, int32_t heads, const void* x_other,
                                     int64_t num_rows_other, int32_t dim, int64_t num_rows_self, float default_attr,
                                     void* grad_self, int x_dtype, int ptr_kind, void* stream);

/* ---- trainable embedding tables: the coalesced row gradient of a lookup and the sparse optimizer steps that apply it
 * in place, on the touched rows only.  The reference trains tables in two places: one EmbeddingColumn per categorical
 * attribute (python/nn/tf/data/feature_column.py:128-157) and the target / context id embeddings of DeepWalk / node2vec
 * (examples/tf/node2vec/node2vec.py:49-50). -----------------------------------------------------------------------------
 * Common to the two entry points: arguments are checked before any device use; 0 <= num_rows < 2^31, dim >= 1,
 * n * dim <= INT32_MAX; row indices are dense (row r is r: no id map).  A device-pointer call only enqueues work; the
 * workspace comes from the calling thread's per-(device, stream) cache.  No float atomics anywhere; nothing is
 * allocated, cleared or launched in proportion to num_rows.  The build's -ffp-contract=off and
 * -fhip-fp32-correctly-rounded-divide-sqrt give the single roundings the contracts name. */
#define GLX_EMB_SGD 0
#define GLX_EMB_ADAGRAD 1
#define GLX_EMB_ADAM 2
#define GLX_COALESCE_CHUNK 256
/* glx_rows_coalesce (bit-exact contract): the gradient g[n * dim] of a lookup of rows[n], summed per distinct row.
 * A position whose row is outside [0, num_rows) is dropped.  With U the number of distinct remaining rows,
 * urows_out[0 .. U) holds them ascending, urows_out[U .. n) is -1, *num_unique_out = U (one word, of the same ptr_kind
 * as the other buffers) and rows U .. n of ug_out[n * dim] are NOT written.  For u < U let p_0 < p_1 < ... < p_{L-1} be
 * the positions with rows[p] == urows_out[u], cut into chunks of GLX_COALESCE_CHUNK consecutive list entries: chunk k's
 * partial starts at +0.0f and becomes fadd_rn(partial, g[p, c]) in ascending p; ug_out[u, c] starts at +0.0f and becomes
 * fadd_rn(ug_out[u, c], partial_k) in ascending k.  A list of at most GLX_COALESCE_CHUNK positions is therefore summed in
 * plain ascending order and equals the row glx_aggregate_backward(GLX_AGG_SUM, implied layout, one position per segment)
 * writes, bit for bit; a longer list -- a categorical value shared by a whole batch, a hub -- is reduced by
 * ceil(L / GLX_COALESCE_CHUNK) lane groups and a second pass that adds their partial sums in that fixed order.
 * (A stable radix sort of (row, position) over the bits num_rows needs, the sentinel key num_rows for dropped
 * positions; run and chunk heads from flags and one scan over the n sorted keys; one lane group per chunk.) */
GLX_API int glx_rows_coalesce(int device, const int64_t* rows, int32_t n, int64_t num_rows, int32_t dim, const float* g,
                              int64_t* urows_out, float* ug_out, int64_t* num_unique_out, int ptr_kind, void* stream);
/* glx_embedding_update (bit-exact contract): one optimizer step on the rows urows[n] names, DEVICE pointers only (the
 * tables live in HBM).  For each entry u < n with urows[u] in [0, num_rows) and each column, with g = ug[u, c] and w, s,
 * m, v the elements of row urows[u] of W, state1, state2 -- every operation one correctly rounded float32 operation, in
 * this order:
 *   GLX_EMB_SGD                                    w = w - alpha * g
 *   GLX_EMB_ADAGRAD  (state1 = s)                  s = s + g * g;  w = w - alpha * (g / (sqrtf(s) + eps))
 *   GLX_EMB_ADAM     (state1 = m, state2 = v)      m = beta1 * m + c1 * g;  v = beta2 * v + c2 * (g * g);
 *                                                  w = w - alpha * (m / (sqrtf(v) + eps))
 * The caller computes the scalars in double and rounds each to float32 once: alpha = lr for SGD and Adagrad; for Adam at
 * global step t, alpha = lr * sqrt(1 - beta2^t) / (1 - beta1^t), c1 = 1 - beta1, c2 = 1 - beta2 -- in exact arithmetic
 * torch.optim.SGD, Adagrad (lr_decay = 0, weight_decay = 0) and SparseAdam on the coalesced gradient.  An entry outside
 * the table is skipped -- the -1 tail of glx_rows_coalesce among them, so a step is launched over n without U on the
 * host.  Rows nobody names are not touched, not even rewritten.  A state table the algorithm does not use must be NULL,
 * one it uses must not be.  PRECONDITION, not detected: the valid entries name distinct rows; a repeated row is a lost
 * update, not a fault.  (One lane group per entry, 16-byte accesses when dim % 4 == 0 and every base is 16-byte aligned;
 * each row read once, each written row written once, one kernel.) */
GLX_API int glx_embedding_update(int device, int algo, float* W, float* state1, float* state2, int64_t num_rows,
                                 int32_t dim, const int64_t* urows, const float* ug, int32_t n, float alpha, float eps,
                                 float beta1, float c1, float beta2, float c2, void* stream);

/* ---- chunked row gradients (K5-bwd-chunked): a second, named summation order for the row gradients of the
 * differentiable segment reductions under the reference's layers (python/nn/tf/layers/sage_conv.py:69-73,
 * gcn_conv.py:52-73, gat_conv.py:96-110, ego_gat_conv.py:98-103), for requests in which a few rows -- the hubs an
 * EdgeWeight sampler keeps drawing -- are referenced far more often than the rest. ----------------------------------
 * glx_aggregate_backward_chunked takes glx_aggregate_backward_ex's arguments, glx_aggregate_weighted_backward_x_chunked
 * those of glx_aggregate_weighted_backward_x_ex, with the same checks in the same order (grad_x_dtype first, before any
 * device use; GLX_DTYPE_F32 or GLX_DTYPE_BF16), the same segment layouts, host and device pointers.  The _ex entry
 * points and their float32 siblings are untouched: the ascending-position order stays the default, and this one is
 * chosen per call.
 *
 * The list of table row r is the consumed, in-range request positions p_0 < p_1 < ... with rows[p] == r.  An entry that
 * a Max / Min arg does not select is still a list entry: chunk boundaries count ENTRIES, not selected terms.  The list
 * is cut into chunks of GLX_COALESCE_CHUNK consecutive entries.  The TERMS are exactly the default order's:
 * grad_out[s(p), c] (Sum); grad_out[s(p), c] / float(cnt[s(p)]) (Mean, the raw count as in glx_aggregate_backward);
 * grad_out[s(p), c] where arg[s(p), c] == p and no add otherwise (Max / Min); fmul_rn(w[p, head(c)], t) with t the Sum
 * or Mean term and count(s) as in glx_aggregate_weighted_backward_x (weighted: two roundings, never an FMA).
 *     partial_k[c]  = +0.0f, then one fadd_rn per selected term of chunk k, in ascending p
 *     grad_x[r, c]  = +0.0f, then one fadd_rn per partial, in ascending k
 * Consequences: a row whose list has at most GLX_COALESCE_CHUNK entries gets the default order's bits; for Sum the
 * result equals glx_rows_coalesce applied to g[p] = grad_out[s(p)] over the consumed positions, bit for bit; EVERY row
 * of grad_x is written, exactly once; a row nobody references is all bits clear; no float atomics; the same inputs give
 * the same bits on every call.  A bfloat16 grad_x: partials and the combine are float32 and the finished sum is rounded
 * ONCE, in the final store -- the float32 chunked result pushed through the converter of the _ex entry points -- and no
 * float32 [num_rows, dim] buffer is allocated.
 * (The transpose of glx_aggregate_backward; a chunk directory built on the device from its row offsets -- one scan, one
 * search per work item; one lane group per short row, one per chunk of a long row, one per long row to combine.  The
 * number of long rows and of chunks never reaches the host: no read-back, no synchronisation.  A list of L >
 * GLX_COALESCE_CHUNK entries has fewer than L / 128 chunks, so the partial sums take at most (num_ids / 128 + 1) * dim
 * floats of the calling thread's workspace, beside the transpose.)
 * Still summed by one lane group per list, in ascending position: glx_pair_dot_backward and grad_t of
 * glx_gat_attention_backward (dot-product attention has a chunked order of its own, for its long segments and for
 * grad_k / grad_v: glx_dot_attention_chunked, glx_dot_attention_backward_chunked); Prod has no backward; the
 * distributed store has none either; request plans (graph capture) do not cover the backward. */
GLX_API int glx_aggregate_backward_chunked(int device, int op, const int64_t* rows, const int32_t* cnt,
                                           const int32_t* arg, int32_t num_ids, int32_t num_segments, int64_t num_rows,
                                           int32_t dim, const float* grad_out, void* grad_x, int grad_x_dtype,
                                           int ptr_kind, void* stream);
GLX_API int glx_aggregate_weighted_backward_x_chunked(int device, int op, const int64_t* rows, const float* w,
                                                      int32_t heads, const int32_t* cnt, int32_t num_ids,
                                                      int32_t num_segments, int64_t num_rows, int32_t dim,
                                                      const float* grad_out, void* grad_x, int grad_x_dtype,
                                                      int ptr_kind, void* stream);

/* ---- TGN memory: the device-resident message store, the fused message and the memory write of the memory module the
 * reference's TGN example takes from torch_geometric -- TGNMemory(num_nodes, msg_dim, memory_dim, time_dim,
 * message_module=IdentityMessage(...), aggregator_module=LastAggregator()) (examples/pytorch/tgn/train_and_eval.py:70,
 * the imports at train_and_eval.py:27 above it; used at train_and_eval.py:118 and train_and_eval.py:130). -------------
 * With the Last aggregator and a message function without parameters the only stored message of a node that is ever
 * used is the node's latest event over both roles, and the store never clears a message on consumption.  So the store
 * is ONE pending slot per node, in caller-owned DEVICE buffers (as glx_embedding_update keeps its tables):
 *   memory      [N, M] float32   +0.0        node memory
 *   last_update [N]    int64     0           time of the last memory write
 *   pend_t      [N]    int64     INT64_MIN   timestamp of the node's latest event
 *   pend_seq    [N]    int64     -1          its sequence number; -1: no message
 *   pend_other  [N]    int64     -1          the event's other end point
 *   pend_raw    [N, R] float32   +0.0        the event's raw message (a copy of the row)
 * (the third column is the initial value the caller fills in).  The sequence number of position p of a
 * glx_tgn_store_update call is seq_base + p, seq_base = the number of events passed to earlier calls since the buffers
 * were initialised.  The slot of node v holds the event with the largest (t, seq) among all events that ever named v as
 * src or dst; a self loop names v twice with the same content.  On a time-ordered stream this is TGNMemory +
 * LastAggregator with the tie rule fixed -- of two events of one timestamp the larger seq wins, where
 * LastAggregator's scatter_argmax leaves it open.  On a stream that is NOT time-ordered the rule is still total, and
 * then DIFFERS from torch_geometric, which lets a later call overwrite a role's list whatever its timestamps are.
 * Ids outside [0, N) are dropped everywhere.  Common to the four: all pointers are DEVICE pointers; arguments are
 * checked before any device use; 0 <= N < 2^31; a call only enqueues work on `stream`; every element of every output
 * is written; no float atomics; nothing is allocated, cleared or launched in proportion to N.  Limits: Last aggregator
 * and identity message only; float32 only; one GPU (not the distributed store); no graph capture (the backward leases a
 * workspace); a hub's candidates meet in same-address integer atomics; N * (4 M + 4 R + 32) bytes of state. */
/* glx_tgn_store_update (bit-exact contract): applies the slot rule to the 2 * batch (event, end point) candidates of
 * src[batch], dst[batch], t[batch], raw_msg[batch * raw_dim].  The result depends on no scheduling order: launch one
 * raises pend_t[v] to the largest t (64-bit signed atomic max); launch two raises pend_seq[v] to the largest
 * seq_base + p among the candidates with t[p] == pend_t[v] -- every older slot has seq < seq_base, so a slot whose t
 * was neither beaten nor equalled stays whole; in launch three the winners write pend_other[v] and copy their raw row,
 * one lane group per winning candidate.  A candidate loads the word first and skips the atomic when it cannot raise it,
 * and the lanes of a wave that agree on an address issue one atomic (for the first 4 addresses a wave names).
 * batch = 0 is a no-op; raw_dim = 0 is legal (raw_msg and pend_raw may be NULL); 0 <= seq_base, batch < 2^30. */
GLX_API int glx_tgn_store_update(int device, int64_t num_nodes, int32_t raw_dim, const int64_t* src, const int64_t* dst,
                                 const int64_t* t, const float* raw_msg, int32_t batch, int64_t seq_base,
                                 int64_t* pend_t, int64_t* pend_seq, int64_t* pend_other, float* pend_raw, void* stream);
/* glx_tgn_message: entry i < n, v = n_id[i] (repeats allowed), row width 2 M + R + T.
 *   h_out[i]   = memory[v], or +0.0 for an id outside the table.
 *   v inside the table and pend_seq[v] >= 0:  has_out[i] = 1, t_out[i] = pend_t[v],
 *     dt_out[i] = (float)(pend_t[v] - last_update[v]) -- the int64 difference, then one conversion, round to nearest --
 *     msg_out[i] = [memory[v] | memory[pend_other[v]] | pend_raw[v] | cosf(fmaf(time_w[j], dt, time_b[j])) for j < T];
 *     a pend_other outside the table reads +0.0.  The three copied parts are bit copies; the last uses the accurate
 *     cosf (checked against a bound).
 *   otherwise: has_out[i] = 0, t_out[i] = last_update[v] (0 for an id outside the table), dt_out[i] = +0.0 and the
 *     whole row is +0.0 (torch_geometric feeds the GRU a zero message for such a node).
 * One lane group per entry; each piece moves 16 bytes at a time when its two addresses are 16-byte aligned, one word
 * at a time otherwise (R = 3 makes every later column unaligned).  mem_dim >= 1, raw_dim >= 0, time_dim >= 0. */
GLX_API int glx_tgn_message(int device, int64_t num_nodes, int32_t mem_dim, int32_t raw_dim, int32_t time_dim,
                            const float* memory, const int64_t* last_update, const int64_t* pend_t,
                            const int64_t* pend_seq, const int64_t* pend_other, const float* pend_raw,
                            const float* time_w, const float* time_b, const int64_t* n_id, int32_t n, float* msg_out,
                            float* h_out, float* dt_out, int64_t* t_out, int32_t* has_out, void* stream);
/* glx_tgn_message_backward: the gradient of the time encoder through columns [time_off, time_off + time_dim) of
 * grad_msg[n * width], from the dt[n] and has[n] glx_tgn_message wrote.  With x_ij = fmaf(time_w[j], dt[i], time_b[j])
 * and term_ij = grad_msg[i, time_off + j] * (-sinf(x_ij)) (one rounding):
 *   grad_b[j] = the sum over the i with has[i] != 0 of term_ij,   grad_w[j] = the same sum of term_ij * dt[i].
 * A row with has[i] == 0 contributes nothing, whatever its gradient holds.  memory and pend_raw are constants (they are
 * buffers, and the reference detaches the memory every batch, train_and_eval.py:134).  The sum is a FIXED tree, the
 * same bits on every call: rows are cut into chunks of GLX_TGN_BWD_ROWS; in a chunk, wave w of 4 adds rows w, w + 4, ..
 * ascending to +0.0 (64 additions), the four waves combine as (0 + 1) + (2 + 3) (2 additions); then per column lane l of
 * 64 adds the partials of chunks l, l + 64, .. ascending to +0.0 (ceil(chunks / 64) additions) and the lanes combine
 * in an xor butterfly (6 additions).  D, the float32 additions on the longest path, is GLX_TGN_BWD_DEPTH(n).
 * n = 0 writes +0.0.  time_dim >= 1. */
#define GLX_TGN_BWD_ROWS 256
#define GLX_TGN_BWD_DEPTH(n) (72 + ((n) + 16383) / 16384)
GLX_API int glx_tgn_message_backward(int device, int32_t n, int32_t width, int32_t time_off, int32_t time_dim,
                                     const float* grad_msg, const float* dt, const int32_t* has, const float* time_w,
                                     const float* time_b, float* grad_w, float* grad_b, void* stream);
/* glx_tgn_memory_write (bit-exact): row i of new_memory[n * mem_dim] goes to row n_id[i] of memory, and
 * last_update[n_id[i]] = t_new[i].  An id outside the table is skipped -- the -1 padding of a distinct-id list among
 * them.  Rows nobody names are not touched, not even rewritten.  PRECONDITION, not detected: the valid entries name
 * distinct rows; a repeated row is a lost update, not a fault.  (One lane group per entry.) */
GLX_API int glx_tgn_memory_write(int device, int64_t num_nodes, int32_t mem_dim, const int64_t* n_id, int32_t n,
                                 const float* new_memory, const int64_t* t_new, float* memory, int64_t* last_update,
                                 void* stream);

/* ---- negative sampling: replaces RandomNegativeSampler (random_negative_sampler.cc:30-63),
 * InDegreeNegativeSampler / SoftInDegreeNegativeSampler (in_degree_negative_sampler.cc:29-135)
 * and NodeWeightNegativeSampler (node_weight_negative_sampler.cc:29-110). ---------------
 * A glx_negative is the candidate list all rows of a request draw from, in HBM:
 *   glx_negative_from_graph: the edge type's distinct destination ids in first-appearance
 *     order (TopoStatics::Add, topo_statics.cc:32-55 = GetAllDstIds()), uniform
 *     (by_in_degree = 0) or weighted by in-degree (GetAllInDegrees()) through ONE alias
 *     table over the whole list (AliasMethodFactory::LookupOrCreate), bit-identical to
 *     AliasMethod::Build (alias_method.cc:57-107);
 *   glx_negative_create: explicit ids (+ weights or NULL = uniform): a node type's ids and
 *     node weights for NodeWeightNegativeSampler.
 * glx_negative_sample: out[batch * count] candidates (no edge ids, as in the reference).
 *   exclude = GLX_NEG_EXCLUDE_NONE      every draw is taken (Random, SoftInDegree);
 *             GLX_NEG_EXCLUDE_NEIGHBORS a candidate that is an out-neighbour of src[i] in `g` is
 *                                       skipped (InDegree; needs glx_graph_enable_negative(g));
 *             GLX_NEG_EXCLUDE_BATCH     a candidate equal to ANY src id of the request is skipped
 *                                       (NodeWeight).
 *   The strict modes follow the reference's retry loop: blocks of `count` draws, accepted
 *   candidates keep their order, the exclusion set is dropped from the 4th block on
 *   (kRetryTimes = 3).  Row i draws from the random stream (seed, call_counter, i); draw
 *   b * count + j is candidate j of block b.  Weighted draws use AliasMethod::Sample's formula
 *   (alias_method.cc:117-121), uniform ones floor(u * num_ids / 2^64).  An empty candidate
 *   list yields `default_neighbor_id` everywhere. */
#define GLX_NEG_EXCLUDE_NONE 0
#define GLX_NEG_EXCLUDE_NEIGHBORS 1
#define GLX_NEG_EXCLUDE_BATCH 2
typedef struct glx_negative glx_negative;
GLX_API int glx_negative_create(int device, int64_t num_ids, const int64_t* ids, const float* weights, int ptr_kind,
                                void* stream, glx_negative** out);
GLX_API int glx_negative_from_graph(const glx_graph* g, int by_in_degree, void* stream, glx_negative** out);
GLX_API void glx_negative_destroy(glx_negative* t);
GLX_API int glx_negative_info(const glx_negative* t, int64_t* num_ids, int* weighted);
/* Copies the candidate ids and the alias table to HOST arrays (parity checks). */
GLX_API int glx_negative_export(const glx_negative* t, int64_t* ids, float* prob, int32_t* alias, void* stream);
/* Builds every row's neighbour ids in ascending order, each with the CSR slot it came from: the exclusion
 * test of strict negative sampling is a binary search in it, and an id == value filter
 * (glx_sample_filtered) finds its hits the same way instead of scanning the row.  MUTATES the handle. */
GLX_API int glx_graph_enable_negative(glx_graph* g, void* stream);
GLX_API int glx_negative_sample(const glx_negative* t, int exclude, const glx_graph* g, const int64_t* src,
                                int32_t batch, int32_t count, int64_t default_neighbor_id, uint64_t seed,
                                uint64_t call_counter, int64_t* out, int ptr_kind, void* stream);

/* ---- feature lookup: replaces LookupNodes' float-attribute gather
 * (node_lookuper.cc:24-52); out[n*dim], unknown ids -> default_attr. */
GLX_API int glx_lookup(const glx_features* f, const int64_t* node_ids, int64_t n, float default_attr,
               float* out, int ptr_kind, void* stream);

/* ---- property columns: replaces NodeStorage::GetWeight / GetLabel / GetTimestamp / GetAttribute()->GetInts()
 * (memory_node_storage.cc:88-138) and EdgeStorage's (memory_edge_storage.cc:90-125) as LookupNodes / LookupEdges read them
 * (node_lookuper.cc:24-52, edge_lookuper.cc:24-52) for everything but the float block (glx_lookup) and strings. --------
 * A glx_columns is a device table of fixed-width records, one per node row or per edge id, holding whichever of these
 * the type has, interleaved:  int_attrs int64[i_num] | timestamp int64 | weight float32 | label int32  -- padded to 8
 * bytes, and to a multiple of 16 once the record is 16 bytes or longer, so that one id translation
 * and one contiguous read serve every column a request asks for.
 * glx_columns_create: weights[num_rows], labels[num_rows], timestamps[num_rows], int_attrs[num_rows * i_num]; any of them
 *   may be NULL = the type does not have it (int_attrs exactly when i_num == 0).  The id map is one of
 *     ids[num_rows]  raw id of every row: the table builds its own map;
 *     map_of         a glx_features of the same rows whose map is BORROWED (it must outlive the table): a node type that
 *                    already has a feature table does not pay for a second hash table;
 *     neither        dense: id r is row r (edge ids).  Both: GLX_INVALID_ARGUMENT.
 * glx_columns_lookup: ids[n] -> weights_out[n], labels_out[n], timestamps_out[n], int_attrs_out[n * i_num] (the reference's
 *   response layout); any out pointer may be NULL.  For an output that is asked for:
 *     the type lacks the column   weight 0.0, label -1, timestamp -1 (memory_node_storage.cc:88-112);
 *     the id is unknown           the caller's default_* (GLOBAL_FLAG(DefaultWeight) ...; for a dense table: an id outside
 *                                 [0, num_rows), e.g. the -1 edge id of a default-filled sample);
 *   values are moved, never converted: a weight's bits arrive as they were stored (NaN payloads included).
 *   n == 0 is GLX_OK without a launch.
 * glx_columns_info: any out pointer may be NULL; *record_bytes is the padded record (0: no column at all), *id_map one of
 *   GLX_COLUMNS_MAP_*. */
#define GLX_COLUMNS_MAP_DENSE 0
#define GLX_COLUMNS_MAP_OWN 1
#define GLX_COLUMNS_MAP_BORROWED 2
typedef struct glx_columns glx_columns;
GLX_API int glx_columns_create(int device, int64_t num_rows, int32_t i_num, const float* weights, const int32_t* labels,
                               const int64_t* timestamps, const int64_t* int_attrs, const int64_t* ids,
                               const glx_features* map_of, int ptr_kind, void* stream, glx_columns** out);
GLX_API void glx_columns_destroy(glx_columns* c);
GLX_API int glx_columns_info(const glx_columns* c, int64_t* num_rows, int32_t* i_num, int* has_weight, int* has_label,
                             int* has_timestamp, int32_t* record_bytes, int* id_map, int* device);
GLX_API int glx_columns_lookup(const glx_columns* c, const int64_t* ids, int64_t n, float default_weight,
                               int32_t default_label, int64_t default_timestamp, int64_t default_int_attr,
                               float* weights_out, int32_t* labels_out, int64_t* timestamps_out, int64_t* int_attrs_out,
                               int ptr_kind, void* stream);

/* ---- shard exchange helpers: replace HashPartitioner::Partition
 * (hash_partitioner.h:33-92; shard = llabs(id) % P, stable inside a shard) and
 * Stitcher::DoStitch (stitcher.h:67-107).  These take device pointers only
 * (they sit between two RCCL all-to-alls). ---------------------------------
 * glx_partition: ids[n] -> bucketed[n] (ids grouped by shard, original order
 *   kept inside a shard), order[n] (the concatenated Sticker lists: order[i] is
 *   the original index of bucketed[i]), counts[num_shards] (int64, device).
 * glx_stitch_i64 / _f32: out[order[i]*width + c] = in[i*width + c]. */
GLX_API int glx_partition(int device, const int64_t* ids, int64_t n, int32_t num_shards,
                  int64_t* bucketed, int64_t* order, int64_t* counts, void* stream);
GLX_API int glx_stitch_i64(int device, const int64_t* in, const int64_t* order, int64_t n, int32_t width,
                   int64_t* out, void* stream);
GLX_API int glx_stitch_f32(int device, const float* in, const int64_t* order, int64_t n, int32_t width,
                   float* out, void* stream);

/* glx_aggregate_stitch: replaces AggregatingResponse::Stitch
 *   (aggregating_request.cc:172-213 + the aggregators' AggFunc/FinalFunc): combines the
 *   partial results of `num_parts` shards, parts[num_parts][num_segments*dim] and
 *   cnts[num_parts][num_segments] (the receive buffers of one all-to-all), folding in
 *   shard order from InitFunc's value; Mean re-weights partial means by their counts.
 *   A shard with count 0 for a segment is skipped (the reference folds its
 *   DefaultFloatAttribute row in, which corrupts Max/Min/Prod: SURVEY 8(a) quirk 8);
 *   when no partial is empty the result is bit-identical to the reference's Stitch. */
GLX_API int glx_aggregate_stitch(int device, int op, int32_t num_parts, const float* parts,
                                 const int32_t* cnts, int32_t num_segments, int32_t dim, float default_attr,
                                 float* emb_out, int32_t* cnt_out, void* stream);

/* ---- shard communicator: replaces the RPC layer under DistributeRunner
 * (core/runner/op_runner.h:86-152 RunInParallel: one gRPC call per remote shard,
 * service/client_impl.cc + rpc/) with RCCL point-to-point groups over xGMI. -----------
 * One glx_comm per process (= per GPU) and per concurrently used stream; `rank` plays the
 * role of the reference's server id and `world` of its server count (hash_partitioner.h:33-92
 * routes id v to shard llabs(v) % world).  Three transports, one interface:
 *   glx_comm_init_rccl       ncclCommInitRank from a unique id that rank 0 made with
 *                            glx_comm_unique_id and handed to the others out of band (the
 *                            role of the reference's coordinator / naming engine);
 *                            exchanges are ncclGroupStart + ncclSend/ncclRecv + ncclGroupEnd
 *                            on the caller's stream (librccl is loaded with dlopen, so the
 *                            library loads without it);
 *   glx_comm_init_local      `world` ranks that are threads of ONE process (each may use its
 *                            own GPU or all the same one): peers copy device-to-device out of
 *                            each other's send buffers between two host barriers.  Ranks that
 *                            pass the same `fabric_key` form one communicator.  This is the
 *                            one-GPU test rig and the single-process multi-GPU mode;
 *   glx_comm_init_callbacks  host-staged: buffers are copied to pinned host memory and handed
 *                            to the caller's all-to-all / all-gather (e.g. torch.distributed
 *                            gloo, MPI) -- for ranks that cannot run RCCL together. */
#define GLX_UNIQUE_ID_BYTES 128
#define GLX_COMM_RCCL 0
#define GLX_COMM_LOCAL 1
#define GLX_COMM_CALLBACKS 2
typedef struct glx_comm glx_comm;
/* send/recv are packed host buffers (peer-major); counts are in elements of elem_bytes. */
typedef int (*glx_host_alltoallv_fn)(void* user, const void* send, const int64_t* send_counts, void* recv,
                                     const int64_t* recv_counts, int64_t elem_bytes);
typedef int (*glx_host_allgather_fn)(void* user, const void* send, void* recv, int64_t bytes_per_rank);
GLX_API int glx_comm_unique_id(void* id_out /* GLX_UNIQUE_ID_BYTES */);
GLX_API int glx_comm_init_rccl(int device, int rank, int world, const void* unique_id, glx_comm** out);
GLX_API int glx_comm_init_local(int64_t fabric_key, int device, int rank, int world, glx_comm** out);
GLX_API int glx_comm_init_callbacks(int device, int rank, int world, glx_host_alltoallv_fn alltoallv,
                                    glx_host_allgather_fn allgather, void* user, glx_comm** out);
GLX_API void glx_comm_destroy(glx_comm* c);
GLX_API int glx_comm_info(const glx_comm* c, int* rank, int* world, int* device, int* transport);
/* No peer message of one exchange round exceeds this many bytes (default 512 MiB; RCCL 2.26
 * was seen to deliver only half of an all-to-all message above 1 GiB); larger exchanges are
 * cut into rounds of pointer offsets -- no staging copies.  Returns the previous value. */
GLX_API int64_t glx_comm_set_max_message_bytes(glx_comm* c, int64_t bytes);
/* all-to-all(v): send_counts[p] consecutive elements of `send` (peer-major, packed) go to rank
 * p; recv_counts[q] elements arrive from rank q into `recv` (packed in rank order).  Counts are
 * HOST arrays of `world` entries; data pointers are host or device per ptr_kind.  Collective:
 * every rank of the communicator must call it.  Device pointers: enqueued on `stream`. */
GLX_API int glx_exchange_v(glx_comm* c, const void* send, const int64_t* send_counts, void* recv,
                           const int64_t* recv_counts, int64_t elem_bytes, int ptr_kind, void* stream);
/* vals[nvals] int64 of every rank -> out[world * nvals] on every rank (rank-major), host or
 * device pointers.  The call returns when `out` is valid (it synchronises `stream`). */
GLX_API int glx_comm_allgather_i64(glx_comm* c, const int64_t* vals, int32_t nvals, int64_t* out, int ptr_kind,
                                   void* stream);
GLX_API int glx_comm_barrier(glx_comm* c, void* stream);

/* ---- distributed store: replaces DistributeRunner<Req, Res>::Run (op_runner.h:60-84) for
 * the sampling (dense samplers, FullSampler, DeepWalk), aggregating and node-lookup requests:
 * Partition (hash_partitioner.h:33-92) -> ship the
 * parts -> Process on the owning shard -> ship the results back -> Stitch
 * (stitcher.h:67-107; aggregating_request.cc:117-213) -- all on the device, between the
 * caller's request and response buffers.  SPMD: every rank calls the same entry point at the
 * same time with ITS OWN request (a rank with nothing to ask passes batch / num_ids = 0).
 * `graph` is this rank's shard of one edge type (out-edges of the vertices it owns, GLOBAL
 * destination ids, global edge ids); `features` its shard of one node type's rows, with the
 * raw ids as id map.  Either may be NULL when only the other operator family is used.
 * Results are bit-identical to the unpartitioned operator for every world size: a sampled
 * row draws from the random stream of its index in the ORIGINAL request (glx_sample_ex), and
 * aggregation reduces on the requester, in request order, over rows fetched from
 *   (1) this rank's own shard,
 *   (2) the HOT-ROW REPLICA: a copy, on every GPU, of the rows of a caller-chosen id set
 *       (glx_dist_store_set_cache; glx_dist_hot_ids picks the top-K vertices by global
 *       in-degree) -- in power-law graphs a few percent of the rows take most accesses, and
 *   (3) the HALO: the remaining remote ids, deduplicated on the device, requested from their
 *       owners (ids out, rows back: the halo-vertex feature exchange).
 * One store must not be used from two host threads at once; use one store (and one
 * communicator) per concurrently used stream. */
typedef struct glx_dist_store glx_dist_store;
GLX_API int glx_dist_store_create(glx_comm* comm, const glx_graph* graph, const glx_features* features,
                                  glx_dist_store** out);
GLX_API void glx_dist_store_destroy(glx_dist_store* st);
/* Collective.  hot_ids[n] (identical on every rank; host or device) -> every rank fetches the
 * rows from their owners once and keeps them.  n = 0 drops the replica. */
GLX_API int glx_dist_store_set_cache(glx_dist_store* st, const int64_t* hot_ids, int64_t n, float default_attr,
                                     int ptr_kind, void* stream);
/* Graph replica: complete adjacency rows of a set of (hot) vertices on this GPU, as a glx_graph the caller built with
 * explicit vertex ids -- every row with exactly the edges, weights and edge ids its owner holds (hub vertices of a
 * power-law graph are both the rows requests ask for most and cheap to hold everywhere: the hybrid-cut idea on top of
 * the hash partition of graphlearn/src/core/partition/hash_partitioner.h:33-92).  glx_dist_sample then serves the
 * request rows the replica knows locally -- same draws, the random stream is the row's index in the request -- and
 * only the rest travels to its owner.  Requests with a filter and InDegreeSampler keep the full exchange.  The store
 * borrows `replica` (NULL detaches it); the caller keeps it alive and destroys it.  Not collective. */
GLX_API int glx_dist_store_set_graph_replica(glx_dist_store* st, const glx_graph* replica);
/* Collective.  Builds such a replica from the shards themselves: every owner cuts the rows of its vertices in
 * hot_ids[n] (the same list on every rank; host or device) out of its shard -- neighbours, ITS edge ids and weights, in
 * storage order -- and the pieces are all-gathered; *out is a new glx_graph over the hot vertices (ids unknown to their
 * owner become empty rows), with its own alias tables, identical on every rank.  The caller owns it
 * (glx_graph_destroy) and attaches it with glx_dist_store_set_graph_replica.  The load-time counterpart of the
 * per-request exchange, as glx_dist_store_set_cache is for features. */
GLX_API int glx_dist_build_graph_replica(glx_dist_store* st, const int64_t* hot_ids, int64_t n, int ptr_kind,
                                         void* stream, glx_graph** out);
/* Rows of the last glx_dist_sample on this rank: all, served by the graph replica, sent to another rank. */
GLX_API int glx_dist_last_sample_rows(const glx_dist_store* st, int64_t* rows, int64_t* from_replica, int64_t* remote);
/* Collective.  The `want` destination ids with the largest in-degree summed over all shards
 * of the store's graph (ties: smaller id first), the same list on every rank, in descending
 * order of in-degree; *n_out <= want.  ids_out is a HOST array of `want` entries. */
GLX_API int glx_dist_hot_ids(glx_dist_store* st, int64_t want, int64_t* ids_out, int64_t* n_out, void* stream);
/* Collective.  InDegreeSampler (in_degree_sampler.cc:33-114) weighs a neighbour by its in-degree in the WHOLE
 * edge type (GraphStorage::GetInDegree, topo_statics.cc:62-69); a shard only sees the edges it owns.  This
 * sums the per-destination counts over all shards (pairs routed to the destination's owner, reduced there,
 * answers routed back) and builds `shard`'s per-row alias tables -- and glx_graph_in_degrees -- from the
 * totals.  `shard` must be the graph the store was created with; MUTATES it like glx_graph_enable_in_degree.
 * Until it has run, glx_dist_sample refuses GLX_SAMPLER_IN_DEGREE on a store with more than one shard. */
GLX_API int glx_dist_enable_in_degree(glx_dist_store* st, glx_graph* shard, void* stream);
/* Collective.  DistributeRunner<SamplingRequest, SamplingResponse>::Run: glx_sample_filtered's
 * arguments (filter may be NULL), request rows routed to their owners and back. */
GLX_API int glx_dist_sample(glx_dist_store* st, int sampler, const int64_t* src, int32_t batch, int32_t k,
                            int padding_mode, int64_t default_neighbor_id, uint64_t seed, uint64_t call_counter,
                            const glx_filter* filter, int64_t* nbr_out, int64_t* eid_out, int ptr_kind,
                            void* stream);
/* Collective.  The same runner for FullSampler's sparse response (full_sampler.cc:28-97; the segments + values of
 * sampling_request.cc:198-224, stitched row by row as SamplingResponse::Stitch does for the sparse case): request rows
 * to their owners, the owners' row sizes back -> degrees_out[batch], offsets_out[batch + 1] (last entry = the total);
 * glx_dist_sample_full additionally brings the values back, row i at offsets_out[i] of nbr_out / eid_out, which hold
 * `capacity` entries (InvalidArgument when the response is larger: ask _sizes first).  Host or device pointers; both
 * return when their outputs are valid. */
GLX_API int glx_dist_sample_full_sizes(glx_dist_store* st, const int64_t* src, int32_t batch, int32_t max_limit,
                                       int32_t* degrees_out, int64_t* offsets_out, int ptr_kind, void* stream);
GLX_API int glx_dist_sample_full(glx_dist_store* st, const int64_t* src, int32_t batch, int32_t max_limit,
                                 int32_t* degrees_out, int64_t* offsets_out, int64_t* nbr_out, int64_t* eid_out,
                                 int64_t capacity, int ptr_kind, void* stream);
/* glx_dist_sample_full with a filter (full_sampler.cc:66-84 behind DistributeRunner): every row's filter value travels
 * with its id, the owners answer with glx_sample_full_filtered -- same sizes as without a filter, reserved neighbours
 * padded up to them, rows whose neighbours all hit default-filled.  Every rank passes a filter of the same kind (or none). */
GLX_API int glx_dist_sample_full_filtered(glx_dist_store* st, const int64_t* src, int32_t batch, int32_t max_limit,
                                          int32_t* degrees_out, int64_t* offsets_out, int padding_mode,
                                          int64_t default_neighbor_id, const glx_filter* filter, int64_t* nbr_out,
                                          int64_t* eid_out, int64_t capacity, int ptr_kind, void* stream);
/* Collective.  GetDegree for DESTINATION ids over the shards (GraphStorage::GetInDegree, topo_statics.cc:62-69;
 * degree_getter.cc): degrees_out[n] = edges pointing to ids[i] summed over ALL shards (held by the id's owner,
 * llabs(id) % P, in a table built collectively on first use); ids nobody points to: 0. */
GLX_API int glx_dist_in_degrees(glx_dist_store* st, const int64_t* ids, int32_t n, int32_t* degrees_out, int ptr_kind,
                                void* stream);
/* Collective.  The negative samplers' candidate list over the WHOLE edge type on every rank
 * (random_negative_sampler.cc:30-63, in_degree_negative_sampler.cc:29-135: GetAllDstIds() / GetAllInDegrees() of the
 * unpartitioned storage): every destination id of any shard, ids ascending, uniform (by_in_degree = 0) or weighted by
 * the in-degree summed over all shards.  The result is an ordinary glx_negative, identical on every rank and equal to
 * glx_negative_create(ids ascending, global in-degrees) on an unpartitioned store; destroy with glx_negative_destroy. */
GLX_API int glx_dist_negative_create(glx_dist_store* st, int by_in_degree, void* stream, glx_negative** out);
/* glx_negative_sample across the shards.  GLX_NEG_EXCLUDE_NEIGHBORS is collective: the rows travel to the owners of their
 * source ids (whose adjacency is the exclusion set; the shard needs glx_graph_enable_negative) and draw there from their
 * ORIGINAL row's random stream; the other modes run locally.  Every rank passes the same `table` contents and `count`;
 * answers equal the unpartitioned glx_negative_sample on that table for every shard count. */
GLX_API int glx_dist_negative_sample(glx_dist_store* st, const glx_negative* table, int exclude, const int64_t* src,
                                     int32_t batch, int32_t count, int64_t default_neighbor_id, uint64_t seed,
                                     uint64_t call_counter, int64_t* out, int ptr_kind, void* stream);
/* Collective.  The RandomWalk operator (random_walk.cc:30-276) across the shards, glx_random_walk's layout and draws.
 * DeepWalk (p = q = 1 as RandomWalkRequest::IsDeepWalk decides, :168-190): step t is one partitioned RandomSampler request
 * with neighbor_count 1 and call counter call_counter + t, walker i drawing from stream i.  node2vec (:192-272): per step
 * ONE partitioned FullSampler request (limit full_nbr_num) brings the first full_nbr_num neighbours of the vertices the
 * walkers stand on -- with their edge weights -- to the requesters; the parents' lists are the previous step's; the step
 * (bias by 1/p, 1, 1/q, alias table, one draw) then runs on the requester with the single store's arithmetic: walks equal
 * glx_random_walk on the unpartitioned graph for every shard count.  glx_dist_random_walk uses the reference's flag
 * defaults (DefaultFullNbrNum 100, DefaultWeight 0: config.cc:102,111), _ex takes them. */
GLX_API int glx_dist_random_walk(glx_dist_store* st, const int64_t* seeds, int32_t batch, int32_t walk_len, float p, float q,
                                 int64_t default_neighbor_id, uint64_t seed, uint64_t call_counter, int64_t* walks_out,
                                 int ptr_kind, void* stream);
GLX_API int glx_dist_random_walk_ex(glx_dist_store* st, const int64_t* seeds, int32_t batch, int32_t walk_len, float p,
                                    float q, int32_t full_nbr_num, float default_weight, int64_t default_neighbor_id,
                                    uint64_t seed, uint64_t call_counter, int64_t* walks_out, int ptr_kind, void* stream);
/* Collective.  DistributeRunner<AggregatingRequest, AggregatingResponse>::Run with
 * glx_aggregate's arguments; segment_ids == NULL means num_segments equal segments of
 * num_ids / num_segments consecutive ids (a dense sampler response). */
GLX_API int glx_dist_aggregate(glx_dist_store* st, int op, const int64_t* node_ids, const int32_t* segment_ids,
                               int32_t num_ids, int32_t num_segments, float default_attr, float* emb_out,
                               int32_t* cnt_out, int ptr_kind, void* stream);
/* Collective.  The same request served the way the reference's servers serve it (SURVEY 8(e) design R, kept as the
 * ablation of the halo exchange above): AggregatingRequest::Partition routes every (id, segment id) to the id's owner
 * (aggregating_request.cc:117-170), each owner runs Aggregator::Aggregate over what it received, and
 * AggregatingResponse::Stitch folds the world-size partial [num_segments, dim] results and counts on the requester
 * (:172-213; glx_aggregate_stitch).  Per request it moves 12 B per remote id out and world * num_segments * (4 dim + 4) B
 * back instead of 4 dim B per distinct remote id: cheaper when segments are long (fan-out >> world).  Max / Min / counts
 * equal the single-store operator exactly; Sum / Mean / Prod fold per-shard partial results, so they differ from it by
 * the floating-point reassociation the reference's distributed mode has as well (<= 1e-5 relative at the fan-outs of
 * BASELINE's configs).  A segment none of whose ids a shard owns contributes nothing from that shard (SURVEY 8(a)
 * quirk 8: the reference folds a default row in there).  Replicas (hot rows, graph) are not consulted. */
GLX_API int glx_dist_aggregate_partial(glx_dist_store* st, int op, const int64_t* node_ids, const int32_t* segment_ids,
                                       int32_t num_ids, int32_t num_segments, float default_attr, float* emb_out,
                                       int32_t* cnt_out, int ptr_kind, void* stream);
/* The same in two halves, for software pipelining (device pointers only).  _begin is the collective part:
 * it resolves the ids and fetches the halo rows into buffer set `slot` (0 <= slot < GLX_DIST_SLOTS); it may run
 * on the stream that PRODUCED the ids, one or more requests ahead of the reduce.  _end is local: the segmented
 * reduce over the slot's rows, on any stream ordered after _begin's.  The caller keeps a slot untouched between
 * its _begin and the completion of its _end.  glx_dist_aggregate == _begin + _end on slot 0.  Why: with the
 * halo exchange of request i+1 running beside the HBM-bound reduce of request i, link time and the probe passes
 * leave the critical path. */
#define GLX_DIST_SLOTS 8
GLX_API int glx_dist_aggregate_begin(glx_dist_store* st, int32_t slot, const int64_t* node_ids, int32_t num_ids,
                                     float default_attr, void* stream);
GLX_API int glx_dist_aggregate_end(glx_dist_store* st, int32_t slot, int op, const int32_t* segment_ids,
                                   int32_t num_segments, float* emb_out, int32_t* cnt_out, void* stream);
/* ABI 3.  The reduce over ids [first_id, first_id + num_ids) of the request begun in `slot`: ONE _begin (one count
 * exchange, one deduplicated halo fetch) can serve several aggregating requests whose ids were handed over back to back
 * -- the hop-2 and the hop-1 neighbours of one sampling step.  release != 0 ends the slot's request (as _end does). */
GLX_API int glx_dist_aggregate_end_range(glx_dist_store* st, int32_t slot, int32_t first_id, int32_t num_ids, int release,
                                         int op, const int32_t* segment_ids, int32_t num_segments, float* emb_out,
                                         int32_t* cnt_out, void* stream);
/* Collective.  LookupNodes in distributed mode (node_lookuper.cc:24-52 behind
 * DistributeRunner): out[n * dim] rows of ids owned by any shard. */
GLX_API int glx_dist_lookup(glx_dist_store* st, const int64_t* node_ids, int64_t n, float default_attr,
                            float* out, int ptr_kind, void* stream);
/* Where the ids of this store's LAST glx_dist_aggregate / glx_dist_lookup came from, and what
 * crossed the links because of it (this rank's view).  The call synchronises nothing: read it
 * after the stream has drained. */
typedef struct glx_dist_stats {
  int64_t ids;             /* request size */
  int64_t from_replica;    /* served by the hot-row replica */
  int64_t from_own_shard;  /* owned by this rank (or unknown everywhere: default row) */
  int64_t remote;          /* remote and not replicated (with repeats) */
  int64_t remote_distinct; /* ... distinct: the ids sent, = halo rows received */
  int64_t served_rows;     /* halo rows this rank gathered for its peers */
  int64_t bytes_sent;      /* ids out + rows out over the transport, self-copies excluded */
  int64_t bytes_received;
  int64_t exchange_rounds; /* transport rounds of the last row exchange (message-size limit) */
  /* ABI 3.  Cumulative since the store was created: every partitioned request exchanges its per-shard counts once and the
   * calling host thread waits there for the slowest rank (the reference's RunInParallel waits for every remote shard's RPC
   * the same way, op_runner.h:86-117) -- how many such waits, and how long they took in total. */
  int64_t host_syncs;
  int64_t host_stall_us;
} glx_dist_stats;
GLX_API int glx_dist_last_stats(const glx_dist_store* st, glx_dist_stats* out);

/* ---- ABI 4: partitioned sampling WITHOUT a count exchange.  DistributeRunner waits for every shard's reply before it
 * goes on (RunInParallel, core/runner/op_runner.h:86-117); glx_dist_sample does the same once per request, at the count
 * exchange that tells the ranks how many rows each message carries -- a blocking host wait per hop.  A ledger removes it
 * for calls whose place in the step repeats: the i-th glx_dist_sample call after a confirmation point goes through the
 * count exchange once and records the largest bucket any rank sent to any owner; later calls at position i send
 * FIXED-capacity messages (that bucket x 1.25 + 1024 rows, padded with ids no shard knows), the owners answer every slot,
 * and each requester keeps the answers of its real rows -- no count leaves the device, the host never waits.  Whether a
 * call speculates depends only on its position and on what the ranks learned together, never on this rank's request
 * length: a rank with a shorter tail batch (or an empty request) enters the same collectives as its peers.  Whether every bucket fitted its
 * message is recorded in a device word and travels with the NEXT count exchange of any store attached to the same
 * ledger (the aggregation's, glx_dist_aggregate_begin; or glx_dist_confirm): that call returns GLX_ABORTED on every rank
 * when any bucket of any rank did not fit, and the results of all speculated calls since the previous successful
 * exchange are void -- redo them (same call counters: same answers); the capacities have been raised to what was
 * needed, so the repeat fits (voided calls still in flight on other streams need no draining: an abort starts a new
 * epoch and their flags are not heeded).  Results of confirmed calls are bit-identical to the count-exchange path.
 * Contract (SPMD lockstep): every rank issues the same SEQUENCE of glx_dist_sample calls and confirmation points, with
 * the same neighbor_count, sampler, padding, seed and call_counter -- the owners serve all requesters with their OWN
 * parameters; request lengths may differ between the ranks.  (Ranks that issue different sequences of calls enter
 * different collectives: that is a hang on RCCL, with or without a ledger.)
 * A digest of those parameters travels with the confirmation; ranks that disagree get GLX_ABORTED and the ledger stops
 * speculating for good.  Filtered requests, glx_dist_sample_full and random walks always take the count exchange.
 * One ledger per rank, shared by that rank's stores; calls that use it come from one host thread. */
typedef struct glx_dist_ledger glx_dist_ledger;
GLX_API int glx_dist_ledger_create(int device, glx_dist_ledger** out);
GLX_API void glx_dist_ledger_destroy(glx_dist_ledger* l);
/* NULL detaches.  The ledger must outlive the stores attached to it. */
GLX_API int glx_dist_store_set_ledger(glx_dist_store* st, glx_dist_ledger* l);
/* A confirmation point of its own (collective; one count exchange on st's communicator): GLX_OK = every speculated
 * call enqueued before it, on streams ordered before `stream`, is valid. */
GLX_API int glx_dist_confirm(glx_dist_store* st, void* stream);
typedef struct glx_dist_ledger_stats {
  int64_t speculated;  /* glx_dist_sample calls that skipped their count exchange */
  int64_t learned;     /* ... that took it and recorded a request shape */
  int64_t aborted;     /* confirmations that failed */
  int64_t holding;     /* 1: the ranks' requests disagreed once; no more speculation */
  double largest_share; /* largest per-owner share of a request recorded so far */
} glx_dist_ledger_stats;
GLX_API int glx_dist_ledger_get_stats(const glx_dist_ledger* l, glx_dist_ledger_stats* out);
/* Test knob: capacity = share x slack + pad rows (defaults 1.25, 1024).  slack < 1 forces the abort path. */
GLX_API int glx_dist_ledger_set_slack(glx_dist_ledger* l, double slack, int64_t pad_rows);

/* ---- request plans: a multi-hop sample (+ aggregate) request as ONE graph launch.  Replaces the
 * per-batch walk over a chain of DAG nodes (core/runner/dag_node_runner.cc:32-109: each node builds a
 * request, runs its operator, feeds the next) and the hop loop of NeighborSampler.get
 * (python/sampler/neighbor_sampler.py:93-127) for fixed-shape requests. -------------------------
 * glx_plan_create captures, for `batch` seeds: hop h = glx_sample(graphs[h], sampler, hop h-1's
 * neighbours, fanouts[h], ...) with random stream (seed, call_counter + h) -- exactly glx_sample_hops --
 * and, when `features` is given, for every hop h (deepest first) glx_aggregate(features[h], agg_op) of hop
 * h's neighbours into the fanouts[h]-sized segments of hop h-1's rows (features[h] = the node type hop h
 * reaches).  The kernels are recorded once into a hipGraph; glx_plan_run(seeds, call_counter) replays it on
 * `stream`: one launch instead of 2 * num_hops, which is what a small batch (B0 <= 8192) needs -- its kernels
 * take microseconds, launching them one by one takes longer.  Outputs live in plan-owned device buffers
 * (glx_plan_output) valid until the next run; results are bit-identical to the separate calls.  A plan is
 * bound to one device and must not run concurrently with itself. */
typedef struct glx_plan glx_plan;
GLX_API int glx_plan_create(const glx_graph* const* graphs, int32_t num_hops, int sampler, const int32_t* fanouts,
                            int32_t batch, int padding_mode, int64_t default_neighbor_id, uint64_t seed,
                            const glx_features* const* features, int agg_op, float default_attr, glx_plan** out);
/* seeds[batch]: DEVICE pointer, read when the graph executes. */
GLX_API int glx_plan_run(glx_plan* p, const int64_t* seeds, uint64_t call_counter, void* stream);
/* Device buffers of hop `hop`: nbr / eid [rows * fanout], emb [rows * dim] and cnt [rows] (NULL without
 * aggregation); rows = request rows of the hop.  Any out pointer may be NULL. */
GLX_API int glx_plan_output(const glx_plan* p, int32_t hop, int64_t** nbr, int64_t** eid, float** emb, int32_t** cnt,
                            int64_t* rows, int32_t* fanout);
GLX_API void glx_plan_destroy(glx_plan* p);

/* ---- kernel timing: the device-side counterpart of the reference's
 * PROFILING(key) scope timers (common/base/profiling.h:24-71). ------------
 * While enabled (per host thread), every glx_sample / glx_aggregate /
 * glx_lookup call brackets its dominant kernel -- and only that kernel -- with
 * a pair of HIP events on the call's stream.  glx_profile_collect synchronises
 * those events, writes the launch durations of `kind` (oldest first, at most
 * `cap`) to ms_out, stores their number in *count and forgets them. */
#define GLX_KERNEL_SAMPLE 0
#define GLX_KERNEL_AGGREGATE 1
#define GLX_KERNEL_LOOKUP 2
GLX_API int glx_profile_enable(int on);
GLX_API int glx_profile_collect(int kind, float* ms_out, int32_t cap, int32_t* count);

/* ---- conditional negative sampling: replaces ConditionalNegativeSampler (core/operator/sampler/
 * conditional_negative_sampler.cc:37-161) with its ConditionTable (condition_table.cc:65-148) and AttributeNodesMap
 * (attribute_nodes_map.h:74-127). ----------------------------------------------------------------------------
 * glx_cond_table_create: the candidates ids[num_ids] (the edge type's destination ids in first-appearance order, or a
 *   node type's ids: StorageWrapper::GetIds) with weights[num_ids] (in-degrees / node weights; NULL = 1 each, the
 *   "random" strategy) and, per selected attribute column c, the candidates' attribute values as int64 keys
 *   cand_keys[c * num_ids + u] (an int attribute itself, a float's bit pattern with -0 folded onto +0, a string's
 *   dictionary index: equal keys <=> equal attribute values).  Groups candidates by key per column and builds one alias
 *   table per group plus the default table over all candidates -- the reference's lazily built, per-type cached
 *   ConditionTable + AliasMethod pair -- on the device.
 * glx_cond_negative_sample: out[batch * count].  Row i is sampled AFTER rows 0..i-1: the exclusion set grows through the
 *   request (all dst ids up front when batch_share; else the neighbours of src i in `g` -- may be NULL -- and dst i are
 *   added before row i samples; `unique` also adds every accepted id) exactly as the reference's nbr_set does.  Per
 *   column c the row takes (int32)(count * props[c]) ids from the group whose key is dst_keys[i * num_cols + c]
 *   (INT64_MIN: no such group) with AttributeNodesMap::Sample's retry schedule (retry_times = GLOBAL_FLAG(
 *   SamplingRetryTimes)); the rest of the row comes from the default table, then default_neighbor_id.  props is a HOST
 *   array of num_cols floats; the other pointers follow ptr_kind.  Draws: stream (seed, call_counter, i); the layout is
 *   spelled out in DESIGN.md section 5.  The call returns when `out` is valid. */
typedef struct glx_cond_table glx_cond_table;
GLX_API int glx_cond_table_create(int device, int64_t num_ids, const int64_t* ids, const float* weights, int32_t num_cols,
                                  const int64_t* cand_keys, int ptr_kind, void* stream, glx_cond_table** out);
GLX_API void glx_cond_table_destroy(glx_cond_table* t);
GLX_API int glx_cond_negative_sample(const glx_cond_table* t, const glx_graph* g, const int64_t* src, const int64_t* dst,
                                     const int64_t* dst_keys, const float* props, int32_t batch, int32_t count,
                                     int batch_share, int unique, int32_t retry_times, int64_t default_neighbor_id,
                                     uint64_t seed, uint64_t call_counter, int64_t* out, int ptr_kind, void* stream);

/* ---- induced sub-graph: replaces SubGraphSampler::InduceSubGraph (core/operator/subgraph/subgraph_sampler.cc:34-95).
 * nodes[n] is the sub-graph's node list (SubGraphSampler::Process, subgraph_sampler.h:36-78: the seeds, then the sorted set
 * of every neighbour the hop-wise FullSampler calls returned -- duplicates between the two parts are kept, as in the
 * reference); offsets[n + 1] / nbr / eid are FullSampler's response for `nodes` with limit GLOBAL_FLAG(DefaultFullNbrNum)
 * (glx_sample_full, or glx_dist_sample_full across shards).  For every node i, in order, and every j in list order whose
 * id is among row i's neighbours, the entries (i, j, e) and (j, i, e) are appended, e = the edge id of the LAST slot of row
 * i holding that neighbour (node2edge[nbrs[k]] = edge_ids[k], :60-64).  *count_out (host) = the number of entries, 2 per
 * match, whatever `capacity` is (capacity 0: count only).  Entries are written in whole pairs: when the total exceeds
 * `capacity`, the first `capacity` rounded down to even entries of the full answer are written and nothing beyond them
 * is touched, the odd slot included.  INT64_MIN is the empty-slot key of the per-row tables: a node or neighbour with
 * that id matches nothing, where the reference would match the two (the answer is the reference's for the same rows
 * without those neighbours).  The call returns when the outputs are valid. */
GLX_API int glx_subgraph_induce(int device, const int64_t* nodes, int32_t n, const int64_t* offsets, const int64_t* nbr,
                                const int64_t* eid, int32_t* row_out, int32_t* col_out, int64_t* eid_out, int64_t capacity,
                                int64_t* count_out, int ptr_kind, void* stream);

/* ---- frontier dedup: the distinct node set of a sampled batch, every sampled slot's position in it, and the set's
 * size after each frontier.  Stands in for what the reference's loaders do on the host or with sort-based tensor calls:
 * examples/pytorch/tgn/temporal_batch_loader.py:99-121 (torch.cat(...).unique() and an `assoc` array as long as the node
 * type) and the node set of SubGraphSampler::Process (core/operator/subgraph/subgraph_sampler.h:47-72).
 * parts[num_parts] (a host array of 1 .. 16 data pointers) and part_len[num_parts] (host) describe ONE stream
 * x[0 .. n) = part 0, part 1, ... (a loader passes the seeds and every hop's neighbour ids; nothing is concatenated).
 * n <= 2^31 - 1; empty parts (pointer may be NULL) and n == 0 are legal.  Every int64 value is an id, INT64_MIN included.
 *   nodes_out[capacity n]    the distinct ids in order of first occurrence in x; entries from m on are not written
 *   inverse_out[n] or NULL   nodes_out[inverse_out[i]] == x[i]
 *   part_end_out[num_parts]  distinct ids among parts 0 .. p, so nodes_out[0 .. part_end_out[p]) is the node set of
 *                            the first p + 1 parts; m = part_end_out[num_parts - 1].  All zeros when n == 0.
 * The three outputs are a function of the input alone (no sort; a hash table keeps the smallest position of every id,
 * DESIGN.md 4).  The data pointers AND part_end_out follow ptr_kind: a device-pointer call leaves the counts in device
 * memory and never waits for the device; a host-pointer call returns with everything in host memory.  The workspace
 * comes from the calling thread's per-(device, stream) cache: no allocation once it has grown to the largest n. */
GLX_API int glx_unique(int device, const int64_t* const* parts, const int64_t* part_len, int32_t num_parts,
                       int64_t* nodes_out, int64_t* inverse_out, int64_t* part_end_out, int ptr_kind, void* stream);

/* ---- memory-system probes: the measured ceilings the kernels above are priced against -- an addition of this
 * engine with no counterpart in the reference (its PROFILING timers, common/base/profiling.h:24-71, time scopes; they
 * do not measure the machine).  Each probe allocates its own buffers on `device`, runs 2 untimed + `reps` timed
 * launches between two HIP events on `stream` and reports the bytes one launch moves and its average duration.
 *   GLX_PROBE_STREAM_READ  reads a `bytes` buffer once (16 B per lane, grid-strided)          moved = bytes
 *   GLX_PROBE_COPY         b = a                                                             moved = 2 * bytes
 *   GLX_PROBE_TRIAD        a = b + s * c  (STREAM triad)                                     moved = 3 * bytes
 *   GLX_PROBE_GATHER32     `units` aligned 32-byte records from uniformly random positions of a `bytes` table, 16 B
 *                          written per record: EdgeWeightSampler's access per output slot (alias_method.cc:117-121 on
 *                          one packed record)                                                moved = 48 * units
 *   GLX_PROBE_GATHER_ROWS  `units` rows of `unit_bytes` from uniformly random rows of a `bytes` table, reduced ten to
 *                          one in registers: the gather of Aggregator::Aggregate (aggregator.cc:25-59) without cache
 *                          reuse                                                             moved = 1.1 * units * unit_bytes */
#define GLX_PROBE_STREAM_READ 0
#define GLX_PROBE_COPY 1
#define GLX_PROBE_TRIAD 2
#define GLX_PROBE_GATHER32 3
#define GLX_PROBE_GATHER_ROWS 4
GLX_API int glx_probe_bandwidth(int device, int kind, int64_t bytes, int64_t units, int32_t unit_bytes, int32_t reps,
                                double* moved_bytes_out, double* avg_ms_out, void* stream);

/* Measurement knobs of the aggregation launch (Aggregator::Aggregate, aggregator.cc:25-59), for A/B probes inside one
 * process.  Each is read from the environment once (first use) and may be set here at any time; 0 restores the
 * product's default.  Names: "agg_mfma" (GLX_AGG_MFMA), "agg_unroll" (GLX_AGG_UNROLL), "agg_slices" (GLX_AGG_SLICES),
 * "agg_legacy" (GLX_AGG_LEGACY), "agg_segs" (GLX_AGG_SEGS), "agg_xcd_slices" (GLX_AGG_XCD_SLICES), "agg_occupancy"
 * (GLX_AGG_OCCUPANCY), "agg_store" (GLX_AGG_STORE), "agg_repeats" (GLX_AGG_REPEATS: Max / Min load every position of a
 * segment = 1, only the first occurrence of every row = 2, by segment length = 0); of the bookkeeping of explicit
 * segment_ids: "seg_scan_parent" (GLX_SEG_SCAN_PARENT = 1: the scan and fix-up launches of a thread per four ids and per
 * segment), "seg_scan_wgs" (GLX_SEG_SCAN_WGS: at most this many workgroups in the scan's grid).  Results are
 * bit-identical under every setting.  Unknown name: GLX_INVALID_ARGUMENT.
 * Test knobs of the side paths, same rules, -1 restores the default: "cond_sequential" (GLX_COND_SEQUENTIAL),
 * "dist_no_bitmap" (GLX_DIST_NO_BITMAP), "filter_span_cap" (GLX_FILTER_SPAN_CAP), "filter_dedup_min_rows"
 * (GLX_FILTER_DEDUP_MIN_ROWS), "idmap_hash_only" (GLX_IDMAP_HASH_ONLY: feature tables created afterwards keep a hash table
 * even when their ids are an arithmetic progression); of the partitioned aggregation's resolve pass: "resolve_ids"
 * (GLX_RESOLVE_IDS: ids per thread per pass), "resolve_blocks" (GLX_RESOLVE_BLOCKS: workgroups), "resolve_set_share"
 * (GLX_RESOLVE_SET_SHARE: the halo id set holds at least n / 1024 of a request's ids), "resolve_peek" (GLX_RESOLVE_PEEK = 0:
 * no plain load of a set slot before the compare-and-swap), "resolve_own_first" (GLX_RESOLVE_OWN_FIRST = 1 | 0: ids this
 * rank owns skip / take the replica lookup; default: skip at world size 1 only); of the KNN search: "knn_chunk_rows",
 * "knn_query_block" (see glx_knn_search).  Test aid: "seg_epochs_before_wrap" (the
 * calling thread's segment-word buffers hand out `value` more epochs before their counter wraps). */
GLX_API int glx_tune(const char* name, int32_t value);

#ifdef __cplusplus
}
#endif
#endif /* GLX_H_ */
