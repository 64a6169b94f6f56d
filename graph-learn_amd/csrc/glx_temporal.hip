// glx temporal neighbour sampling: "the neighbours of v over edges that happened before t", one cutoff per request row.
// Stands in for the time-blind topk sample of the reference's TGN loader (examples/pytorch/tgn/temporal_batch_loader.py:
// 70-80) and answers per row what the timestamp filter answers for request row 0's value only (filter.cc:74-82), over
// the timestamp-ascending rows of memory_adj_matrix.cc:129-148.
//
// Latency-bound work: a binary search of a 138 K-slot hub row is 17 dependent HBM loads.  A lane group of W lanes owns
// one request row and searches W-ary: every round the W lanes load W evenly spaced probes of the live interval at once
// and a ballot narrows it by W + 1, so a row takes about log_{W+1}(deg) round trips.  The row's (start, deg) is loaded
// by the group's first lane and shared through cross-lane reads.  Positions inside a row are 64-bit.
#include "glx_lane_groups.h"

namespace {

struct TemporalArgs {
  GlxIdMap map;
  GlxRowDir dir;
  const int64_t* row_ptr;
  const GlxAdj* adj;
  const int64_t* ts;        // per CSR slot, ascending inside every row
  const int64_t* src;       // [batch] raw ids
  const int64_t* cutoff;    // [batch]
  const int64_t* rng_rows;  // nullptr: request row i uses stream i
  // Hops: request row i is slot i % parent_k of the previous hop's row i / parent_k, which holds a sampled edge only
  // below that row's count.  nullptr: every request row is live.
  const int32_t* parent_cnt;
  int32_t parent_k;
  int64_t* nbr_out;
  int64_t* eid_out;  // may be nullptr
  int64_t* ts_out;   // may be nullptr
  int32_t* cnt_out;  // may be nullptr
  int64_t default_nbr;
  int64_t default_ts;
  uint64_t seed;
  uint64_t cc;
  int32_t batch;
  int32_t k;
  int32_t inclusive;
};

// Whether slot timestamp `v` lies before the cutoff.
__device__ __forceinline__ bool temporal_before(int64_t v, int64_t t, int32_t inclusive) {
  return inclusive ? v <= t : v < t;
}

template <int W, int STRATEGY>
__global__ __launch_bounds__(256) void glx_temporal_kernel(TemporalArgs a) {
  const int lane = threadIdx.x & 63;
  const int l = lane & (W - 1);
  const int base = lane - l;
  const uint64_t wmask = (W == 64) ? ~0ull : ((1ull << W) - 1ull);
  const int64_t i = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / W;
  if (i >= a.batch) return;  // whole groups leave together: W divides the block
  // ---- the row: one span load per group
  int64_t start = 0, deg = 0, t = 0;
  if (l == 0) {
    bool live = true;
    if (a.parent_cnt) {
      const int64_t pr = i / a.parent_k;
      live = (int32_t)(i - pr * a.parent_k) < a.parent_cnt[pr];
    }
    if (live) {
      const GlxRowSpan span = glx_row_span(a.dir, a.map, a.row_ptr, a.src[i]);
      start = span.start;
      deg = span.deg;
      t = a.cutoff[i];
    }
  }
  start = __shfl(start, base);
  deg = __shfl(deg, base);
  t = __shfl(t, base);
  const int64_t* __restrict__ row_ts = a.ts + start;
  // ---- c = the length of the row's prefix before the cutoff.  Invariant: every position below lo lies before it, no
  // position from hi on does; all loads are at positions in [lo, hi), a sub-range of [0, deg).
  int64_t lo = 0, hi = deg;
  while (hi - lo > W) {
    const uint64_t n = (uint64_t)(hi - lo);  // < 2^32: (l + 1) * n stays far below 2^64
    const int64_t p = lo + (int64_t)(((uint64_t)(l + 1) * n) / (uint64_t)(W + 1));
    const bool before = temporal_before(row_ts[p], t, a.inclusive);
    const int m = __popcll((__ballot(before) >> base) & wmask);  // probes before the cutoff: probes 0 .. m - 1
    // Past probe m - 1 and up to probe m.  Consecutive probes are at least n / (W + 1) >= 1 apart, so lo <= hi holds
    // for any m in [0, W] -- also the m a row that is not ascending yields.
    const int64_t nlo = m > 0 ? lo + (int64_t)(((uint64_t)m * n) / (uint64_t)(W + 1)) + 1 : lo;
    const int64_t nhi = m < W ? lo + (int64_t)(((uint64_t)(m + 1) * n) / (uint64_t)(W + 1)) : hi;
    lo = nlo;
    hi = nhi;
  }
  bool before = false;
  if (lo + l < hi) before = temporal_before(row_ts[lo + l], t, a.inclusive);
  const int64_t c = lo + __popcll((__ballot(before) >> base) & wmask);
  // ---- the k slots: lanes j = l, l + W, ...
  const uint32_t rr = (STRATEGY == GLX_TEMPORAL_UNIFORM && a.rng_rows) ? (uint32_t)a.rng_rows[i] : (uint32_t)i;
  const int64_t obase = i * (int64_t)a.k;
  for (int32_t j = l; j < a.k; j += W) {
    int64_t pick = -1;
    if (STRATEGY == GLX_TEMPORAL_UNIFORM) {
      // random_sampler.cc:61-63 with the prefix length in place of the degree
      if (c > 0) pick = (int64_t)glx_bounded(glx_draw64(a.seed, a.cc, rr, (uint32_t)j), (uint64_t)c);
    } else {
      if (j < c) pick = c - 1 - j;  // latest first
    }
    GlxAdj rec = GlxAdj{a.default_nbr, -1};
    int64_t tv = a.default_ts;
    if (pick >= 0) {
      rec = a.adj[start + pick];
      tv = row_ts[pick];
    }
    a.nbr_out[obase + j] = rec.nbr;
    if (a.eid_out) a.eid_out[obase + j] = rec.eid;
    if (a.ts_out) a.ts_out[obase + j] = tv;
  }
  if (l == 0 && a.cnt_out) {
    if (STRATEGY == GLX_TEMPORAL_UNIFORM) a.cnt_out[i] = c > 0 ? a.k : 0;
    else a.cnt_out[i] = (int32_t)(c < a.k ? c : a.k);
  }
}

int temporal_device(const glx_graph* g, int strategy, TemporalArgs a, hipStream_t s) {
  a.map = g->map();
  a.dir = g->dir();
  a.row_ptr = g->row_ptr;
  a.adj = g->adj;
  a.ts = g->ts;
  GlxKernelTimer timer(GLX_KERNEL_SAMPLE, s);
  glx_for_group(glx_group_for(a.k), [&](auto gw) {
    constexpr int W = decltype(gw)::value;
    const int64_t threads = (int64_t)a.batch * W;
    const unsigned blocks = (unsigned)((threads + 255) / 256);
    if (strategy == GLX_TEMPORAL_UNIFORM) glx_temporal_kernel<W, GLX_TEMPORAL_UNIFORM><<<blocks, 256, 0, s>>>(a);
    else glx_temporal_kernel<W, GLX_TEMPORAL_RECENT><<<blocks, 256, 0, s>>>(a);
  });
  timer.stop();
  GLX_HIP(hipGetLastError());
  return GLX_OK;
}

int temporal_check_graph(const glx_graph* g) {
  GLX_REQUIRE(g != nullptr, "graph is NULL");
  GLX_REQUIRE(g->ts != nullptr || g->num_edges == 0,
              "temporal sampling needs a graph that keeps timestamps (glx_graph_build_ordered with "
              "GLX_ORDER_TIMESTAMP_ASC, or glx_graph_set_timestamps)");
  return GLX_OK;
}

int temporal_check_common(int strategy, int32_t batch, int ptr_kind) {
  GLX_REQUIRE(strategy == GLX_TEMPORAL_RECENT || strategy == GLX_TEMPORAL_UNIFORM, "bad temporal strategy %d", strategy);
  GLX_REQUIRE(batch >= 0, "negative batch");
  GLX_REQUIRE(ptr_kind == GLX_PTR_HOST || ptr_kind == GLX_PTR_DEVICE, "bad ptr_kind");
  return GLX_OK;
}

}  // namespace

extern "C" int glx_graph_has_timestamps(const glx_graph* g, int* has) {
  GLX_REQUIRE(g != nullptr && has != nullptr, "NULL argument");
  *has = g->ts != nullptr ? 1 : 0;
  return GLX_OK;
}

extern "C" int glx_sample_temporal(const glx_graph* g, int strategy, const int64_t* src, const int64_t* cutoff,
                                   const int64_t* rng_rows, int32_t batch, int32_t k, int inclusive,
                                   int64_t default_neighbor_id, int64_t default_timestamp, uint64_t seed,
                                   uint64_t call_counter, int64_t* nbr_out, int64_t* eid_out, int64_t* ts_out,
                                   int32_t* cnt_out, int ptr_kind, void* stream) {
  GLX_REQUIRE(g != nullptr, "graph is NULL");
  int rc = temporal_check_common(strategy, batch, ptr_kind);
  if (rc != GLX_OK) return rc;
  GLX_REQUIRE(k >= 1, "neighbor_count must be at least 1");
  // Tensor sizes are int32 in the reference (tensor.h:47): batch*k must fit.
  GLX_REQUIRE((int64_t)batch * k <= INT32_MAX, "batch * neighbor_count exceeds int32 (tensor.h:47)");
  rc = temporal_check_graph(g);
  if (rc != GLX_OK) return rc;
  if (batch == 0) return GLX_OK;
  GLX_REQUIRE(src && cutoff && nbr_out, "NULL data pointer");
  GlxDeviceGuard guard(g->device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", g->device);

  TemporalArgs a;
  a.parent_cnt = nullptr;
  a.parent_k = 1;
  a.default_nbr = default_neighbor_id;
  a.default_ts = default_timestamp;
  a.seed = seed;
  a.cc = call_counter;
  a.batch = batch;
  a.k = k;
  a.inclusive = inclusive ? 1 : 0;
  GlxHostStage st(g->device, ptr_kind, stream, GlxHostStage::ADMIT);
  const size_t n_out = (size_t)batch * k;
  st.in(&a.src, src, (size_t)batch);
  st.in(&a.cutoff, cutoff, (size_t)batch);
  st.in(&a.rng_rows, rng_rows, (size_t)batch);
  st.out(&a.nbr_out, nbr_out, n_out);
  st.out(&a.eid_out, eid_out, n_out);
  st.out(&a.ts_out, ts_out, n_out);
  st.out(&a.cnt_out, cnt_out, (size_t)batch);
  rc = st.begin();
  if (rc == GLX_OK) rc = temporal_device(g, strategy, a, st.s);
  return st.finish(rc);
}

extern "C" int glx_sample_temporal_hops(const glx_graph* const* graphs, int32_t num_hops, int strategy,
                                        const int64_t* seeds, const int64_t* cutoff, int32_t batch,
                                        const int32_t* fanouts, int inclusive, int64_t default_neighbor_id,
                                        int64_t default_timestamp, uint64_t seed, uint64_t call_counter,
                                        int64_t* const* nbr_out, int64_t* const* eid_out, int64_t* const* ts_out,
                                        int32_t* const* cnt_out, int ptr_kind, void* stream) {
  GLX_REQUIRE(graphs && fanouts && nbr_out, "NULL argument");
  // host-pointer staging declares up to four copies per hop (GlxHostStage holds 40 pieces)
  GLX_REQUIRE(num_hops >= 1 && num_hops <= 8, "num_hops must be in [1, 8]");
  int rc = temporal_check_common(strategy, batch, ptr_kind);
  if (rc != GLX_OK) return rc;
  const bool host = ptr_kind == GLX_PTR_HOST;
  int64_t rows = batch;
  for (int32_t h = 0; h < num_hops; ++h) {
    GLX_REQUIRE(graphs[h] != nullptr && (nbr_out[h] != nullptr || batch == 0), "hop %d: NULL graph / output", h);
    GLX_REQUIRE(graphs[h]->device == graphs[0]->device, "all hops must live on one device");
    GLX_REQUIRE(fanouts[h] >= 1, "hop %d: fanout must be at least 1", h);
    GLX_REQUIRE(rows <= INT32_MAX && rows * fanouts[h] <= INT32_MAX, "hop %d exceeds int32 slots (tensor.h:47)", h);
    rc = temporal_check_graph(graphs[h]);
    if (rc != GLX_OK) return rc;
    // the next hop reads this hop's timestamps (its cutoffs) and counts (which parent slots hold an edge)
    GLX_REQUIRE(host || batch == 0 || h + 1 == num_hops || (ts_out && ts_out[h] && cnt_out && cnt_out[h]),
                "device mode needs ts_out[%d] and cnt_out[%d]: the next hop reads them", h, h);
    rows *= fanouts[h];
  }
  if (batch == 0) return GLX_OK;
  GLX_REQUIRE(seeds && cutoff, "NULL data pointer");
  GlxDeviceGuard guard(graphs[0]->device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", graphs[0]->device);

  // Host pointers: one upload of the seeds and cutoffs, every hop sampled from the previous hop's device buffers, one
  // download per hop output.  Device pointers: the caller's outputs are the frontiers.
  GlxHostStage st(graphs[0]->device, ptr_kind, stream);
  TemporalArgs a;
  a.rng_rows = nullptr;
  a.default_nbr = default_neighbor_id;
  a.default_ts = default_timestamp;
  a.seed = seed;
  a.inclusive = inclusive ? 1 : 0;
  int64_t* d = nullptr;
  st.in(&a.src, seeds, (size_t)batch);
  st.in(&a.cutoff, cutoff, (size_t)batch);
  if (host) {
    size_t total = 0;  // in int64 words: nbr, eid, ts per slot and an int32 count per row (rounded up to a word)
    int64_t n = batch;
    for (int32_t h = 0; h < num_hops; ++h) {
      total += 3 * (size_t)(n * fanouts[h]) + ((size_t)n + 1) / 2;
      n *= fanouts[h];
    }
    st.scratch(&d, total);
  }
  rc = st.begin();
  int64_t* cursor = d;
  int64_t n = batch;
  a.parent_cnt = nullptr;
  a.parent_k = 1;
  for (int32_t h = 0; h < num_hops && rc == GLX_OK; ++h) {
    const int32_t k = fanouts[h];
    const int64_t slots = n * k;
    if (host) {
      a.nbr_out = cursor;
      a.eid_out = cursor + slots;
      a.ts_out = cursor + 2 * slots;
      a.cnt_out = reinterpret_cast<int32_t*>(cursor + 3 * slots);
      cursor += 3 * slots + (n + 1) / 2;
    } else {
      a.nbr_out = nbr_out[h];
      a.eid_out = eid_out ? eid_out[h] : nullptr;
      a.ts_out = ts_out ? ts_out[h] : nullptr;
      a.cnt_out = cnt_out ? cnt_out[h] : nullptr;
    }
    a.batch = (int32_t)n;
    a.k = k;
    a.cc = call_counter + (uint64_t)h;
    rc = temporal_device(graphs[h], strategy, a, st.s);
    if (host) {
      st.out_after(nbr_out[h], a.nbr_out, (size_t)slots * 8);
      if (eid_out && eid_out[h]) st.out_after(eid_out[h], a.eid_out, (size_t)slots * 8);
      if (ts_out && ts_out[h]) st.out_after(ts_out[h], a.ts_out, (size_t)slots * 8);
      if (cnt_out && cnt_out[h]) st.out_after(cnt_out[h], a.cnt_out, (size_t)n * 4);
    }
    a.src = a.nbr_out;
    a.cutoff = a.ts_out;
    a.parent_cnt = a.cnt_out;
    a.parent_k = k;
    n = slots;
  }
  return st.finish(rc);
}
