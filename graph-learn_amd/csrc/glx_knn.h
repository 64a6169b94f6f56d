// glx KNN core: what the exact search (glx_knn.hip), the IVF-Flat index (glx_knn_ivf.hip) and the IVF-PQ index
// (glx_knn_ivfpq.hip) share.  The contract's pieces -- the key, the order, the chain over gathered rows, the sorted-batch
// fold, the padding and id rules -- are written here once, as inline device functions every file compiles for itself.
// A kernel stays in one file; another file reaches it through a host launcher declared at the end of this header.
// Including this header turns floating-point contraction off for the rest of the translation unit: the contract's
// chains are written fmaf by fmaf.
#ifndef GLX_KNN_H_
#define GLX_KNN_H_
#include "glx_common.h"

#pragma clang fp contract(off)

constexpr int kBK = 32;           // columns per LDS tile
constexpr int kSortN = 1024;      // keys per sorted batch of the select kernel = the largest k
constexpr int kSelThreads = 512;  // one compare-exchange per thread and step
constexpr uint64_t kNoKey = ~0ull;  // an empty slot of a running list: above every real key (rows are < 2^31)
constexpr size_t kCandBudgetBytes = (size_t)256 << 20;
constexpr int kIvfRows = 256;         // rows per gathered scoring pass, one lane each
constexpr int kIvfLd = kIvfRows + 1;  // LDS pitch of a k-major row tile
constexpr size_t kIvfStageBytes = (size_t)64 << 20;  // float32 staging of the rows one assign call takes as queries

// Order-preserving image of dist: ascending unsigned = better first.  +0 and -0 share one image, every NaN maps to
// the largest one.  IP (larger is better) is the complement of the L2 image over the numbers.
__host__ __device__ __forceinline__ uint32_t knn_ord(uint32_t bits, int metric) {
  if ((bits & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  if (bits == 0x80000000u) bits = 0;
  const uint32_t asc = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
  return metric == GLX_KNN_L2 ? asc : ~asc;
}
// the float behind a number's image (a zero comes back as +0)
__host__ __device__ __forceinline__ uint32_t knn_unord(uint32_t ord, int metric) {
  const uint32_t asc = metric == GLX_KNN_L2 ? ord : ~ord;
  return (asc & 0x80000000u) ? (asc & 0x7fffffffu) : ~asc;
}
// the one 64-bit key of a (query, row): the image of dist above the row
__device__ __forceinline__ uint64_t knn_key(uint32_t ord, uint32_t row) { return ((uint64_t)ord << 32) | row; }
__device__ __forceinline__ uint64_t knn_key(float dist, uint32_t row, int metric) {
  return knn_key(knn_ord(__float_as_uint(dist), metric), row);
}

__device__ __forceinline__ float knn_elem(const void* X, int dtype, int64_t i) {
  if (dtype == GLX_DTYPE_F32) return static_cast<const float*>(X)[i];
  if (dtype == GLX_DTYPE_BF16) return AggElem<GLX_DTYPE_BF16>::up(static_cast<const uint16_t*>(X)[i]);
  if (dtype == GLX_DTYPE_F8E4M3) return AggElem<GLX_DTYPE_F8E4M3>::up(static_cast<const uint8_t*>(X)[i]);
  if (dtype == GLX_DTYPE_F8E5M2) return AggElem<GLX_DTYPE_F8E5M2>::up(static_cast<const uint8_t*>(X)[i]);
  return AggElem<GLX_DTYPE_F16>::up(static_cast<const _Float16*>(X)[i]);
}

__device__ __forceinline__ float knn_l2(float ip, float qn, float xn) {
  const float s = qn + xn;
  const float d = __builtin_fmaf(-2.0f, ip, s);
  return d < 0.0f ? 0.0f : d;  // a NaN stays a NaN
}

struct KnnTable {
  const void* X;
  int64_t stride, swizzle_rows;
  int32_t num_rows, dim;
  int dtype;
};
inline KnnTable knn_table(const glx_features* f) {
  return KnnTable{f->X, f->stride, f->swizzle_rows, (int32_t)f->num_rows, f->dim, f->dtype};
}
// a float32 table of rows x dim over device memory the caller holds: centroids, codebooks, staged residuals
inline glx_features knn_f32_view(int device, float* p, int64_t rows, int32_t dim) {
  glx_features v{};
  v.device = device;
  v.num_rows = rows;
  v.dim = dim;
  v.stride = dim;
  v.X = p;
  v.dtype = GLX_DTYPE_F32;
  v.elem_size = 4;
  return v;
}

struct KnnArgs {
  KnnTable t;
  const float* queries;  // [nq, dim] of this query block
  const float* qn;       // [nq] (L2)
  const float* xn;       // [num_rows] (L2)
  uint32_t* thr;         // [nq] image of the current k-th best, kNoThr = none yet
  uint32_t* cnt;         // [nq] candidates of the current chunk
  uint64_t* cand;        // [nq, cap]
  uint64_t* run;         // [nq, KP] running list, ascending, kNoKey = empty
  int32_t nq, cap, KP, k, metric;
};

// ---- the k smallest keys, one workgroup of kSelThreads ------------------------------------------------------
// v[kSortN] ascending
__device__ __forceinline__ void knn_sort_batch(uint64_t* v, int t) {
  for (int size = 2; size <= kSortN; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      const int i = 2 * t - (t & (stride - 1)), j = i + stride;
      const bool up = (i & size) == 0;
      const uint64_t x = v[i], y = v[j];
      if ((x > y) == up) {
        v[i] = y;
        v[j] = x;
      }
    }
  }
  __syncthreads();
}

// run[KP] ascending (KP a power of two <= kSortN), v[kSortN] ascending -> run = the KP smallest of both, ascending
__device__ __forceinline__ void knn_merge_batch(uint64_t* run, const uint64_t* v, int KP, int t) {
  for (int i = t; i < KP; i += kSelThreads) {
    const uint64_t x = run[i], y = v[KP - 1 - i];
    run[i] = x < y ? x : y;  // a bitonic sequence that holds the KP smallest
  }
  for (int stride = KP >> 1; stride > 0; stride >>= 1) {
    __syncthreads();
    if (t < (KP >> 1)) {
      const int i = 2 * t - (t & (stride - 1)), j = i + stride;
      const uint64_t x = run[i], y = run[j];
      if (x > y) {
        run[i] = y;
        run[j] = x;
      }
    }
  }
  __syncthreads();
}

template <typename Fetch>
__device__ __forceinline__ void knn_fold(uint64_t* run, uint64_t* v, int KP, int64_t n, int t, Fetch fetch) {
  for (int64_t base = 0; base < n; base += kSortN) {
    __syncthreads();  // v and run of the previous batch are settled
    for (int i = t; i < kSortN; i += kSelThreads) v[i] = base + i < n ? fetch(base + i) : kNoKey;
    knn_sort_batch(v, t);
    knn_merge_batch(run, v, KP, t);
  }
}

// The exact scores of up to kIvfRows table rows against one query, as keys.  The whole workgroup of kSelThreads calls
// it: for lane t < kIvfRows row_of(t) names the lane's storage row (-1 or a row past the table: none) and the lane gets
// v[t] = its key (kNoKey without a row).  The rows' column tiles are gathered through Bs (k-major, padded pitch, as
// knn_score_kernel stages its tiles), the query's columns are broadcast from qs, and each lane runs its row's chain
// with the accumulator in a register across all column tiles.  qn[q] is the query's norm, xn the table's norms (L2).
template <int DT, typename RowOf>
__device__ __forceinline__ void knn_score_gathered(const KnnTable& tab, const float* qv, const float* qn, int32_t q,
                                                   const float* xn, int metric, RowOf row_of, float (*Bs)[kIvfLd],
                                                   float* qs, int64_t* rbase, uint64_t* v) {
  typedef typename AggElem<DT>::raw raw_t;
  const int t = threadIdx.x;
  const int32_t dim = tab.dim;
  const raw_t* const X = static_cast<const raw_t*>(tab.X);
  const int lc = t & (kBK - 1), lr = t / kBK;
  int32_t row = -1;
  if (t < kIvfRows) {
    row = row_of(t);
    if (row >= tab.num_rows) row = -1;
    rbase[t] = row >= 0 ? glx_swizzle_row(row, tab.swizzle_rows) * tab.stride : (int64_t)-1;
  }
  float acc = 0.0f;
  for (int32_t k0 = 0; k0 < dim; k0 += kBK) {
    __syncthreads();  // rbase is written; the previous tile has been consumed
    const int32_t c = k0 + lc;
#pragma unroll
    for (int j = 0; j < kIvfRows / (kSelThreads / kBK); ++j) {
      const int r = lr + (kSelThreads / kBK) * j;
      const int64_t base = rbase[r];
      float xb = 0.0f;
      if (c < dim && base >= 0) xb = AggElem<DT>::up(X[base + c]);
      Bs[lc][r] = xb;
    }
    if (t < kBK) qs[t] = k0 + t < dim ? qv[k0 + t] : 0.0f;
    __syncthreads();
    if (t < kIvfRows) {
      const int n = dim - k0 < kBK ? dim - k0 : kBK;
      for (int kk = 0; kk < n; ++kk) acc = __builtin_fmaf(qs[kk], Bs[kk][t], acc);
    }
  }
  if (t < kIvfRows) {
    uint64_t key = kNoKey;
    if (row >= 0) key = knn_key(metric == GLX_KNN_L2 ? knn_l2(acc, qn[q], xn[row]) : acc, row, metric);
    v[t] = key;
  }
}

// ---- keys -> output ---------------------------------------------------------------------------------------------
// an empty slot of a result: id -1, the worst distance
__device__ __forceinline__ void knn_emit_absent(int64_t o, int metric, int64_t* ids_out, float* dist_out) {
  ids_out[o] = -1;
  dist_out[o] = metric == GLX_KNN_L2 ? __builtin_inff() : -__builtin_inff();
}
// storage row -> node id: the table's id column, its arithmetic ids (id_step > 0), or the row itself
__device__ __forceinline__ int64_t knn_row_id(int64_t row, const int64_t* row_ids, int64_t id_base, int64_t id_step) {
  return row_ids ? row_ids[row] : (id_step > 0 ? id_base + id_step * row : row);
}

// storage row of sample element t of a T-element sample of an N-row table
__device__ __forceinline__ int64_t knn_ivf_sample_row(int64_t t, int64_t N, int64_t T) { return T == N ? t : t * N / T; }

// *list = the list a (query, probe slot) scans; false when the coarse step named none.  probe == nullptr: probe slot p
// is list p.
__device__ __forceinline__ bool knn_ivf_slot_list(const int64_t* probe, int32_t q, int32_t nprobe, int32_t p,
                                                  int32_t nlist, int64_t* list) {
  *list = probe ? probe[(int64_t)q * nprobe + p] : (int64_t)p;
  return *list >= 0 && *list < nlist;
}

// launch KERNEL<DT> for a table's storage type; an unknown type launches nothing, sets the error and *(rc) = GLX_INTERNAL
#define GLX_KNN_LAUNCH_DT(rc, dtype, KERNEL, grid, block, s, ...)                                         \
  do {                                                                                                    \
    if ((dtype) == GLX_DTYPE_F32) KERNEL<GLX_DTYPE_F32><<<grid, block, 0, s>>>(__VA_ARGS__);              \
    else if ((dtype) == GLX_DTYPE_BF16) KERNEL<GLX_DTYPE_BF16><<<grid, block, 0, s>>>(__VA_ARGS__);       \
    else if ((dtype) == GLX_DTYPE_F16) KERNEL<GLX_DTYPE_F16><<<grid, block, 0, s>>>(__VA_ARGS__);         \
    else if ((dtype) == GLX_DTYPE_F8E4M3) KERNEL<GLX_DTYPE_F8E4M3><<<grid, block, 0, s>>>(__VA_ARGS__);   \
    else if ((dtype) == GLX_DTYPE_F8E5M2) KERNEL<GLX_DTYPE_F8E5M2><<<grid, block, 0, s>>>(__VA_ARGS__);   \
    else {                                                                                                \
      glx_set_error(#KERNEL ": no instantiation for storage dtype %d", (int)(dtype));                     \
      *(rc) = GLX_INTERNAL;                                                                               \
    }                                                                                                     \
  } while (0)

// ---- host side ----------------------------------------------------------------------------------------------------
struct glx_knn_ivf {
  const glx_features* f;  // the table the lists index (not owned; outlives the index)
  glx_features cview;     // a view of `centroids` for knn_search_device
  int device;
  int32_t nlist, dim;
  int64_t num_rows, longest;
  float* centroids;    // [nlist, dim]
  int32_t* list_ptr;   // [nlist + 1]
  int32_t* list_rows;  // [num_rows] storage rows by list, ascending within a list
};

inline int knn_pow2_at_least(int32_t k) {
  int p = 1;
  while (p < k) p <<= 1;
  return p;
}

// One workspace layout, written once and run twice: over base == nullptr to size it (`off` ends as the byte count), then
// over the leased base to place it.  Every piece starts 256-byte aligned; a piece that is not enabled takes nothing.
struct KnnCarve {
  char* base;
  size_t off = 0;
  template <typename T>
  T* take(size_t count, bool enabled = true) {
    if (!enabled) return nullptr;
    off = (off + 255) & ~(size_t)255;
    T* const p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += count * sizeof(T);
    return p;
  }
};

// glx_knn.hip
int knn_not_capturing(hipStream_t s);
// the exact search on device pointers (workspace slot 1)
int knn_search_device(const glx_features* f, int metric, const float* d_q, int32_t num_queries, int32_t k,
                      int64_t* d_ids, float* d_dist, hipStream_t s);
// needs_l2: qn[num_queries] = the queries' norms and *xn = the table's -- an owned table's are built once and kept, a
// view's are built into xn_ws[num_rows] on every call
int knn_prepare_norms(const glx_features* f, bool needs_l2, const float* d_q, int32_t num_queries, float* qn,
                      float* xn_ws, hipStream_t s, const float** xn);
// knn_finish_kernel: a.run[a.nq, a.KP] -> (node id of f, dist)[a.nq, a.k]
void knn_finish(const KnnArgs& a, const glx_features* f, int64_t* d_ids, float* d_dist, hipStream_t s);

// glx_knn_ivf.hip
// keys[n] = kNoKey
void knn_ivf_fill(uint64_t* keys, int64_t n, hipStream_t s);
// run[q] = the KP smallest of run[q] and part[q, P, KP], q < nq
void knn_ivf_fold(uint64_t* run, const uint64_t* part, int32_t nq, int32_t P, int32_t KP, hipStream_t s);
// both index searches' checks of nprobe, in the order the entry points report them (ix == nullptr: "index is NULL")
int knn_ivf_check_nprobe(const glx_knn_ivf* ix, int32_t nprobe, int32_t num_queries);

// What Lloyd's iterations need: the table, the centroids they move and a view of those for knn_search_device.
struct KnnTrainSet {
  KnnTable t;
  float* centroids;  // [nlist, t.dim]
  int32_t nlist;
  glx_features cview;
};
// ts.centroids = the start (centroids_init, else evenly spaced sample rows), then niter Lloyd iterations over the
// T-element sample of ts.t.  stage [chunk, dim], dist [chunk] and assign [>= T] are the caller's.
int knn_ivf_train_device(const KnnTrainSet& ts, int32_t niter, int64_t T, const float* centroids_init, int ptr_kind,
                         int64_t chunk, float* stage, float* dist, int64_t* assign, hipStream_t s);

// The slot lists of an index search hold qb queries x P probe slots x keys_per_slot keys under the flat search's
// candidate budget: as many queries per block as fit, at least one; a query whose nprobe * keys_per_slot keys alone
// exceed the budget takes its slots in passes of P that fold into the same running list.  "knn_query_block" may shrink
// the block (the bits do not depend on it).
struct KnnSlotPlan {
  int64_t qb, P;
};
inline KnnSlotPlan knn_slot_plan(int32_t nprobe, int32_t keys_per_slot, int32_t num_queries) {
  const int64_t budget_keys = (int64_t)(kCandBudgetBytes / sizeof(uint64_t));
  KnnSlotPlan plan{budget_keys / ((int64_t)nprobe * keys_per_slot), nprobe};
  if (plan.qb < 1) {
    plan.qb = 1;
    plan.P = budget_keys / keys_per_slot;
  }
  if (plan.qb > num_queries) plan.qb = num_queries;
  const int64_t knob_qb = glx_side_knobs().knn_query_block.load(std::memory_order_relaxed);
  if (knob_qb > 0 && knob_qb < plan.qb) plan.qb = knob_qb;
  return plan;
}

// The query-block and probe-pass loops of both index searches.  Per block of plan.qb queries: the coarse step names
// every query's lists (probe != nullptr; else slot p is list p), run[nq, KP] starts empty, and per pass of at most
// plan.P slots scan(q0, nq, p0, P) fills part[nq, P, KP], which is folded into run; then finish(q0, nq).
template <typename Scan, typename Finish>
int knn_ivf_passes(const glx_knn_ivf* ix, int metric, const float* d_q, int32_t num_queries, int32_t nprobe,
                   KnnSlotPlan plan, int64_t* probe, float* pdist, uint64_t* run, const uint64_t* part, int32_t KP,
                   hipStream_t s, Scan scan, Finish finish) {
  for (int64_t q0 = 0; q0 < num_queries; q0 += plan.qb) {
    const int32_t nq = (int32_t)(num_queries - q0 < plan.qb ? num_queries - q0 : plan.qb);
    if (probe) {
      const int rc = knn_search_device(&ix->cview, metric, d_q + q0 * ix->dim, nq, nprobe, probe, pdist, s);
      if (rc != GLX_OK) return rc;
    }
    knn_ivf_fill(run, (int64_t)nq * KP, s);
    for (int64_t p0 = 0; p0 < nprobe; p0 += plan.P) {
      const int32_t P = (int32_t)(nprobe - p0 < plan.P ? nprobe - p0 : plan.P);
      scan(q0, nq, (int32_t)p0, P);
      knn_ivf_fold(run, part, nq, P, KP, s);
    }
    finish(q0, nq);
  }
  return GLX_OK;
}

// ---- entry points -------------------------------------------------------------------------------------------------
#define GLX_KNN_REQUIRE()                                                                                      \
  GLX_REQUIRE(metric == GLX_KNN_L2 || metric == GLX_KNN_IP, "metric must be GLX_KNN_L2 (0) or GLX_KNN_IP (1), got %d", \
              metric);                                                                                         \
  GLX_REQUIRE(k >= 1 && k <= kSortN, "k must be in [1, %d], got %d", kSortN, k);                               \
  GLX_REQUIRE(num_queries >= 0, "negative sizes: num_queries %d", num_queries);                                \
  GLX_REQUIRE((int64_t)num_queries * k < INT32_MAX, "num_queries * k must be < 2^31");                         \
  GLX_REQUIRE(ptr_kind == GLX_PTR_HOST || ptr_kind == GLX_PTR_DEVICE, "bad ptr_kind")

// after `GlxDeviceGuard guard(device);`: the guard took, and (when the work goes to the caller's stream) no capture is
// on that stream
#define GLX_KNN_CALL_BEGIN(guard, device, on_callers_stream, stream)    \
  do {                                                                  \
    GLX_REQUIRE((guard).ok, "cannot select device %d", device);         \
    if (on_callers_stream) {                                            \
      const int cap_rc = knn_not_capturing(glx_stream(stream));         \
      if (cap_rc != GLX_OK) return cap_rc;                              \
    }                                                                   \
  } while (0)

// The tail every search entry point shares once its own arguments are checked: the buffers' null checks, the guard,
// the capture check and the staging of queries in / (ids, dist) out around body(d_q, d_ids, d_dist, stream).
template <typename Body>
int knn_search_entry(int device, int32_t dim, const float* queries, int32_t num_queries, int32_t k, int64_t* ids_out,
                     float* dist_out, int ptr_kind, void* stream, Body body) {
  GLX_REQUIRE(num_queries == 0 || queries != nullptr, "queries is NULL");
  GLX_REQUIRE(num_queries == 0 || ids_out != nullptr, "ids_out is NULL");
  GLX_REQUIRE(num_queries == 0 || dist_out != nullptr, "dist_out is NULL");
  if (num_queries == 0) return GLX_OK;
  GlxDeviceGuard guard(device);
  GLX_KNN_CALL_BEGIN(guard, device, ptr_kind == GLX_PTR_DEVICE, stream);
  GlxHostStage st(device, ptr_kind, stream, GlxHostStage::ADMIT);
  const float* d_q;
  int64_t* d_ids;
  float* d_dist;
  st.in(&d_q, queries, (size_t)num_queries * dim);
  st.out(&d_ids, ids_out, (size_t)num_queries * k);
  st.out(&d_dist, dist_out, (size_t)num_queries * k);
  int rc = st.begin();
  if (rc == GLX_OK) rc = body(d_q, d_ids, d_dist, st.s);
  return st.finish(rc);
}

#endif  // GLX_KNN_H_
