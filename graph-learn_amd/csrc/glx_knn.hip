// glx exact KNN search over a device feature table: the reference's KnnOperator (contrib/knn/knn_op.cc:29-59) on its
// flat index (contrib/knn/flat_index.cc:26-55), without faiss and without a second copy of the table -- the "index" is
// the glx_features matrix as it lies in HBM.
//
// Contract (DESIGN.md 4, K-knn; include/glx.h).  For a query q and a stored row x (a half element upcast exactly):
//   ip   = +0.0f, then ip = fmaf(q[c], x[c], ip) for c ascending: ONE chain over all columns.  That is the numerics of
//          v_mfma_f32_32x32x2_f32 (D = fma(a_k1, b_k1, fma(a_k0, b_k0, C))) and of a VALU fmaf loop, so the score kernel
//          below runs the even columns on the matrix cores and an odd last column as a VALU fmaf on the accumulator.
//   IP   dist = ip, larger is better.   L2  dist = max-with-NaN-kept(0, fmaf(-2, ip, qn + xn)), smaller is better.
//   order  better dist first; equal dist (+0 == -0): smaller storage row first; NaN after every number, by row.
// The order is TOTAL, so each (query, row) has one 64-bit key -- an order-preserving image of dist in the high word,
// the row in the low word -- and "the k best" is "the k smallest keys" whatever order candidates arrive in.  That is why
// the integer counters that compact survivors below do not disturb determinism.  No float atomics anywhere.
//
// Schedule.  The table is walked in chunks of rows.  Per chunk, knn_score_kernel computes a (128 queries x 128 rows)
// tile per workgroup and keeps only scores not worse than the query's current k-th best (equality passes: the row may
// win the tie); survivors land in a per-query candidate buffer.  knn_select_kernel (one workgroup per query) folds the
// candidates into the running sorted list and refreshes the threshold.  knn_finish_kernel turns keys into (id, dist).
//
// The key, the order, the sorted-batch fold and the output rules live in glx_knn.h, shared with the two indexes
// (glx_knn_ivf.hip, glx_knn_ivfpq.hip); those reach this file's kernels through knn_search_device, knn_prepare_norms
// and knn_finish.
#include <mutex>

#include "glx_knn.h"

#pragma clang fp contract(off)

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kBQ = 128;          // queries per workgroup tile
constexpr int kBR = 128;          // table rows per workgroup tile
constexpr int kLd = kBQ + 1;      // LDS pitch of a k-major tile
constexpr uint32_t kNoThr = 0xffffffffu;   // "none yet": everything passes
constexpr int32_t kDefaultChunkRows = 8192;
constexpr int32_t kMaxChunkRows = 1 << 18;
constexpr int32_t kDefaultFirstChunkRows = 2048;  // the first chunk passes whole: keep it small

// The four constants of the schedule that glx_knn.h defines, restated and held to its values at compile time.  They
// serve readers that take the schedule's constants from this file alone: the previous release's
// tests/test_knn_cpu.py is one, and it must still collect and pass against this library.
namespace restated {
constexpr int kBK = 32;
constexpr int kSortN = 1024;
constexpr int kSelThreads = 512;
constexpr size_t kCandBudgetBytes = (size_t)256 << 20;
static_assert(kBK == ::kBK && kSortN == ::kSortN && kSelThreads == ::kSelThreads &&
                  kCandBudgetBytes == ::kCandBudgetBytes,
              "the constants restated for tests/test_knn_cpu.py differ from glx_knn.h");
}  // namespace restated

// out[r] = the chain of row r with itself; one lane per row (built once per owned table; per search for a view and for
// the request's queries)
__global__ __launch_bounds__(256) void knn_norms_kernel(KnnTable t, float* __restrict__ out) {
  const int64_t r = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (r >= t.num_rows) return;
  const int64_t base = glx_swizzle_row(r, t.swizzle_rows) * t.stride;
  float acc = 0.0f;
  for (int32_t c = 0; c < t.dim; ++c) {
    const float x = knn_elem(t.X, t.dtype, base + c);
    acc = __builtin_fmaf(x, x, acc);
  }
  out[r] = acc;
}

__global__ __launch_bounds__(256) void knn_init_kernel(KnnArgs a) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i < (int64_t)a.nq * a.KP) a.run[i] = kNoKey;
  if (i < a.nq) {
    a.thr[i] = kNoThr;
    a.cnt[i] = 0;
  }
}

// One (128 queries x 128 rows) tile of scores for rows [row0, row1) of the table, filtered into the candidate buffers.
// Four waves as 2 x 2, each owning 64 x 64 = four 32x32 accumulators that live across the WHOLE column loop.  A holds
// queries (the accumulator's row index), B holds table rows (the accumulator's column index = the lane), so for one
// accumulator register the 32 lanes of a half-wave share a query: one ballot and one counter add per (half-wave,
// register).  Rows past row1, queries past nq and columns past dim are loaded as zeros and never multiplied into a
// kept score: a score is per (query, row), the column loop stops at dim, and masked outputs are dropped.
template <int DT>
__global__ __launch_bounds__(256) void knn_score_kernel(KnnArgs a, int32_t row0, int32_t row1) {
  typedef typename AggElem<DT>::raw raw_t;
  __shared__ float As[kBK][kLd];
  __shared__ float Bs[kBK][kLd];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int wq = (w & 1) * 64, wr = (w >> 1) * 64;
  const int32_t qbase = blockIdx.y * kBQ;
  const int32_t rbase = row0 + blockIdx.x * kBR;
  const int32_t dim = a.t.dim, dim_even = dim & ~1;
  const raw_t* const X = static_cast<const raw_t*>(a.t.X);
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
  const int lc = t & 31, lr = t >> 5;
  for (int32_t k0 = 0; k0 < dim; k0 += kBK) {
    __syncthreads();  // the previous tile has been consumed
    const int32_t c = k0 + lc;
    const bool cok = c < dim;
#pragma unroll
    for (int j = 0; j < kBQ / 8; ++j) {
      const int r = lr + 8 * j;
      const int32_t q = qbase + r, row = rbase + r;
      float qa = 0.0f, xb = 0.0f;
      if (cok && q < a.nq) qa = a.queries[(int64_t)q * dim + c];
      if (cok && row < row1) xb = AggElem<DT>::up(X[glx_swizzle_row(row, a.t.swizzle_rows) * a.t.stride + c]);
      As[lc][r] = qa;
      Bs[lc][r] = xb;
    }
    __syncthreads();
    int32_t left = dim_even - k0;
    const int steps = (left < kBK ? (left > 0 ? left : 0) : kBK) / 2;
    for (int s = 0; s < steps; ++s) {
      const int kk = 2 * s + half;
      const float a0 = As[kk][wq + l31], a1 = As[kk][wq + 32 + l31];
      const float b0 = Bs[kk][wr + l31], b1 = Bs[kk][wr + 32 + l31];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    if ((dim & 1) && k0 + kBK >= dim) {
      // the odd last column: a real fmaf on the accumulator.  A zero-padded MFMA step would turn a chain that
      // underflowed to -0.0f into +0.0f and make inf * 0 a NaN.
      const int kk = dim - 1 - k0;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const float xb = Bs[kk][wr + j * 32 + l31];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float qa = As[kk][wq + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half];
            acc[i][j][r] = __builtin_fmaf(qa, xb, acc[i][j][r]);
          }
        }
    }
  }
  // ---- epilogue: threshold filter, survivors as keys into the per-query buffers
  const uint32_t below = (1u << l31) - 1u;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int32_t row = rbase + wr + j * 32 + l31;
    const bool rok = row < row1;
    const float xn = (a.metric == GLX_KNN_L2 && rok) ? a.xn[row] : 0.0f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int32_t q = qbase + wq + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const bool qok = q < a.nq;
        float dist = acc[i][j][r];
        uint32_t thr = 0;
        if (qok) {
          thr = a.thr[q];
          if (a.metric == GLX_KNN_L2) dist = knn_l2(dist, a.qn[q], xn);
        }
        const uint32_t ord = knn_ord(__float_as_uint(dist), a.metric);
        const bool pass = qok && rok && ord <= thr;
        const uint64_t ball = __ballot(pass);
        if (ball == 0) continue;  // wave-uniform
        const uint32_t mine = (uint32_t)(ball >> (32 * half));
        uint32_t base = 0;
        if (l31 == 0 && mine != 0) base = atomicAdd(&a.cnt[q], (uint32_t)__popc(mine));
        base = __shfl(base, half * 32);
        if (pass) {
          const uint32_t pos = base + (uint32_t)__popc(mine & below);
          // the key from the image the threshold test already holds: knn_key(dist, ...) would compute it again
          if (pos < (uint32_t)a.cap) a.cand[(int64_t)q * a.cap + pos] = knn_key(ord, row);
        }
      }
    }
  }
}

__global__ __launch_bounds__(kSelThreads) void knn_select_kernel(KnnArgs a) {
  __shared__ uint64_t srun[kSortN];
  __shared__ uint64_t v[kSortN];
  const int q = blockIdx.x, t = threadIdx.x;
  uint32_t n = a.cnt[q];
  if (n == 0) return;  // nothing beat the threshold: list and threshold stand
  if (n > (uint32_t)a.cap) n = (uint32_t)a.cap;
  uint64_t* const run = a.run + (int64_t)q * a.KP;
  const uint64_t* const cand = a.cand + (int64_t)q * a.cap;
  for (int i = t; i < a.KP; i += kSelThreads) srun[i] = run[i];
  knn_fold(srun, v, a.KP, (int64_t)n, t, [&](int64_t i) { return cand[i]; });
  for (int i = t; i < a.KP; i += kSelThreads) run[i] = srun[i];
  if (t == 0) {
    const uint64_t kth = srun[a.k - 1];
    a.thr[q] = kth == kNoKey ? kNoThr : (uint32_t)(kth >> 32);
    a.cnt[q] = 0;
  }
}

// keys -> (node id, dist); one lane per output slot.  The image in a key gives back every number's bits except a
// zero's sign; zeros and NaNs are recomputed as the contract's chain on the VALU (the same numerics).
__global__ __launch_bounds__(256) void knn_finish_kernel(KnnArgs a, const int64_t* __restrict__ row_ids, int64_t id_base,
                                                         int64_t id_step, int64_t* __restrict__ ids_out,
                                                         float* __restrict__ dist_out) {
  const int64_t o = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (o >= (int64_t)a.nq * a.k) return;
  const int32_t q = (int32_t)(o / a.k), j = (int32_t)(o % a.k);
  const uint64_t key = a.run[(int64_t)q * a.KP + j];
  if (key == kNoKey) return knn_emit_absent(o, a.metric, ids_out, dist_out);
  const int64_t row = (int64_t)(uint32_t)key;
  const uint32_t ord = (uint32_t)(key >> 32);
  uint32_t bits = knn_unord(ord, a.metric);
  if (ord == 0xffffffffu || (bits & 0x7fffffffu) == 0) {
    const int64_t base = glx_swizzle_row(row, a.t.swizzle_rows) * a.t.stride;
    const float* const qv = a.queries + (int64_t)q * a.t.dim;
    float ip = 0.0f;
    for (int32_t c = 0; c < a.t.dim; ++c) ip = __builtin_fmaf(qv[c], knn_elem(a.t.X, a.t.dtype, base + c), ip);
    bits = __float_as_uint(a.metric == GLX_KNN_L2 ? knn_l2(ip, a.qn[q], a.xn[row]) : ip);
  }
  dist_out[o] = __uint_as_float(bits);
  ids_out[o] = knn_row_id(row, row_ids, id_base, id_step);
}

// KnnResponse::Merge (knn_request.cc:186-202): the k best of num_parts lists per query; ties to the lower part, then
// to the earlier position, id == -1 entries are absent.  One workgroup per query.
struct KnnMergeArgs {
  const int64_t* ids;  // [num_parts, nq, k]
  const float* dist;
  int64_t* ids_out;    // [nq, k]
  float* dist_out;
  int32_t num_parts, nq, k, KP, metric;
};

__global__ __launch_bounds__(kSelThreads) void knn_merge_kernel(KnnMergeArgs a) {
  __shared__ uint64_t srun[kSortN];
  __shared__ uint64_t v[kSortN];
  const int q = blockIdx.x, t = threadIdx.x;
  for (int i = t; i < a.KP; i += kSelThreads) srun[i] = kNoKey;
  auto slot = [&](int64_t i) { return ((i / a.k) * a.nq + q) * a.k + i % a.k; };
  knn_fold(srun, v, a.KP, (int64_t)a.num_parts * a.k, t, [&](int64_t i) {
    const int64_t at = slot(i);
    if (a.ids[at] == -1) return kNoKey;
    return knn_key(a.dist[at], (uint32_t)i, a.metric);
  });
  for (int j = t; j < a.k; j += kSelThreads) {
    const uint64_t key = srun[j];
    const int64_t o = (int64_t)q * a.k + j;
    if (key == kNoKey) {
      knn_emit_absent(o, a.metric, a.ids_out, a.dist_out);
    } else {
      const int64_t at = slot((int64_t)(uint32_t)key);
      a.ids_out[o] = a.ids[at];
      a.dist_out[o] = a.dist[at];
    }
  }
}

std::mutex g_norm_mu;

// xn of an OWNED table (nothing in the C ABI rewrites its rows): built once, on the first L2 search, on that search's
// stream; later searches on other streams wait for the build's event.  Concurrent first searches are serialised by the
// lock around the queueing (not the work).  A view reads the caller's matrix as it is at each call -- a halo buffer, an
// embedding table under glx_embedding_update -- so its xn is built per search into the call's workspace instead.
int knn_table_norms(const glx_features* f, const KnnTable& t, hipStream_t s, const float** xn) {
  std::lock_guard<std::mutex> lk(g_norm_mu);
  if (f->knn_xn == nullptr) {
    float* p = nullptr;
    hipEvent_t ev = nullptr;
    GLX_HIP(hipMalloc(&p, (size_t)(t.num_rows > 0 ? t.num_rows : 1) * sizeof(float)));
    hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess && t.num_rows > 0) {
      knn_norms_kernel<<<(unsigned)((t.num_rows + 255) / 256), 256, 0, s>>>(t, p);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(ev, s);
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(s);
      (void)hipFree(p);
      if (ev) (void)hipEventDestroy(ev);
      glx_set_error("building the table's L2 norms failed: %s", hipGetErrorString(e));
      return GLX_INTERNAL;
    }
    f->knn_xn_ready = ev;
    f->knn_xn = p;
  } else {
    GLX_HIP(hipStreamWaitEvent(s, static_cast<hipEvent_t>(f->knn_xn_ready), 0));
  }
  *xn = f->knn_xn;
  return GLX_OK;
}

}  // namespace

int knn_prepare_norms(const glx_features* f, bool needs_l2, const float* d_q, int32_t num_queries, float* qn,
                      float* xn_ws, hipStream_t s, const float** xn) {
  if (!needs_l2) return GLX_OK;
  const KnnTable t = knn_table(f);
  if (f->owns_x) {
    const int rc = knn_table_norms(f, t, s, xn);
    if (rc != GLX_OK) return rc;
  } else {
    if (t.num_rows > 0) knn_norms_kernel<<<(unsigned)((t.num_rows + 255) / 256), 256, 0, s>>>(t, xn_ws);
    *xn = xn_ws;
  }
  const KnnTable qt{d_q, f->dim, 0, num_queries, f->dim, GLX_DTYPE_F32};
  knn_norms_kernel<<<(unsigned)((num_queries + 255) / 256), 256, 0, s>>>(qt, qn);
  return GLX_OK;
}

void knn_finish(const KnnArgs& a, const glx_features* f, int64_t* d_ids, float* d_dist, hipStream_t s) {
  const bool arith = f->idmap.keys == nullptr && f->idmap.step > 0;
  knn_finish_kernel<<<(unsigned)(((int64_t)a.nq * a.k + 255) / 256), 256, 0, s>>>(
      a, f->knn_row_ids, arith ? f->idmap.base : 0, arith ? f->idmap.step : 0, d_ids, d_dist);
}

int knn_search_device(const glx_features* f, int metric, const float* d_q, int32_t num_queries, int32_t k,
                      int64_t* d_ids, float* d_dist, hipStream_t s) {
  KnnArgs a;
  memset(&a, 0, sizeof(a));
  a.t = knn_table(f);
  a.k = k;
  a.KP = knn_pow2_at_least(k);
  a.metric = metric;
  const GlxSideKnobs& knobs = glx_side_knobs();
  const int64_t knob_chunk = knobs.knn_chunk_rows.load(std::memory_order_relaxed);
  const int64_t knob_qb = knobs.knn_query_block.load(std::memory_order_relaxed);
  auto round_up = [](int64_t x, int64_t m) { return (x + m - 1) / m * m; };
  // The candidate buffer holds qb queries x chunk rows under the budget.  Many queries: blocks of 4,096 and chunks
  // of 8,192 rows.  Few queries: the chunk grows instead (up to 2^18 rows), so that a launch still fills the device and a
  // 10 M-row table is not a thousand launches of a few workgroups.
  const int64_t rows_up = round_up(a.t.num_rows > 0 ? a.t.num_rows : 1, kBR);
  const int64_t budget_keys = (int64_t)(kCandBudgetBytes / sizeof(uint64_t));
  int64_t qb, chunk;
  if (knob_chunk > 0) {
    chunk = round_up(knob_chunk, kBR);
    qb = budget_keys / chunk / kBQ * kBQ;
  } else {
    qb = round_up(num_queries, kBQ);
    if (qb > budget_keys / kDefaultChunkRows) qb = budget_keys / kDefaultChunkRows;
    chunk = budget_keys / qb / kBR * kBR;
    if (chunk > kMaxChunkRows) chunk = kMaxChunkRows;
  }
  if (chunk > rows_up) chunk = rows_up;
  if (knob_qb > 0) qb = round_up(knob_qb, kBQ);
  if (qb < kBQ) qb = kBQ;
  if (qb > round_up(num_queries, kBQ)) qb = round_up(num_queries, kBQ);
  const int64_t first = knob_chunk > 0 ? chunk : (chunk < kDefaultFirstChunkRows ? chunk : kDefaultFirstChunkRows);
  a.cap = (int32_t)chunk;

  // workspace slot 1
  float *qn, *xn_ws;
  auto layout = [&](KnnCarve c) {
    qn = c.take<float>(num_queries);
    xn_ws = c.take<float>(a.t.num_rows, metric == GLX_KNN_L2 && !f->owns_x);
    a.thr = c.take<uint32_t>(qb);
    a.cnt = c.take<uint32_t>(qb);
    a.run = c.take<uint64_t>(qb * a.KP);
    a.cand = c.take<uint64_t>(qb * a.cap);
    return c.off;
  };
  GlxScratch ws;
  int rc = ws.alloc(layout(KnnCarve{nullptr}), s, 1);
  if (rc != GLX_OK) return rc;
  layout(KnnCarve{ws.as<char>()});
  rc = knn_prepare_norms(f, metric == GLX_KNN_L2, d_q, num_queries, qn, xn_ws, s, &a.xn);
  if (rc != GLX_OK) return rc;
  for (int64_t q0 = 0; q0 < num_queries; q0 += qb) {
    a.nq = (int32_t)(num_queries - q0 < qb ? num_queries - q0 : qb);
    a.queries = d_q + q0 * f->dim;
    a.qn = qn + q0;
    knn_init_kernel<<<(unsigned)(((int64_t)a.nq * a.KP + 255) / 256), 256, 0, s>>>(a);
    for (int64_t row0 = 0; row0 < a.t.num_rows;) {
      const int64_t len = row0 == 0 ? first : chunk;
      const int64_t row1 = row0 + len < a.t.num_rows ? row0 + len : a.t.num_rows;
      const dim3 grid((unsigned)((row1 - row0 + kBR - 1) / kBR), (unsigned)((a.nq + kBQ - 1) / kBQ));
      GLX_KNN_LAUNCH_DT(&rc, a.t.dtype, knn_score_kernel, grid, 256, s, a, (int32_t)row0, (int32_t)row1);
      if (rc != GLX_OK) return rc;
      knn_select_kernel<<<(unsigned)a.nq, kSelThreads, 0, s>>>(a);
      row0 = row1;
    }
    knn_finish(a, f, d_ids + q0 * k, d_dist + q0 * k, s);
  }
  return GLX_OK;
}

int knn_not_capturing(hipStream_t s) {
  if (s == nullptr) return GLX_OK;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) == hipSuccess) {
    GLX_REQUIRE(cs == hipStreamCaptureStatusNone, "KNN search does not run under graph capture");
  }
  return GLX_OK;
}

extern "C" int glx_knn_search(const glx_features* f, int metric, const float* queries, int32_t num_queries, int32_t k,
                              int64_t* ids_out, float* dist_out, int ptr_kind, void* stream) {
  GLX_REQUIRE(f != nullptr, "features is NULL");
  GLX_KNN_REQUIRE();
  GLX_REQUIRE(f->num_rows < INT32_MAX, "num_rows must be < 2^31");
  return knn_search_entry(f->device, f->dim, queries, num_queries, k, ids_out, dist_out, ptr_kind, stream,
                          [&](const float* d_q, int64_t* d_ids, float* d_dist, hipStream_t s) {
                            return knn_search_device(f, metric, d_q, num_queries, k, d_ids, d_dist, s);
                          });
}

extern "C" int glx_knn_merge(int device, int metric, int32_t num_parts, const int64_t* ids, const float* dist,
                             int32_t num_queries, int32_t k, int64_t* ids_out, float* dist_out, int ptr_kind,
                             void* stream) {
  GLX_KNN_REQUIRE();
  GLX_REQUIRE(num_parts >= 1, "num_parts must be at least 1, got %d", num_parts);
  GLX_REQUIRE((int64_t)num_parts * k < INT32_MAX, "num_parts * k must be < 2^31");
  GLX_REQUIRE(num_queries == 0 || (ids != nullptr && dist != nullptr), "ids or dist is NULL");
  GLX_REQUIRE(num_queries == 0 || (ids_out != nullptr && dist_out != nullptr), "ids_out or dist_out is NULL");
  int rc = glx_init_device(device);
  if (rc != GLX_OK) return rc;
  if (num_queries == 0) return GLX_OK;
  GlxDeviceGuard guard(device);
  GLX_KNN_CALL_BEGIN(guard, device, ptr_kind == GLX_PTR_DEVICE, stream);
  GlxHostStage st(device, ptr_kind, stream, GlxHostStage::ADMIT);
  KnnMergeArgs a;
  const size_t n_in = (size_t)num_parts * num_queries * k;
  st.in(&a.ids, ids, n_in);
  st.in(&a.dist, dist, n_in);
  st.out(&a.ids_out, ids_out, (size_t)num_queries * k);
  st.out(&a.dist_out, dist_out, (size_t)num_queries * k);
  rc = st.begin();
  if (rc == GLX_OK) {
    a.num_parts = num_parts;
    a.nq = num_queries;
    a.k = k;
    a.KP = knn_pow2_at_least(k);
    a.metric = metric;
    knn_merge_kernel<<<(unsigned)num_queries, kSelThreads, 0, st.s>>>(a);
  }
  return st.finish(rc);
}
