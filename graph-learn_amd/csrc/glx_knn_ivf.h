// glx IVF-Flat index over a device feature table: the reference's IVFFlatKnnIndex (contrib/knn/ivfflat_index.cc:25-55,
// made by contrib/knn/index_factory.cc:32-34) without faiss and without a second copy of the table.  Included at the END
// of glx_knn.hip: it shares that file's contract helpers (knn_ord, knn_l2, knn_elem, knn_sort_batch, knn_merge_batch,
// knn_fold, knn_finish_kernel, knn_table_norms, knn_search_device) and adds what an inverted file needs on top.
//
// Contract (DESIGN.md 4, K-knn-ivf; include/glx.h "IVF-Flat index").  The index holds centroids, list_ptr and list_rows
// (storage rows, ascending within a list).  A search scores the rows of the probed lists from the TABLE with the flat
// search's chain and keys, so with every list probed it is the flat search bit for bit, and with fewer lists it is the
// flat search restricted to the probed lists' rows.
//
// Build.  Assignments are glx's own L2 search with k = 1 over a view of the centroids (knn_search_device), rows staged
// as float32 queries in chunks; the update walks each list's sample rows in ascending order (a stable radix sort by
// list: glx_agg_transpose) and adds them sequentially.  No RNG, no float atomic.
//
// Search schedule.  One workgroup per (query, probe slot): 256 lanes own 256 list rows at a time, the rows' column
// tiles are gathered through LDS (k-major, padded pitch, as knn_score_kernel stages its tiles), each lane runs its row's
// chain against the query's columns broadcast from LDS with the accumulator in a register across all column tiles.
// The keys of 1,024 rows form one sorted batch that is merged into the slot's KP-entry list (knn_sort_batch /
// knn_merge_batch: the body of knn_fold); knn_ivf_fold_kernel then folds a query's slot lists into its running list
// and knn_finish_kernel turns keys into (id, dist).  No counters, no atomics of any kind.
#ifndef GLX_KNN_IVF_H_
#define GLX_KNN_IVF_H_
#include <vector>

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

namespace {

constexpr int kIvfRows = 256;           // list rows per scoring pass, one lane each
constexpr int kIvfLd = kIvfRows + 1;    // LDS pitch of a k-major row tile
constexpr int32_t kIvfMaxLists = 65536;
constexpr int32_t kIvfMaxProbe = 1024;  // the coarse step is a flat search with k = nprobe
constexpr size_t kIvfStageBytes = (size_t)64 << 20;  // float32 staging of the rows one assign call takes as queries
constexpr int kIvfU = 4;                // rows in flight per lane of the centroid update

// storage row of sample element t of a T-element sample of an N-row table
__device__ __forceinline__ int64_t knn_ivf_sample_row(int64_t t, int64_t N, int64_t T) { return T == N ? t : t * N / T; }

// out[j, :] = sample element e(j) upcast to float32, j < n.  seeds == 0: e(j) = t0 + j (a chunk of the sample);
// seeds > 0: e(j) = floor(j * T / seeds) (the default initial centroids).
__global__ __launch_bounds__(256) void knn_ivf_stage_kernel(KnnTable t, int64_t t0, int64_t n, int64_t T, int64_t seeds,
                                                            float* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i >= n * t.dim) return;
  const int64_t j = i / t.dim;
  const int32_t c = (int32_t)(i - j * t.dim);
  const int64_t e = seeds > 0 ? j * T / seeds : t0 + j;
  const int64_t row = knn_ivf_sample_row(e, t.num_rows, T);
  out[i] = knn_elem(t.X, t.dtype, glx_swizzle_row(row, t.swizzle_rows) * t.stride + c);
}

// One wave per list: centroid = (+0.0f + row + row + ...) / (float)n over the list's sample elements in ascending
// order, a lane per column; a list without elements keeps its centroid.
__global__ __launch_bounds__(256) void knn_ivf_update_kernel(KnnTable t, int64_t T, const int32_t* __restrict__ row_ptr,
                                                             const int32_t* __restrict__ pos, int32_t nlist,
                                                             float* __restrict__ centroids) {
  const int32_t list = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (list >= nlist) return;
  const int32_t l0 = row_ptr[list], l1 = row_ptr[list + 1];
  if (l1 <= l0) return;
  for (int32_t col = lane; col < t.dim; col += 64) {
    float acc = 0.0f;
    for (int32_t base = l0; base < l1; base += kIvfU) {
      float val[kIvfU];
#pragma unroll
      for (int u = 0; u < kIvfU; ++u) {
        val[u] = 0.0f;
        if (base + u < l1) {
          const int64_t row = knn_ivf_sample_row(pos[base + u], t.num_rows, T);
          val[u] = knn_elem(t.X, t.dtype, glx_swizzle_row(row, t.swizzle_rows) * t.stride + col);
        }
      }
#pragma unroll
      for (int u = 0; u < kIvfU; ++u) {
        if (base + u < l1) acc = acc + val[u];
      }
    }
    centroids[(int64_t)list * t.dim + col] = acc / (float)(l1 - l0);
  }
}

__global__ __launch_bounds__(256) void knn_ivf_fill_kernel(uint64_t* __restrict__ p, int64_t n) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i < n) p[i] = kNoKey;
}

__global__ __launch_bounds__(256) void knn_ivf_widen_kernel(const int32_t* __restrict__ in, int64_t n,
                                                            int64_t* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i < n) out[i] = in[i];
}

struct KnnIvfScan {
  KnnTable t;
  const float* queries;      // [nq, dim] of this query block
  const float* qn;           // [nq] (L2)
  const float* xn;           // [num_rows] (L2)
  const int32_t* list_ptr;   // [nlist + 1]
  const int32_t* list_rows;  // [num_rows]
  const int64_t* probe;      // [nq, nprobe] the lists of every query, best first; nullptr: probe slot p is list p
  uint64_t* part;            // [nq, P, KP] the sorted list of every (query, probe slot) of this pass, kNoKey = empty
  int32_t nlist, nprobe, p0, P, KP, metric;
};

// The KP best keys of one list for one query.  Block b serves query b / P and probe slot p0 + b % P.
template <int DT>
__global__ __launch_bounds__(kSelThreads) void knn_ivf_scan_kernel(KnnIvfScan a) {
  typedef typename AggElem<DT>::raw raw_t;
  __shared__ float Bs[kBK][kIvfLd];
  __shared__ float qs[kBK];
  __shared__ int64_t rbase[kIvfRows];
  __shared__ uint64_t srun[kSortN];
  __shared__ uint64_t v[kSortN];
  const int t = threadIdx.x;
  const int32_t q = (int32_t)(blockIdx.x / (uint32_t)a.P), slot = (int32_t)(blockIdx.x % (uint32_t)a.P);
  const int32_t p = a.p0 + slot;
  const int64_t list = a.probe ? a.probe[(int64_t)q * a.nprobe + p] : (int64_t)p;
  int32_t l0 = 0, l1 = 0;
  if (list >= 0 && list < a.nlist) {
    l0 = a.list_ptr[list];
    l1 = a.list_ptr[list + 1];
  }
  const int32_t dim = a.t.dim;
  const raw_t* const X = static_cast<const raw_t*>(a.t.X);
  const float* const qv = a.queries + (int64_t)q * dim;
  for (int i = t; i < a.KP; i += kSelThreads) srun[i] = kNoKey;
  const int lc = t & (kBK - 1), lr = t / kBK;
  for (int32_t b0 = l0; b0 < l1; b0 += kSortN) {
    __syncthreads();  // v and srun of the previous batch are settled
    for (int sub = 0; sub < kSortN / kIvfRows; ++sub) {
      const int32_t r0 = b0 + sub * kIvfRows;
      if (r0 >= l1) {  // uniform: the batch's tail is empty
        if (t < kIvfRows) v[sub * kIvfRows + t] = kNoKey;
        continue;
      }
      int32_t row = -1;
      if (t < kIvfRows) {
        if (r0 + t < l1) row = a.list_rows[r0 + t];
        if (row >= a.t.num_rows) row = -1;
        rbase[t] = row >= 0 ? glx_swizzle_row(row, a.t.swizzle_rows) * a.t.stride : (int64_t)-1;
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
        if (row >= 0) {
          const float dist = a.metric == GLX_KNN_L2 ? knn_l2(acc, a.qn[q], a.xn[row]) : acc;
          key = ((uint64_t)knn_ord(__float_as_uint(dist), a.metric) << 32) | (uint32_t)row;
        }
        v[sub * kIvfRows + t] = key;
      }
    }
    knn_sort_batch(v, t);
    knn_merge_batch(srun, v, a.KP, t);
  }
  __syncthreads();
  uint64_t* const out = a.part + ((int64_t)q * a.P + slot) * a.KP;
  for (int i = t; i < a.KP; i += kSelThreads) out[i] = srun[i];
}

// run[q] = the KP smallest of run[q] and the P * KP keys of the query's slot lists; one workgroup per query
__global__ __launch_bounds__(kSelThreads) void knn_ivf_fold_kernel(uint64_t* __restrict__ run_all,
                                                                   const uint64_t* __restrict__ part, int32_t P,
                                                                   int32_t KP) {
  __shared__ uint64_t srun[kSortN];
  __shared__ uint64_t v[kSortN];
  const int q = blockIdx.x, t = threadIdx.x;
  uint64_t* const run = run_all + (int64_t)q * KP;
  const uint64_t* const mine = part + (int64_t)q * P * KP;
  for (int i = t; i < KP; i += kSelThreads) srun[i] = run[i];
  knn_fold(srun, v, KP, (int64_t)P * KP, t, [&](int64_t i) { return mine[i]; });
  for (int i = t; i < KP; i += kSelThreads) run[i] = srun[i];
}

KnnTable knn_ivf_table(const glx_features* f) {
  return KnnTable{f->X, f->stride, f->swizzle_rows, (int32_t)f->num_rows, f->dim, f->dtype};
}

int knn_ivf_search_device(const glx_knn_ivf* ix, int metric, const float* d_q, int32_t num_queries, int32_t k,
                          int32_t nprobe, int64_t* d_ids, float* d_dist, hipStream_t s) {
  const glx_features* const f = ix->f;
  const bool coarse = nprobe != ix->nlist;
  KnnArgs a;
  memset(&a, 0, sizeof(a));
  a.t = knn_ivf_table(f);
  a.k = k;
  a.KP = knn_pow2_at_least(k);
  a.metric = metric;
  // The slot lists hold qb queries x P probe slots x KP keys under the flat search's candidate budget: as many queries
  // per block as fit, at least one; a query whose nprobe * KP keys alone exceed the budget takes its slots in passes
  // of P that fold into the same running list.  "knn_query_block" may shrink the block (the bits do not depend on it).
  const int64_t budget_keys = (int64_t)(kCandBudgetBytes / sizeof(uint64_t));
  int64_t P = nprobe, qb = budget_keys / ((int64_t)nprobe * a.KP);
  if (qb < 1) {
    qb = 1;
    P = budget_keys / a.KP;
  }
  if (qb > num_queries) qb = num_queries;
  const int64_t knob_qb = glx_side_knobs().knn_query_block.load(std::memory_order_relaxed);
  if (knob_qb > 0 && knob_qb < qb) qb = knob_qb;

  // workspace (slot 2; knn_search_device leases slot 1 for the coarse step):
  // qn[num_queries] | xn[num_rows] (L2 on a view) | probe[qb, nprobe] | pdist[qb, nprobe] | run[qb, KP] | part[qb, P, KP]
  const bool view_norms = metric == GLX_KNN_L2 && !f->owns_x;
  const size_t off_xn = knn_align((size_t)num_queries * sizeof(float));
  const size_t off_probe = off_xn + (view_norms ? knn_align((size_t)a.t.num_rows * sizeof(float)) : 0);
  const size_t off_pdist = off_probe + (coarse ? knn_align((size_t)qb * nprobe * sizeof(int64_t)) : 0);
  const size_t off_run = off_pdist + (coarse ? knn_align((size_t)qb * nprobe * sizeof(float)) : 0);
  const size_t off_part = off_run + knn_align((size_t)qb * a.KP * sizeof(uint64_t));
  const size_t total = off_part + (size_t)qb * P * a.KP * sizeof(uint64_t);
  GlxScratch ws;
  int rc = ws.alloc(total, s, 2);
  if (rc != GLX_OK) return rc;
  char* const base = ws.as<char>();
  float* const qn = reinterpret_cast<float*>(base);
  int64_t* const probe = coarse ? reinterpret_cast<int64_t*>(base + off_probe) : nullptr;
  float* const pdist = coarse ? reinterpret_cast<float*>(base + off_pdist) : nullptr;
  a.run = reinterpret_cast<uint64_t*>(base + off_run);
  if (metric == GLX_KNN_L2) {
    if (view_norms) {
      float* const xn = reinterpret_cast<float*>(base + off_xn);
      if (a.t.num_rows > 0) knn_norms_kernel<<<(unsigned)((a.t.num_rows + 255) / 256), 256, 0, s>>>(a.t, xn);
      a.xn = xn;
    } else {
      rc = knn_table_norms(f, a.t, s, &a.xn);
      if (rc != GLX_OK) return rc;
    }
    const KnnTable qt{d_q, f->dim, 0, num_queries, f->dim, GLX_DTYPE_F32};
    knn_norms_kernel<<<(unsigned)((num_queries + 255) / 256), 256, 0, s>>>(qt, qn);
  }
  KnnIvfScan sc;
  memset(&sc, 0, sizeof(sc));
  sc.t = a.t;
  sc.xn = a.xn;
  sc.list_ptr = ix->list_ptr;
  sc.list_rows = ix->list_rows;
  sc.probe = probe;
  sc.part = reinterpret_cast<uint64_t*>(base + off_part);
  sc.nlist = ix->nlist;
  sc.nprobe = nprobe;
  sc.KP = a.KP;
  sc.metric = metric;
  const int64_t* const row_ids = f->knn_row_ids;
  const bool arith = f->idmap.keys == nullptr && f->idmap.step > 0;
  for (int64_t q0 = 0; q0 < num_queries; q0 += qb) {
    a.nq = (int32_t)(num_queries - q0 < qb ? num_queries - q0 : qb);
    a.queries = d_q + q0 * f->dim;
    a.qn = qn + q0;
    if (coarse) {
      rc = knn_search_device(&ix->cview, metric, a.queries, a.nq, nprobe, probe, pdist, s);
      if (rc != GLX_OK) return rc;
    }
    knn_ivf_fill_kernel<<<(unsigned)(((int64_t)a.nq * a.KP + 255) / 256), 256, 0, s>>>(a.run, (int64_t)a.nq * a.KP);
    sc.queries = a.queries;
    sc.qn = a.qn;
    for (int64_t p0 = 0; p0 < nprobe; p0 += P) {
      sc.p0 = (int32_t)p0;
      sc.P = (int32_t)(nprobe - p0 < P ? nprobe - p0 : P);
      const unsigned grid = (unsigned)((int64_t)a.nq * sc.P);
      if (a.t.dtype == GLX_DTYPE_F32) knn_ivf_scan_kernel<GLX_DTYPE_F32><<<grid, kSelThreads, 0, s>>>(sc);
      else if (a.t.dtype == GLX_DTYPE_BF16) knn_ivf_scan_kernel<GLX_DTYPE_BF16><<<grid, kSelThreads, 0, s>>>(sc);
      else knn_ivf_scan_kernel<GLX_DTYPE_F16><<<grid, kSelThreads, 0, s>>>(sc);
      knn_ivf_fold_kernel<<<(unsigned)a.nq, kSelThreads, 0, s>>>(a.run, sc.part, sc.P, a.KP);
    }
    knn_finish_kernel<<<(unsigned)(((int64_t)a.nq * k + 255) / 256), 256, 0, s>>>(
        a, row_ids, arith ? f->idmap.base : 0, arith ? f->idmap.step : 0, d_ids + q0 * k, d_dist + q0 * k);
  }
  return GLX_OK;
}

// assign[t] = the centroid of sample element t of a T-element sample, t < T: glx's L2 search with k = 1 over the
// centroid view, the rows staged as float32 queries `chunk` at a time
int knn_ivf_assign(const glx_knn_ivf* ix, int64_t T, int64_t chunk, float* stage, float* dist, int64_t* assign,
                   hipStream_t s) {
  const KnnTable t = knn_ivf_table(ix->f);
  for (int64_t t0 = 0; t0 < T; t0 += chunk) {
    const int64_t n = T - t0 < chunk ? T - t0 : chunk;
    knn_ivf_stage_kernel<<<(unsigned)((n * t.dim + 255) / 256), 256, 0, s>>>(t, t0, n, T, 0, stage);
    const int rc = knn_search_device(&ix->cview, GLX_KNN_L2, stage, (int32_t)n, 1, assign + t0, dist, s);
    if (rc != GLX_OK) return rc;
  }
  return GLX_OK;
}

// ix->cview = a float32 view of ix->centroids for knn_search_device
void knn_ivf_set_view(glx_knn_ivf* ix) {
  memset(static_cast<void*>(&ix->cview), 0, sizeof(ix->cview));
  ix->cview.device = ix->device;
  ix->cview.num_rows = ix->nlist;
  ix->cview.dim = ix->dim;
  ix->cview.stride = ix->dim;
  ix->cview.X = ix->centroids;
  ix->cview.dtype = GLX_DTYPE_F32;
  ix->cview.elem_size = 4;
}

// ix->centroids (allocated, viewed by ix->cview) = the start, then niter Lloyd iterations over the T-element sample of
// ix->f.  stage [chunk, dim], dist [chunk] and assign [>= T] are the caller's.  (The IVF-PQ build trains its codebooks
// through this too: a codebook is the centroids of a float32 table of residual sub-vectors.)
int knn_ivf_train_device(glx_knn_ivf* ix, int32_t niter, int64_t T, const float* centroids_init, int ptr_kind,
                         int64_t chunk, float* stage, float* dist, int64_t* assign, hipStream_t s) {
  const int32_t nlist = ix->nlist, dim = ix->dim;
  const KnnTable t = knn_ivf_table(ix->f);
  if (centroids_init != nullptr) {
    GLX_HIP(hipMemcpyAsync(ix->centroids, centroids_init, (size_t)nlist * dim * sizeof(float),
                           ptr_kind == GLX_PTR_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
  } else {
    knn_ivf_stage_kernel<<<(unsigned)(((int64_t)nlist * dim + 255) / 256), 256, 0, s>>>(t, 0, nlist, T, nlist,
                                                                                         ix->centroids);
  }
  for (int32_t it = 0; it < niter; ++it) {
    int rc = knn_ivf_assign(ix, T, chunk, stage, dist, assign, s);
    if (rc != GLX_OK) return rc;
    GlxScratch lease;
    GlxAggTranspose tr;
    rc = glx_agg_transpose(assign, nullptr, (int32_t)T, 1, nlist, s, &lease, &tr);
    if (rc != GLX_OK) return rc;
    knn_ivf_update_kernel<<<(unsigned)((nlist + 3) / 4), 256, 0, s>>>(t, T, tr.row_ptr, tr.pos, nlist, ix->centroids);
  }
  return GLX_OK;
}

int knn_ivf_build_device(glx_knn_ivf* ix, int32_t niter, int64_t train_rows, const float* centroids_init, int ptr_kind,
                         hipStream_t s) {
  const glx_features* const f = ix->f;
  const int64_t N = f->num_rows;
  const int32_t nlist = ix->nlist, dim = ix->dim;
  int64_t T = train_rows > 0 ? train_rows : (int64_t)256 * nlist;
  if (T < nlist) T = nlist;
  if (T > N) T = N;
  GLX_HIP(hipMalloc(&ix->centroids, (size_t)nlist * dim * sizeof(float)));
  GLX_HIP(hipMalloc(&ix->list_ptr, (size_t)(nlist + 1) * sizeof(int32_t)));
  GLX_HIP(hipMalloc(&ix->list_rows, (size_t)N * sizeof(int32_t)));
  knn_ivf_set_view(ix);
  int64_t chunk = (int64_t)(kIvfStageBytes / ((size_t)dim * sizeof(float)));
  if (chunk < 1) chunk = 1;
  if (chunk > N) chunk = N;
  GlxTemp stage, dist, assign;
  GLX_HIP(hipMalloc(&stage.p, (size_t)chunk * dim * sizeof(float)));
  GLX_HIP(hipMalloc(&dist.p, (size_t)chunk * sizeof(float)));
  GLX_HIP(hipMalloc(&assign.p, (size_t)N * sizeof(int64_t)));
  int rc = knn_ivf_train_device(ix, niter, T, centroids_init, ptr_kind, chunk, stage.as<float>(), dist.as<float>(),
                                assign.as<int64_t>(), s);
  if (rc != GLX_OK) return rc;
  rc = knn_ivf_assign(ix, N, chunk, stage.as<float>(), dist.as<float>(), assign.as<int64_t>(), s);
  if (rc != GLX_OK) return rc;
  std::vector<int32_t> ptr((size_t)nlist + 1);
  {
    GlxScratch lease;
    GlxAggTranspose tr;
    rc = glx_agg_transpose(assign.as<int64_t>(), nullptr, (int32_t)N, 1, nlist, s, &lease, &tr);
    if (rc != GLX_OK) return rc;
    GLX_HIP(hipMemcpyAsync(ix->list_ptr, tr.row_ptr, (size_t)(nlist + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    GLX_HIP(hipMemcpyAsync(ix->list_rows, tr.pos, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    GLX_HIP(hipMemcpyAsync(ptr.data(), ix->list_ptr, (size_t)(nlist + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    GLX_HIP(hipStreamSynchronize(s));
  }
  GLX_HIP(hipGetLastError());
  GLX_REQUIRE(ptr[0] == 0 && ptr[nlist] == N, "the lists hold %d of %lld rows", ptr[nlist] - ptr[0], (long long)N);
  ix->longest = 0;
  for (int32_t l = 0; l < nlist; ++l) {
    if (ptr[l + 1] - ptr[l] > ix->longest) ix->longest = ptr[l + 1] - ptr[l];
  }
  return GLX_OK;
}

}  // namespace

extern "C" int glx_knn_ivf_build(const glx_features* f, int32_t nlist, int32_t niter, int64_t train_rows,
                                 const float* centroids_init, int ptr_kind, void* stream, glx_knn_ivf** out) {
  GLX_REQUIRE(out != nullptr, "out is NULL");
  *out = nullptr;
  GLX_REQUIRE(nlist >= 1 && nlist <= kIvfMaxLists, "nlist must be in [1, %d], got %d", kIvfMaxLists, nlist);
  GLX_REQUIRE(niter >= 0, "niter must not be negative, got %d", niter);
  GLX_REQUIRE(train_rows >= 0, "train_rows must not be negative, got %lld", (long long)train_rows);
  GLX_REQUIRE(ptr_kind == GLX_PTR_HOST || ptr_kind == GLX_PTR_DEVICE, "bad ptr_kind");
  GLX_REQUIRE(f != nullptr, "features is NULL");
  GLX_REQUIRE(f->num_rows < INT32_MAX, "num_rows must be < 2^31");
  GLX_REQUIRE(nlist <= f->num_rows, "nlist %d exceeds the table's %lld rows", nlist, (long long)f->num_rows);
  GlxDeviceGuard guard(f->device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", f->device);
  const int cap_rc = knn_not_capturing(glx_stream(stream));
  if (cap_rc != GLX_OK) return cap_rc;
  glx_knn_ivf* ix = new (std::nothrow) glx_knn_ivf();
  GLX_REQUIRE(ix != nullptr, "out of host memory");
  ix->f = f;
  ix->device = f->device;
  ix->nlist = nlist;
  ix->dim = f->dim;
  ix->num_rows = f->num_rows;
  ix->longest = 0;
  ix->centroids = nullptr;
  ix->list_ptr = nullptr;
  ix->list_rows = nullptr;
  const int rc = knn_ivf_build_device(ix, niter, train_rows, centroids_init, ptr_kind, glx_stream(stream));
  if (rc != GLX_OK) {
    (void)hipStreamSynchronize(glx_stream(stream));
    glx_knn_ivf_destroy(ix);
    return rc;
  }
  *out = ix;
  return GLX_OK;
}

extern "C" void glx_knn_ivf_destroy(glx_knn_ivf* ix) {
  if (!ix) return;
  GlxDeviceGuard guard(ix->device);
  if (ix->centroids) (void)hipFree(ix->centroids);
  if (ix->list_ptr) (void)hipFree(ix->list_ptr);
  if (ix->list_rows) (void)hipFree(ix->list_rows);
  delete ix;
}

extern "C" int glx_knn_ivf_info(const glx_knn_ivf* ix, int32_t* nlist, int32_t* dim, int64_t* num_rows,
                                int64_t* longest_list, int64_t* device_bytes) {
  GLX_REQUIRE(ix != nullptr, "index is NULL");
  if (nlist) *nlist = ix->nlist;
  if (dim) *dim = ix->dim;
  if (num_rows) *num_rows = ix->num_rows;
  if (longest_list) *longest_list = ix->longest;
  if (device_bytes) {
    *device_bytes = (int64_t)ix->nlist * ix->dim * (int64_t)sizeof(float) + (int64_t)(ix->nlist + 1) * (int64_t)sizeof(int32_t) +
                    ix->num_rows * (int64_t)sizeof(int32_t);
  }
  return GLX_OK;
}

extern "C" int glx_knn_ivf_export(const glx_knn_ivf* ix, float* centroids_out, int64_t* list_ptr_out,
                                  int64_t* list_rows_out, int ptr_kind, void* stream) {
  GLX_REQUIRE(ix != nullptr, "index is NULL");
  GLX_REQUIRE(ptr_kind == GLX_PTR_HOST || ptr_kind == GLX_PTR_DEVICE, "bad ptr_kind");
  GlxDeviceGuard guard(ix->device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", ix->device);
  if (ptr_kind == GLX_PTR_DEVICE) {
    const int cap_rc = knn_not_capturing(glx_stream(stream));
    if (cap_rc != GLX_OK) return cap_rc;
  }
  GlxHostStage st(ix->device, ptr_kind, stream, GlxHostStage::ADMIT);
  float* d_c;
  int64_t* d_ptr;
  int64_t* d_rows;
  const size_t nc = (size_t)ix->nlist * ix->dim;
  st.out(&d_c, centroids_out, nc);
  st.out(&d_ptr, list_ptr_out, (size_t)ix->nlist + 1);
  st.out(&d_rows, list_rows_out, (size_t)ix->num_rows);
  int rc = st.begin();
  if (rc == GLX_OK) {
    if (d_c) {
      const hipError_t e = hipMemcpyAsync(d_c, ix->centroids, nc * sizeof(float), hipMemcpyDeviceToDevice, st.s);
      if (e != hipSuccess) {
        glx_set_error("copying the centroids failed: %s", hipGetErrorString(e));
        rc = GLX_INTERNAL;
      }
    }
    if (d_ptr) knn_ivf_widen_kernel<<<(unsigned)((ix->nlist + 1 + 255) / 256), 256, 0, st.s>>>(ix->list_ptr, ix->nlist + 1, d_ptr);
    if (d_rows) knn_ivf_widen_kernel<<<(unsigned)((ix->num_rows + 255) / 256), 256, 0, st.s>>>(ix->list_rows, ix->num_rows, d_rows);
  }
  return st.finish(rc);
}

extern "C" int glx_knn_ivf_search(const glx_knn_ivf* ix, int metric, const float* queries, int32_t num_queries, int32_t k,
                                  int32_t nprobe, int64_t* ids_out, float* dist_out, int ptr_kind, void* stream) {
  GLX_KNN_REQUIRE();
  GLX_REQUIRE(nprobe >= 1, "nprobe must be at least 1, got %d", nprobe);
  GLX_REQUIRE(ix != nullptr, "index is NULL");
  GLX_REQUIRE(nprobe <= ix->nlist, "nprobe %d exceeds the index's %d lists", nprobe, ix->nlist);
  GLX_REQUIRE(nprobe == ix->nlist || nprobe <= kIvfMaxProbe, "nprobe must be nlist (%d) or in [1, %d], got %d", ix->nlist,
              kIvfMaxProbe, nprobe);
  GLX_REQUIRE((int64_t)num_queries * nprobe < INT32_MAX, "num_queries * nprobe must be < 2^31");
  GLX_REQUIRE(num_queries == 0 || queries != nullptr, "queries is NULL");
  GLX_REQUIRE(num_queries == 0 || ids_out != nullptr, "ids_out is NULL");
  GLX_REQUIRE(num_queries == 0 || dist_out != nullptr, "dist_out is NULL");
  if (num_queries == 0) return GLX_OK;
  GlxDeviceGuard guard(ix->device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", ix->device);
  if (ptr_kind == GLX_PTR_DEVICE) {
    const int cap_rc = knn_not_capturing(glx_stream(stream));
    if (cap_rc != GLX_OK) return cap_rc;
  }
  GlxHostStage st(ix->device, ptr_kind, stream, GlxHostStage::ADMIT);
  const float* d_q;
  int64_t* d_ids;
  float* d_dist;
  st.in(&d_q, queries, (size_t)num_queries * ix->dim);
  st.out(&d_ids, ids_out, (size_t)num_queries * k);
  st.out(&d_dist, dist_out, (size_t)num_queries * k);
  int rc = st.begin();
  if (rc == GLX_OK) rc = knn_ivf_search_device(ix, metric, d_q, num_queries, k, nprobe, d_ids, d_dist, st.s);
  return st.finish(rc);
}

#endif  // GLX_KNN_IVF_H_
