// glx IVF-Flat index over a device feature table: the reference's IVFFlatKnnIndex (contrib/knn/ivfflat_index.cc:25-55,
// made by contrib/knn/index_factory.cc:32-34) without faiss and without a second copy of the table.  The contract's
// device functions come from glx_knn.h; the exact search's kernels (coarse step, norms, keys -> output) are reached
// through glx_knn.hip's launchers, and this file adds what an inverted file needs on top.  The IVF-PQ index
// (glx_knn_ivfpq.hip) reaches this file's trainer, fill and fold the same way.
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
// Search schedule.  One workgroup per (query, probe slot): 256 lanes own 256 list rows at a time and score them with
// knn_score_gathered.  The keys of 1,024 rows form one sorted batch that is merged into the slot's KP-entry list
// (knn_sort_batch / knn_merge_batch: the body of knn_fold); knn_ivf_fold_kernel then folds a query's slot lists into
// its running list and knn_finish_kernel turns keys into (id, dist).  No counters, no atomics of any kind.
#include <vector>

#include "glx_knn.h"

#pragma clang fp contract(off)

namespace {

constexpr int32_t kIvfMaxLists = 65536;
constexpr int32_t kIvfMaxProbe = 1024;  // the coarse step is a flat search with k = nprobe
constexpr int kIvfU = 4;                // rows in flight per lane of the centroid update

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
  __shared__ float Bs[kBK][kIvfLd];
  __shared__ float qs[kBK];
  __shared__ int64_t rbase[kIvfRows];
  __shared__ uint64_t srun[kSortN];
  __shared__ uint64_t v[kSortN];
  const int t = threadIdx.x;
  const int32_t q = (int32_t)(blockIdx.x / (uint32_t)a.P), slot = (int32_t)(blockIdx.x % (uint32_t)a.P);
  int64_t list;
  int32_t l0 = 0, l1 = 0;
  if (knn_ivf_slot_list(a.probe, q, a.nprobe, a.p0 + slot, a.nlist, &list)) {
    l0 = a.list_ptr[list];
    l1 = a.list_ptr[list + 1];
  }
  const float* const qv = a.queries + (int64_t)q * a.t.dim;
  for (int i = t; i < a.KP; i += kSelThreads) srun[i] = kNoKey;
  for (int32_t b0 = l0; b0 < l1; b0 += kSortN) {
    __syncthreads();  // v and srun of the previous batch are settled
    for (int sub = 0; sub < kSortN / kIvfRows; ++sub) {
      const int32_t r0 = b0 + sub * kIvfRows;
      if (r0 >= l1) {  // uniform: the batch's tail is empty
        if (t < kIvfRows) v[sub * kIvfRows + t] = kNoKey;
        continue;
      }
      knn_score_gathered<DT>(
          a.t, qv, a.qn, q, a.xn, a.metric, [&](int i) { return r0 + i < l1 ? a.list_rows[r0 + i] : -1; }, Bs, qs, rbase,
          v + sub * kIvfRows);
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

}  // namespace

void knn_ivf_fill(uint64_t* keys, int64_t n, hipStream_t s) {
  knn_ivf_fill_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(keys, n);
}

void knn_ivf_fold(uint64_t* run, const uint64_t* part, int32_t nq, int32_t P, int32_t KP, hipStream_t s) {
  knn_ivf_fold_kernel<<<(unsigned)nq, kSelThreads, 0, s>>>(run, part, P, KP);
}

static int knn_ivf_search_device(const glx_knn_ivf* ix, int metric, const float* d_q, int32_t num_queries, int32_t k,
                                 int32_t nprobe, int64_t* d_ids, float* d_dist, hipStream_t s) {
  const glx_features* const f = ix->f;
  const bool coarse = nprobe != ix->nlist;
  KnnArgs a;
  memset(&a, 0, sizeof(a));
  a.t = knn_table(f);
  a.k = k;
  a.KP = knn_pow2_at_least(k);
  a.metric = metric;
  const KnnSlotPlan plan = knn_slot_plan(nprobe, a.KP, num_queries);
  KnnIvfScan sc;
  memset(&sc, 0, sizeof(sc));
  // workspace slot 2: knn_search_device leases slot 1 for the coarse step
  float *qn, *xn_ws, *pdist;
  int64_t* probe;
  auto layout = [&](KnnCarve c) {
    qn = c.take<float>(num_queries);
    xn_ws = c.take<float>(a.t.num_rows, metric == GLX_KNN_L2 && !f->owns_x);
    probe = c.take<int64_t>(plan.qb * nprobe, coarse);
    pdist = c.take<float>(plan.qb * nprobe, coarse);
    a.run = c.take<uint64_t>(plan.qb * a.KP);
    sc.part = c.take<uint64_t>(plan.qb * plan.P * a.KP);
    return c.off;
  };
  GlxScratch ws;
  int rc = ws.alloc(layout(KnnCarve{nullptr}), s, 2);
  if (rc != GLX_OK) return rc;
  layout(KnnCarve{ws.as<char>()});
  rc = knn_prepare_norms(f, metric == GLX_KNN_L2, d_q, num_queries, qn, xn_ws, s, &a.xn);
  if (rc != GLX_OK) return rc;
  sc.t = a.t;
  sc.xn = a.xn;
  sc.list_ptr = ix->list_ptr;
  sc.list_rows = ix->list_rows;
  sc.probe = probe;
  sc.nlist = ix->nlist;
  sc.nprobe = nprobe;
  sc.KP = a.KP;
  sc.metric = metric;
  int launch_rc = GLX_OK;
  rc = knn_ivf_passes(
      ix, metric, d_q, num_queries, nprobe, plan, probe, pdist, a.run, sc.part, a.KP, s,
      [&](int64_t q0, int32_t nq, int32_t p0, int32_t P) {
        sc.queries = d_q + q0 * f->dim;
        sc.qn = qn + q0;
        sc.p0 = p0;
        sc.P = P;
        GLX_KNN_LAUNCH_DT(&launch_rc, a.t.dtype, knn_ivf_scan_kernel, (unsigned)((int64_t)nq * P), kSelThreads, s, sc);
      },
      [&](int64_t q0, int32_t nq) {
        a.nq = nq;
        a.queries = d_q + q0 * f->dim;
        a.qn = qn + q0;
        knn_finish(a, f, d_ids + q0 * k, d_dist + q0 * k, s);
      });
  return rc != GLX_OK ? rc : launch_rc;
}

// assign[t] = the centroid of sample element t of a T-element sample, t < T: glx's L2 search with k = 1 over the
// centroid view, the rows staged as float32 queries `chunk` at a time
static int knn_ivf_assign(const KnnTrainSet& ts, int64_t T, int64_t chunk, float* stage, float* dist, int64_t* assign,
                          hipStream_t s) {
  const KnnTable& t = ts.t;
  for (int64_t t0 = 0; t0 < T; t0 += chunk) {
    const int64_t n = T - t0 < chunk ? T - t0 : chunk;
    knn_ivf_stage_kernel<<<(unsigned)((n * t.dim + 255) / 256), 256, 0, s>>>(t, t0, n, T, 0, stage);
    const int rc = knn_search_device(&ts.cview, GLX_KNN_L2, stage, (int32_t)n, 1, assign + t0, dist, s);
    if (rc != GLX_OK) return rc;
  }
  return GLX_OK;
}

// (The IVF-PQ build trains its codebooks through this too: a codebook is the centroids of a float32 table of residual
// sub-vectors.)
int knn_ivf_train_device(const KnnTrainSet& ts, int32_t niter, int64_t T, const float* centroids_init, int ptr_kind,
                         int64_t chunk, float* stage, float* dist, int64_t* assign, hipStream_t s) {
  const int32_t nlist = ts.nlist, dim = ts.t.dim;
  const KnnTable& t = ts.t;
  if (centroids_init != nullptr) {
    GLX_HIP(hipMemcpyAsync(ts.centroids, centroids_init, (size_t)nlist * dim * sizeof(float),
                           ptr_kind == GLX_PTR_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
  } else {
    knn_ivf_stage_kernel<<<(unsigned)(((int64_t)nlist * dim + 255) / 256), 256, 0, s>>>(t, 0, nlist, T, nlist,
                                                                                         ts.centroids);
  }
  for (int32_t it = 0; it < niter; ++it) {
    int rc = knn_ivf_assign(ts, T, chunk, stage, dist, assign, s);
    if (rc != GLX_OK) return rc;
    GlxScratch lease;
    GlxAggTranspose tr;
    rc = glx_agg_transpose(assign, nullptr, (int32_t)T, 1, nlist, s, &lease, &tr);
    if (rc != GLX_OK) return rc;
    knn_ivf_update_kernel<<<(unsigned)((nlist + 3) / 4), 256, 0, s>>>(t, T, tr.row_ptr, tr.pos, nlist, ts.centroids);
  }
  return GLX_OK;
}

static int knn_ivf_build_device(glx_knn_ivf* ix, int32_t niter, int64_t train_rows, const float* centroids_init,
                                int ptr_kind, hipStream_t s) {
  const glx_features* const f = ix->f;
  const int64_t N = f->num_rows;
  const int32_t nlist = ix->nlist, dim = ix->dim;
  int64_t T = train_rows > 0 ? train_rows : (int64_t)256 * nlist;
  if (T < nlist) T = nlist;
  if (T > N) T = N;
  GLX_HIP(hipMalloc(&ix->centroids, (size_t)nlist * dim * sizeof(float)));
  GLX_HIP(hipMalloc(&ix->list_ptr, (size_t)(nlist + 1) * sizeof(int32_t)));
  GLX_HIP(hipMalloc(&ix->list_rows, (size_t)N * sizeof(int32_t)));
  ix->cview = knn_f32_view(ix->device, ix->centroids, nlist, dim);
  const KnnTrainSet ts{knn_table(f), ix->centroids, nlist, ix->cview};
  int64_t chunk = (int64_t)(kIvfStageBytes / ((size_t)dim * sizeof(float)));
  if (chunk < 1) chunk = 1;
  if (chunk > N) chunk = N;
  GlxTemp stage, dist, assign;
  GLX_HIP(hipMalloc(&stage.p, (size_t)chunk * dim * sizeof(float)));
  GLX_HIP(hipMalloc(&dist.p, (size_t)chunk * sizeof(float)));
  GLX_HIP(hipMalloc(&assign.p, (size_t)N * sizeof(int64_t)));
  int rc = knn_ivf_train_device(ts, niter, T, centroids_init, ptr_kind, chunk, stage.as<float>(), dist.as<float>(),
                                assign.as<int64_t>(), s);
  if (rc != GLX_OK) return rc;
  rc = knn_ivf_assign(ts, N, chunk, stage.as<float>(), dist.as<float>(), assign.as<int64_t>(), s);
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
  GLX_KNN_CALL_BEGIN(guard, f->device, true, stream);
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
  GLX_KNN_CALL_BEGIN(guard, ix->device, ptr_kind == GLX_PTR_DEVICE, stream);
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
  const int rc = knn_ivf_check_nprobe(ix, nprobe, num_queries);
  if (rc != GLX_OK) return rc;
  return knn_search_entry(ix->device, ix->dim, queries, num_queries, k, ids_out, dist_out, ptr_kind, stream,
                          [&](const float* d_q, int64_t* d_ids, float* d_dist, hipStream_t s) {
                            return knn_ivf_search_device(ix, metric, d_q, num_queries, k, nprobe, d_ids, d_dist, s);
                          });
}

int knn_ivf_check_nprobe(const glx_knn_ivf* ix, int32_t nprobe, int32_t num_queries) {
  GLX_REQUIRE(nprobe >= 1, "nprobe must be at least 1, got %d", nprobe);
  GLX_REQUIRE(ix != nullptr, "index is NULL");
  GLX_REQUIRE(nprobe <= ix->nlist, "nprobe %d exceeds the index's %d lists", nprobe, ix->nlist);
  GLX_REQUIRE(nprobe == ix->nlist || nprobe <= kIvfMaxProbe, "nprobe must be nlist (%d) or in [1, %d], got %d", ix->nlist,
              kIvfMaxProbe, nprobe);
  GLX_REQUIRE((int64_t)num_queries * nprobe < INT32_MAX, "num_queries * nprobe must be < 2^31");
  return GLX_OK;
}
