// glx IVF-PQ index over a device feature table: the reference's IVFPQKnnIndex (contrib/knn/ivfpq_index.cc:25-60, made by
// contrib/knn/index_factory.cc; gpu_ivfpq_index.cc:30-60) without faiss and without a second copy of the table.  It sits
// on a glx_knn_ivf (coarse centroids and lists).  The contract's device functions, the slot plan and the pass loop come
// from glx_knn.h; the exact search (codes, coarse step, keys -> output) and the IVF build's Lloyd machinery, fill and
// fold are reached through the launchers of glx_knn.hip and glx_knn_ivf.hip.
//
// Contract (DESIGN.md 4, K-knn-ivfpq; include/glx.h "IVF-PQ index").  The index adds m codebooks [m, 256, dsub] and one
// m-byte code per row in LIST order (position p belongs to storage row list_rows[p]).  A search ranks the rows of the
// probed lists by an ADC score read from per-(query, list) look-up tables, and either returns the k best with that score
// (refine = 0) or re-scores the `refine` best from the TABLE with the flat search's chain and returns the k best of
// those: every distance returned with refine > 0 is the exact search's distance of that row.
//
// Build.  Codebook j is knn_ivf_train_device over a float32 table of the sample's residual sub-vectors j with 256
// lists; codes are glx's own L2 search with k = 1 over a view of the codebook.  No RNG, no float atomic.
//
// Search schedule.  One workgroup per (query, probe slot).  Lane c of 256 owns codeword c and builds the slot's look-up
// table in LDS (kPqPass sub-quantisers per pass: m <= 32 builds it once, m > 32 takes two passes per batch of codes);
// then one lane per list position loads the position's m code bytes and adds m table entries in ascending j with the
// running sum in a register.  Keys (image of adc, row) go through knn_sort_batch / knn_merge_batch into the slot's
// RP-entry list; knn_ivf_fold_kernel folds a query's slots.  The ip(q, centroid) term of the inner-product score is one
// sequential chain per (query, slot), computed by one lane each in a kernel of its own.  No counters, no atomics.
#include "glx_knn.h"

#pragma clang fp contract(off)

struct glx_knn_ivfpq {
  const glx_knn_ivf* ivf;  // coarse centroids and lists (not owned; outlives the index)
  int device;
  int32_t m, dsub, dim;
  int64_t num_rows;
  float* codebooks;  // [m, 256, dsub]
  float* cbt;        // [m, dsub, 256]: the codebooks column-major, what the look-up-table build reads (lane = codeword)
  float* cnorm;      // [m, 256] the chain of every codeword with itself
  uint8_t* codes;    // [num_rows, m] in list order
};

namespace {

constexpr int kPqCodewords = 256;  // 8 bits per sub-quantiser, fixed
constexpr int kPqMaxM = 64;
constexpr int kPqPass = 32;        // sub-quantisers whose look-up tables are in LDS at a time (32 KiB)
constexpr int32_t kPqMaxRefine = kSortN;
constexpr int64_t kPqDefaultTrainRows = 65536;

// row_list[list_rows[p]] = the list that holds position p; one lane per position
__global__ __launch_bounds__(256) void knn_ivfpq_row_list_kernel(const int32_t* __restrict__ list_ptr,
                                                                 const int32_t* __restrict__ list_rows, int32_t nlist,
                                                                 int32_t N, int32_t* __restrict__ row_list) {
  const int64_t p = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (p >= N) return;
  int32_t lo = 0, hi = nlist;  // the last list with list_ptr[l] <= p (empty lists share a start: the last one holds p)
  while (hi - lo > 1) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (list_ptr[mid] <= p) lo = mid;
    else hi = mid;
  }
  const int32_t row = list_rows[p];
  if (row >= 0 && row < N) row_list[row] = lo;
}

// out[i, c] = fsub_rn(x[row(i)][j * dsub + c], centroid[list(row(i))][j * dsub + c]) for i < n, c < dsub.
// by_pos == 0: row(i) = sample element t0 + i of a T-element sample; by_pos == 1: row(i) = list_rows[t0 + i].
__global__ __launch_bounds__(256) void knn_ivfpq_stage_kernel(KnnTable t, const float* __restrict__ centroids,
                                                              const int32_t* __restrict__ row_list,
                                                              const int32_t* __restrict__ list_rows, int by_pos,
                                                              int64_t t0, int64_t n, int64_t T, int32_t j, int32_t dsub,
                                                              int32_t nlist, float* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i >= n * dsub) return;
  const int64_t e = i / dsub;
  const int32_t c = j * dsub + (int32_t)(i - e * dsub);
  int64_t row = by_pos ? (int64_t)list_rows[t0 + e] : knn_ivf_sample_row(t0 + e, t.num_rows, T);
  if (row < 0 || row >= t.num_rows) row = 0;
  int32_t list = row_list[row];
  if (list < 0 || list >= nlist) list = 0;
  const float x = knn_elem(t.X, t.dtype, glx_swizzle_row(row, t.swizzle_rows) * t.stride + c);
  out[i] = x - centroids[(int64_t)list * t.dim + c];
}

// cbt[j, d, c] = codebooks[j, c, d]; cnorm[j, c] = the chain of codeword (j, c) with itself.  One lane per codeword.
__global__ __launch_bounds__(256) void knn_ivfpq_norms_kernel(const float* __restrict__ codebooks, int32_t m, int32_t dsub,
                                                              float* __restrict__ cbt, float* __restrict__ cnorm) {
  const int32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m * kPqCodewords) return;
  const int32_t j = i / kPqCodewords, c = i % kPqCodewords;
  float acc = 0.0f;
  for (int32_t d = 0; d < dsub; ++d) {
    const float x = codebooks[(int64_t)i * dsub + d];
    cbt[((int64_t)j * dsub + d) * kPqCodewords + c] = x;
    acc = __builtin_fmaf(x, x, acc);
  }
  cnorm[i] = acc;
}

__global__ __launch_bounds__(256) void knn_ivfpq_code_kernel(const int64_t* __restrict__ assign, int64_t p0, int64_t n,
                                                             int32_t j, int32_t m, uint8_t* __restrict__ codes) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i < n) codes[(p0 + i) * m + j] = (uint8_t)assign[i];
}

struct KnnPqScan {
  KnnTable t;
  const float* queries;      // [nq, dim] of this query block
  const float* centroids;    // [nlist, dim]
  const float* cbt;          // [m, dsub, 256]
  const float* cnorm;        // [m, 256]
  const uint8_t* codes;      // [num_rows, m] in list order
  const float* cip;          // [nq, P] ip(q, centroid of the slot's list) (IP)
  const int32_t* list_ptr;   // [nlist + 1]
  const int32_t* list_rows;  // [num_rows]
  const int64_t* probe;      // [nq, nprobe]; nullptr: probe slot p is list p
  uint64_t* part;            // [nq, P, RP]
  int32_t nlist, nprobe, p0, P, RP, metric, m, dsub;
};

// cip[q, slot] = the contract chain ip(q, centroid) over all dim columns; one lane per (query, probe slot)
__global__ __launch_bounds__(256) void knn_ivfpq_cip_kernel(KnnPqScan a, int32_t nq, float* __restrict__ cip) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i >= (int64_t)nq * a.P) return;
  const int32_t q = (int32_t)(i / a.P), slot = (int32_t)(i % a.P);
  int64_t list;
  float acc = 0.0f;
  if (knn_ivf_slot_list(a.probe, q, a.nprobe, a.p0 + slot, a.nlist, &list)) {
    const float* const qv = a.queries + (int64_t)q * a.t.dim;
    const float* const cv = a.centroids + list * a.t.dim;
    for (int32_t c = 0; c < a.t.dim; ++c) acc = __builtin_fmaf(qv[c], cv[c], acc);
  }
  cip[i] = acc;
}

// lut entry of sub-quantiser j and codeword c for a query (IP) or a query residual (L2): the contract's score of the
// sub-vector against the codeword.  cw walks the codeword's columns with a stride of `cs` floats.
__device__ __forceinline__ float knn_ivfpq_lut_entry(const float* qv, const float* cv, const float* cw, int64_t cs,
                                                     int32_t dsub, float xn, int metric) {
  float ip = 0.0f;
  if (metric != GLX_KNN_L2) {
    for (int32_t d = 0; d < dsub; ++d) ip = __builtin_fmaf(qv[d], cw[d * cs], ip);
    return ip;
  }
  float qn = 0.0f;
  for (int32_t d = 0; d < dsub; ++d) {
    const float r = qv[d] - cv[d];
    ip = __builtin_fmaf(r, cw[d * cs], ip);
    qn = __builtin_fmaf(r, r, qn);
  }
  return knn_l2(ip, qn, xn);
}

// The RP best keys (image of adc, row) of one list for one query.  Block b serves query b / P and slot p0 + b % P.
__global__ __launch_bounds__(kSelThreads) void knn_ivfpq_scan_kernel(KnnPqScan a) {
  __shared__ float lut[kPqPass][kPqCodewords];
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
  const int32_t m = a.m, dsub = a.dsub;
  for (int i = t; i < a.RP; i += kSelThreads) srun[i] = kNoKey;
  if (l1 > l0) {  // uniform
    const float* const qv = a.queries + (int64_t)q * a.t.dim;
    const float* const cv = a.centroids + list * a.t.dim;
    const float start = a.metric == GLX_KNN_L2 ? 0.0f : a.cip[(int64_t)q * a.P + slot];
    const int cw = t & (kPqCodewords - 1), half = t / kPqCodewords;
    for (int32_t b0 = l0; b0 < l1; b0 += kSortN) {
      float acc[kSortN / kSelThreads];
#pragma unroll
      for (int u = 0; u < kSortN / kSelThreads; ++u) acc[u] = start;
      for (int32_t j0 = 0; j0 < m; j0 += kPqPass) {
        const int32_t nj = m - j0 < kPqPass ? m - j0 : kPqPass;
        if (b0 == l0 || m > kPqPass) {  // uniform: m <= kPqPass builds the tables once per slot
          __syncthreads();              // the previous pass has read its tables
          for (int32_t jj = half; jj < nj; jj += kSelThreads / kPqCodewords) {
            const int32_t j = j0 + jj;
            lut[jj][cw] = knn_ivfpq_lut_entry(qv + j * dsub, cv + j * dsub, a.cbt + (int64_t)j * dsub * kPqCodewords + cw,
                                              kPqCodewords, dsub, a.cnorm[j * kPqCodewords + cw], a.metric);
          }
          __syncthreads();
        }
#pragma unroll
        for (int u = 0; u < kSortN / kSelThreads; ++u) {
          const int64_t p = (int64_t)b0 + u * kSelThreads + t;
          if (p < l1) {
            const uint8_t* const code = a.codes + p * m + j0;
            if ((m & 3) == 0) {
              const uint32_t* const code4 = reinterpret_cast<const uint32_t*>(code);
              for (int32_t jj = 0; jj < nj; jj += 4) {
                const uint32_t w = code4[jj >> 2];
                acc[u] = acc[u] + lut[jj][w & 255u];
                acc[u] = acc[u] + lut[jj + 1][(w >> 8) & 255u];
                acc[u] = acc[u] + lut[jj + 2][(w >> 16) & 255u];
                acc[u] = acc[u] + lut[jj + 3][w >> 24];
              }
            } else {
              for (int32_t jj = 0; jj < nj; ++jj) acc[u] = acc[u] + lut[jj][code[jj]];
            }
          }
        }
      }
      __syncthreads();  // v and srun of the previous batch are settled
#pragma unroll
      for (int u = 0; u < kSortN / kSelThreads; ++u) {
        const int64_t p = (int64_t)b0 + u * kSelThreads + t;
        uint64_t key = kNoKey;
        if (p < l1) {
          const int32_t row = a.list_rows[p];
          if (row >= 0 && row < a.t.num_rows) key = knn_key(acc[u], row, a.metric);
        }
        v[u * kSelThreads + t] = key;
      }
      knn_sort_batch(v, t);
      knn_merge_batch(srun, v, a.RP, t);
    }
  }
  __syncthreads();
  uint64_t* const out = a.part + ((int64_t)q * a.P + slot) * a.RP;
  for (int i = t; i < a.RP; i += kSelThreads) out[i] = srun[i];
}

// refine = 0: keys -> (node id, adc); one lane per output slot.  The image in a key gives back every number's bits
// except a zero's sign.  An L2 adc is a sum of clamped terms from +0.0f and never -0.0f; an inner-product adc of zero is
// recomputed from the row's codes (found by a binary search of the query's probed lists); a NaN is the quiet NaN.
__global__ __launch_bounds__(256) void knn_ivfpq_finish_kernel(KnnPqScan a, const uint64_t* __restrict__ run, int32_t nq,
                                                               int32_t k, const float* __restrict__ codebooks,
                                                               const int64_t* __restrict__ row_ids, int64_t id_base,
                                                               int64_t id_step, int64_t* __restrict__ ids_out,
                                                               float* __restrict__ dist_out) {
  const int64_t o = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (o >= (int64_t)nq * k) return;
  const int32_t q = (int32_t)(o / k), i = (int32_t)(o % k);
  const uint64_t key = run[(int64_t)q * a.RP + i];
  if (key == kNoKey) return knn_emit_absent(o, a.metric, ids_out, dist_out);
  const int32_t row = (int32_t)(uint32_t)key;
  const uint32_t ord = (uint32_t)(key >> 32);
  uint32_t bits = knn_unord(ord, a.metric);
  if (ord == 0xffffffffu) {
    bits = 0x7fc00000u;
  } else if ((bits & 0x7fffffffu) == 0 && a.metric != GLX_KNN_L2) {
    for (int32_t s = 0; s < a.nprobe; ++s) {
      int64_t list;
      if (!knn_ivf_slot_list(a.probe, q, a.nprobe, s, a.nlist, &list)) continue;
      int32_t lo = a.list_ptr[list], hi = a.list_ptr[list + 1];  // rows ascend within a list
      while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (a.list_rows[mid] < row) lo = mid + 1;
        else hi = mid;
      }
      if (lo >= a.list_ptr[list + 1] || a.list_rows[lo] != row) continue;
      const float* const qv = a.queries + (int64_t)q * a.t.dim;
      const float* const cv = a.centroids + list * a.t.dim;
      float adc = 0.0f;
      for (int32_t c = 0; c < a.t.dim; ++c) adc = __builtin_fmaf(qv[c], cv[c], adc);
      for (int32_t j = 0; j < a.m; ++j) {
        const float* const cw = codebooks + ((int64_t)j * kPqCodewords + a.codes[(int64_t)lo * a.m + j]) * a.dsub;
        adc = adc + knn_ivfpq_lut_entry(qv + j * a.dsub, cv + j * a.dsub, cw, 1, a.dsub, 0.0f, a.metric);
      }
      bits = __float_as_uint(adc);
      break;
    }
  }
  dist_out[o] = __uint_as_float(bits);
  ids_out[o] = knn_row_id(row, row_ids, id_base, id_step);
}

// refine > 0: out[q, 0 .. KP) = the KP best keys (image of the contract distance, row) among the rows of the first R
// keys of cand[q, 0 .. RP); one workgroup per query, the rows scored by knn_score_gathered.
template <int DT>
__global__ __launch_bounds__(kSelThreads) void knn_ivfpq_refine_kernel(KnnArgs a, const uint64_t* __restrict__ cand,
                                                                       int32_t RP, int32_t R, uint64_t* __restrict__ out) {
  __shared__ float Bs[kBK][kIvfLd];
  __shared__ float qs[kBK];
  __shared__ int64_t rbase[kIvfRows];
  __shared__ uint64_t v[kSortN];
  const int t = threadIdx.x;
  const int32_t q = blockIdx.x;
  const float* const qv = a.queries + (int64_t)q * a.t.dim;
  const uint64_t* const mine = cand + (int64_t)q * RP;
  for (int sub = 0; sub < kSortN / kIvfRows; ++sub) {
    const int32_t r0 = sub * kIvfRows;
    if (r0 >= R) {  // uniform: the batch's tail is empty
      if (t < kIvfRows) v[r0 + t] = kNoKey;
      continue;
    }
    auto row_of = [&](int i) {
      const uint64_t key = r0 + i < R ? mine[r0 + i] : kNoKey;
      return key != kNoKey ? (int32_t)(uint32_t)key : -1;
    };
    knn_score_gathered<DT>(a.t, qv, a.qn, q, a.xn, a.metric, row_of, Bs, qs, rbase, v + r0);
  }
  knn_sort_batch(v, t);
  for (int i = t; i < a.KP; i += kSelThreads) out[(int64_t)q * a.KP + i] = v[i];
}

}  // namespace

static int knn_ivfpq_search_device(const glx_knn_ivfpq* px, int metric, const float* d_q, int32_t num_queries, int32_t k,
                                   int32_t nprobe, int32_t refine, int64_t* d_ids, float* d_dist, hipStream_t s) {
  const glx_knn_ivf* const ix = px->ivf;
  const glx_features* const f = ix->f;
  const bool coarse = nprobe != ix->nlist;
  KnnArgs a;
  memset(&a, 0, sizeof(a));
  a.t = knn_table(f);
  a.k = k;
  a.KP = knn_pow2_at_least(k);
  a.metric = metric;
  const int32_t RP = knn_pow2_at_least(refine > k ? refine : k);
  const KnnSlotPlan plan = knn_slot_plan(nprobe, RP, num_queries);
  const bool exact_l2 = metric == GLX_KNN_L2 && refine > 0;
  KnnPqScan sc;
  memset(&sc, 0, sizeof(sc));
  // workspace slot 2: knn_search_device leases slot 1 for the coarse step
  float *qn, *xn_ws, *pdist, *cip;
  int64_t* probe;
  uint64_t* cand;
  auto layout = [&](KnnCarve c) {
    qn = c.take<float>(num_queries);
    xn_ws = c.take<float>(a.t.num_rows, exact_l2 && !f->owns_x);
    probe = c.take<int64_t>(plan.qb * nprobe, coarse);
    pdist = c.take<float>(plan.qb * nprobe, coarse);
    cip = c.take<float>(plan.qb * plan.P, metric == GLX_KNN_IP);
    cand = c.take<uint64_t>(plan.qb * RP);
    sc.part = c.take<uint64_t>(plan.qb * plan.P * RP);
    a.run = c.take<uint64_t>(plan.qb * a.KP, refine > 0);
    return c.off;
  };
  GlxScratch ws;
  int rc = ws.alloc(layout(KnnCarve{nullptr}), s, 2);
  if (rc != GLX_OK) return rc;
  layout(KnnCarve{ws.as<char>()});
  rc = knn_prepare_norms(f, exact_l2, d_q, num_queries, qn, xn_ws, s, &a.xn);
  if (rc != GLX_OK) return rc;
  sc.t = a.t;
  sc.centroids = ix->centroids;
  sc.cbt = px->cbt;
  sc.cnorm = px->cnorm;
  sc.codes = px->codes;
  sc.cip = cip;
  sc.list_ptr = ix->list_ptr;
  sc.list_rows = ix->list_rows;
  sc.probe = probe;
  sc.nlist = ix->nlist;
  sc.nprobe = nprobe;
  sc.RP = RP;
  sc.metric = metric;
  sc.m = px->m;
  sc.dsub = px->dsub;
  const bool arith = f->idmap.keys == nullptr && f->idmap.step > 0;
  int launch_rc = GLX_OK;
  rc = knn_ivf_passes(
      ix, metric, d_q, num_queries, nprobe, plan, probe, pdist, cand, sc.part, RP, s,
      [&](int64_t q0, int32_t nq, int32_t p0, int32_t P) {
        sc.queries = d_q + q0 * f->dim;
        sc.p0 = p0;
        sc.P = P;
        const int64_t slots = (int64_t)nq * P;
        if (cip) knn_ivfpq_cip_kernel<<<(unsigned)((slots + 255) / 256), 256, 0, s>>>(sc, nq, cip);
        knn_ivfpq_scan_kernel<<<(unsigned)slots, kSelThreads, 0, s>>>(sc);
      },
      [&](int64_t q0, int32_t nq) {
        if (refine == 0) {
          knn_ivfpq_finish_kernel<<<(unsigned)(((int64_t)nq * k + 255) / 256), 256, 0, s>>>(
              sc, cand, nq, k, px->codebooks, f->knn_row_ids, arith ? f->idmap.base : 0, arith ? f->idmap.step : 0,
              d_ids + q0 * k, d_dist + q0 * k);
          return;
        }
        a.nq = nq;
        a.queries = d_q + q0 * f->dim;
        a.qn = qn + q0;
        GLX_KNN_LAUNCH_DT(&launch_rc, a.t.dtype, knn_ivfpq_refine_kernel, (unsigned)nq, kSelThreads, s, a, cand, RP, refine, a.run);
        knn_finish(a, f, d_ids + q0 * k, d_dist + q0 * k, s);
      });
  return rc != GLX_OK ? rc : launch_rc;
}

static int knn_ivfpq_build_device(glx_knn_ivfpq* px, int32_t niter, int64_t train_rows, const float* codebooks_init,
                           int ptr_kind, hipStream_t s) {
  const glx_knn_ivf* const ix = px->ivf;
  const int64_t N = px->num_rows;
  const int32_t m = px->m, dsub = px->dsub;
  int64_t T = train_rows > 0 ? train_rows : kPqDefaultTrainRows;
  if (T < kPqCodewords) T = kPqCodewords;
  if (T > N) T = N;
  const size_t book = (size_t)kPqCodewords * dsub;
  GLX_HIP(hipMalloc(&px->codebooks, (size_t)m * book * sizeof(float)));
  GLX_HIP(hipMalloc(&px->cbt, (size_t)m * book * sizeof(float)));
  GLX_HIP(hipMalloc(&px->cnorm, (size_t)m * kPqCodewords * sizeof(float)));
  GLX_HIP(hipMalloc(&px->codes, (size_t)N * m));
  const KnnTable t = knn_table(ix->f);
  int64_t chunk = (int64_t)(kIvfStageBytes / ((size_t)dsub * sizeof(float)));
  if (chunk > N) chunk = N;
  if (chunk < T) chunk = T;  // the sample's residual sub-vectors are staged whole: the table a codebook is trained on
  GlxTemp row_list, resid, stage, dist, assign;
  GLX_HIP(hipMalloc(&row_list.p, (size_t)N * sizeof(int32_t)));
  GLX_HIP(hipMalloc(&resid.p, (size_t)chunk * dsub * sizeof(float)));
  GLX_HIP(hipMalloc(&stage.p, (size_t)T * dsub * sizeof(float)));
  GLX_HIP(hipMalloc(&dist.p, (size_t)chunk * sizeof(float)));
  GLX_HIP(hipMalloc(&assign.p, (size_t)chunk * sizeof(int64_t)));
  GLX_HIP(hipMemsetAsync(row_list.p, 0, (size_t)N * sizeof(int32_t), s));
  knn_ivfpq_row_list_kernel<<<(unsigned)((N + 255) / 256), 256, 0, s>>>(ix->list_ptr, ix->list_rows, ix->nlist, (int32_t)N,
                                                                        row_list.as<int32_t>());
  // a float32 table of T rows x dsub columns over `resid`: the table codebook j is trained on, as 256 centroids in place
  const glx_features rf = knn_f32_view(px->device, resid.as<float>(), T, dsub);
  const bool train = niter > 0 || codebooks_init == nullptr;
  if (!train) {
    GLX_HIP(hipMemcpyAsync(px->codebooks, codebooks_init, (size_t)m * book * sizeof(float),
                           ptr_kind == GLX_PTR_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
  }
  for (int32_t j = 0; j < m; ++j) {
    float* const codebook = px->codebooks + (size_t)j * book;
    const KnnTrainSet sub{knn_table(&rf), codebook, kPqCodewords, knn_f32_view(px->device, codebook, kPqCodewords, dsub)};
    if (train) {
      knn_ivfpq_stage_kernel<<<(unsigned)((T * dsub + 255) / 256), 256, 0, s>>>(
          t, ix->centroids, row_list.as<int32_t>(), ix->list_rows, 0, 0, T, T, j, dsub, ix->nlist, resid.as<float>());
      const int rc = knn_ivf_train_device(sub, niter, T, codebooks_init ? codebooks_init + (size_t)j * book : nullptr,
                                          ptr_kind, T, stage.as<float>(), dist.as<float>(), assign.as<int64_t>(), s);
      if (rc != GLX_OK) return rc;
    }
    for (int64_t p0 = 0; p0 < N; p0 += chunk) {
      const int64_t n = N - p0 < chunk ? N - p0 : chunk;
      knn_ivfpq_stage_kernel<<<(unsigned)((n * dsub + 255) / 256), 256, 0, s>>>(
          t, ix->centroids, row_list.as<int32_t>(), ix->list_rows, 1, p0, n, N, j, dsub, ix->nlist, resid.as<float>());
      const int rc = knn_search_device(&sub.cview, GLX_KNN_L2, resid.as<float>(), (int32_t)n, 1, assign.as<int64_t>(),
                                       dist.as<float>(), s);
      if (rc != GLX_OK) return rc;
      knn_ivfpq_code_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(assign.as<int64_t>(), p0, n, j, m, px->codes);
    }
  }
  knn_ivfpq_norms_kernel<<<(unsigned)((m * kPqCodewords + 255) / 256), 256, 0, s>>>(px->codebooks, m, dsub, px->cbt,
                                                                                    px->cnorm);
  GLX_HIP(hipStreamSynchronize(s));
  GLX_HIP(hipGetLastError());
  return GLX_OK;
}

extern "C" int glx_knn_ivfpq_build(const glx_knn_ivf* ivf, int32_t m, int32_t niter, int64_t train_rows,
                                   const float* codebooks_init, int ptr_kind, void* stream, glx_knn_ivfpq** out) {
  GLX_REQUIRE(out != nullptr, "out is NULL");
  *out = nullptr;
  GLX_REQUIRE(m >= 1 && m <= kPqMaxM, "m must be in [1, %d], got %d", kPqMaxM, m);
  GLX_REQUIRE(niter >= 0, "niter must not be negative, got %d", niter);
  GLX_REQUIRE(train_rows >= 0, "train_rows must not be negative, got %lld", (long long)train_rows);
  GLX_REQUIRE(ptr_kind == GLX_PTR_HOST || ptr_kind == GLX_PTR_DEVICE, "bad ptr_kind");
  GLX_REQUIRE(ivf != nullptr, "ivf index is NULL");
  GLX_REQUIRE(ivf->dim % m == 0, "m %d does not divide the table's dim %d", m, ivf->dim);
  GLX_REQUIRE(ivf->num_rows >= kPqCodewords, "num_rows must be at least %d, got %lld", kPqCodewords,
              (long long)ivf->num_rows);
  GlxDeviceGuard guard(ivf->device);
  GLX_KNN_CALL_BEGIN(guard, ivf->device, true, stream);
  glx_knn_ivfpq* px = new (std::nothrow) glx_knn_ivfpq();
  GLX_REQUIRE(px != nullptr, "out of host memory");
  px->ivf = ivf;
  px->device = ivf->device;
  px->m = m;
  px->dim = ivf->dim;
  px->dsub = ivf->dim / m;
  px->num_rows = ivf->num_rows;
  px->codebooks = nullptr;
  px->cbt = nullptr;
  px->cnorm = nullptr;
  px->codes = nullptr;
  const int rc = knn_ivfpq_build_device(px, niter, train_rows, codebooks_init, ptr_kind, glx_stream(stream));
  if (rc != GLX_OK) {
    (void)hipStreamSynchronize(glx_stream(stream));
    glx_knn_ivfpq_destroy(px);
    return rc;
  }
  *out = px;
  return GLX_OK;
}

extern "C" void glx_knn_ivfpq_destroy(glx_knn_ivfpq* px) {
  if (!px) return;
  GlxDeviceGuard guard(px->device);
  if (px->codebooks) (void)hipFree(px->codebooks);
  if (px->cbt) (void)hipFree(px->cbt);
  if (px->cnorm) (void)hipFree(px->cnorm);
  if (px->codes) (void)hipFree(px->codes);
  delete px;
}

extern "C" int glx_knn_ivfpq_info(const glx_knn_ivfpq* px, int32_t* m, int32_t* dsub, int64_t* num_rows,
                                  int64_t* device_bytes) {
  GLX_REQUIRE(px != nullptr, "index is NULL");
  if (m) *m = px->m;
  if (dsub) *dsub = px->dsub;
  if (num_rows) *num_rows = px->num_rows;
  if (device_bytes) {
    // codebooks (row-major and column-major) + codeword norms + codes
    *device_bytes = (int64_t)px->m * kPqCodewords * (2 * px->dsub + 1) * (int64_t)sizeof(float) + px->num_rows * px->m;
  }
  return GLX_OK;
}

extern "C" int glx_knn_ivfpq_export(const glx_knn_ivfpq* px, float* codebooks_out, uint8_t* codes_out, int ptr_kind,
                                    void* stream) {
  GLX_REQUIRE(px != nullptr, "index is NULL");
  GLX_REQUIRE(ptr_kind == GLX_PTR_HOST || ptr_kind == GLX_PTR_DEVICE, "bad ptr_kind");
  GlxDeviceGuard guard(px->device);
  GLX_KNN_CALL_BEGIN(guard, px->device, ptr_kind == GLX_PTR_DEVICE, stream);
  GlxHostStage st(px->device, ptr_kind, stream, GlxHostStage::ADMIT);
  float* d_cb;
  uint8_t* d_codes;
  const size_t ncb = (size_t)px->m * kPqCodewords * px->dsub, ncodes = (size_t)px->num_rows * px->m;
  st.out(&d_cb, codebooks_out, ncb);
  st.out(&d_codes, codes_out, ncodes);
  int rc = st.begin();
  if (rc == GLX_OK) {
    hipError_t e = hipSuccess;
    if (d_cb) e = hipMemcpyAsync(d_cb, px->codebooks, ncb * sizeof(float), hipMemcpyDeviceToDevice, st.s);
    if (e == hipSuccess && d_codes) e = hipMemcpyAsync(d_codes, px->codes, ncodes, hipMemcpyDeviceToDevice, st.s);
    if (e != hipSuccess) {
      glx_set_error("copying the index failed: %s", hipGetErrorString(e));
      rc = GLX_INTERNAL;
    }
  }
  return st.finish(rc);
}

extern "C" int glx_knn_ivfpq_search(const glx_knn_ivfpq* px, int metric, const float* queries, int32_t num_queries,
                                    int32_t k, int32_t nprobe, int32_t refine, int64_t* ids_out, float* dist_out,
                                    int ptr_kind, void* stream) {
  GLX_KNN_REQUIRE();
  GLX_REQUIRE(refine == 0 || (refine >= k && refine <= kPqMaxRefine), "refine must be 0 or in [k = %d, %d], got %d", k,
              kPqMaxRefine, refine);
  GLX_REQUIRE((int64_t)num_queries * (refine > k ? refine : k) < INT32_MAX, "num_queries * max(k, refine) must be < 2^31");
  const int rc = knn_ivf_check_nprobe(px ? px->ivf : nullptr, nprobe, num_queries);
  if (rc != GLX_OK) return rc;
  return knn_search_entry(
      px->device, px->dim, queries, num_queries, k, ids_out, dist_out, ptr_kind, stream,
      [&](const float* d_q, int64_t* d_ids, float* d_dist, hipStream_t s) {
        return knn_ivfpq_search_device(px, metric, d_q, num_queries, k, nprobe, refine, d_ids, d_dist, s);
      });
}
