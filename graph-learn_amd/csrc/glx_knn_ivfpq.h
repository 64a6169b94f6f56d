// glx IVF-PQ index over a device feature table: the reference's IVFPQKnnIndex (contrib/knn/ivfpq_index.cc:25-60, made by
// contrib/knn/index_factory.cc; gpu_ivfpq_index.cc:30-60) without faiss and without a second copy of the table.  Included
// at the END of glx_knn.hip, after glx_knn_ivf.h: it sits on a glx_knn_ivf (coarse centroids and lists) and shares the
// contract helpers and the IVF build's Lloyd machinery.
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
#ifndef GLX_KNN_IVFPQ_H_
#define GLX_KNN_IVFPQ_H_

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

// the list a (query, probe slot) scans, -1 when the coarse step named none
__device__ __forceinline__ int64_t knn_ivfpq_slot_list(const int64_t* probe, int32_t q, int32_t nprobe, int32_t p,
                                                       int32_t nlist) {
  const int64_t list = probe ? probe[(int64_t)q * nprobe + p] : (int64_t)p;
  return list >= 0 && list < nlist ? list : (int64_t)-1;
}

// cip[q, slot] = the contract chain ip(q, centroid) over all dim columns; one lane per (query, probe slot)
__global__ __launch_bounds__(256) void knn_ivfpq_cip_kernel(KnnPqScan a, int32_t nq, float* __restrict__ cip) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i >= (int64_t)nq * a.P) return;
  const int32_t q = (int32_t)(i / a.P), slot = (int32_t)(i % a.P);
  const int64_t list = knn_ivfpq_slot_list(a.probe, q, a.nprobe, a.p0 + slot, a.nlist);
  float acc = 0.0f;
  if (list >= 0) {
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
  const int64_t list = knn_ivfpq_slot_list(a.probe, q, a.nprobe, a.p0 + slot, a.nlist);
  int32_t l0 = 0, l1 = 0;
  if (list >= 0) {
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
          if (row >= 0 && row < a.t.num_rows)
            key = ((uint64_t)knn_ord(__float_as_uint(acc[u]), a.metric) << 32) | (uint32_t)row;
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
  if (key == kNoKey) {
    ids_out[o] = -1;
    dist_out[o] = a.metric == GLX_KNN_L2 ? __builtin_inff() : -__builtin_inff();
    return;
  }
  const int32_t row = (int32_t)(uint32_t)key;
  const uint32_t ord = (uint32_t)(key >> 32);
  uint32_t bits = knn_unord(ord, a.metric);
  if (ord == 0xffffffffu) {
    bits = 0x7fc00000u;
  } else if ((bits & 0x7fffffffu) == 0 && a.metric != GLX_KNN_L2) {
    for (int32_t s = 0; s < a.nprobe; ++s) {
      const int64_t list = knn_ivfpq_slot_list(a.probe, q, a.nprobe, s, a.nlist);
      if (list < 0) continue;
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
  ids_out[o] = row_ids ? row_ids[row] : (id_step > 0 ? id_base + id_step * row : (int64_t)row);
}

// refine > 0: out[q, 0 .. KP) = the KP best keys (image of the contract distance, row) among the rows of the first R
// keys of cand[q, 0 .. RP); one workgroup per query, the rows gathered with knn_ivf_scan_kernel's tile pattern.
template <int DT>
__global__ __launch_bounds__(kSelThreads) void knn_ivfpq_refine_kernel(KnnArgs a, const uint64_t* __restrict__ cand,
                                                                       int32_t RP, int32_t R, uint64_t* __restrict__ out) {
  typedef typename AggElem<DT>::raw raw_t;
  __shared__ float Bs[kBK][kIvfLd];
  __shared__ float qs[kBK];
  __shared__ int64_t rbase[kIvfRows];
  __shared__ uint64_t v[kSortN];
  const int t = threadIdx.x;
  const int32_t q = blockIdx.x;
  const int32_t dim = a.t.dim;
  const raw_t* const X = static_cast<const raw_t*>(a.t.X);
  const float* const qv = a.queries + (int64_t)q * dim;
  const uint64_t* const mine = cand + (int64_t)q * RP;
  const int lc = t & (kBK - 1), lr = t / kBK;
  for (int sub = 0; sub < kSortN / kIvfRows; ++sub) {
    const int32_t r0 = sub * kIvfRows;
    if (r0 >= R) {  // uniform: the batch's tail is empty
      if (t < kIvfRows) v[r0 + t] = kNoKey;
      continue;
    }
    int32_t row = -1;
    if (t < kIvfRows) {
      if (r0 + t < R) {
        const uint64_t key = mine[r0 + t];
        if (key != kNoKey) row = (int32_t)(uint32_t)key;
      }
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
      v[r0 + t] = key;
    }
  }
  knn_sort_batch(v, t);
  for (int i = t; i < a.KP; i += kSelThreads) out[(int64_t)q * a.KP + i] = v[i];
}

int knn_ivfpq_search_device(const glx_knn_ivfpq* px, int metric, const float* d_q, int32_t num_queries, int32_t k,
                            int32_t nprobe, int32_t refine, int64_t* d_ids, float* d_dist, hipStream_t s) {
  const glx_knn_ivf* const ix = px->ivf;
  const glx_features* const f = ix->f;
  const bool coarse = nprobe != ix->nlist;
  KnnArgs a;
  memset(&a, 0, sizeof(a));
  a.t = knn_ivf_table(f);
  a.k = k;
  a.KP = knn_pow2_at_least(k);
  a.metric = metric;
  const int32_t RP = knn_pow2_at_least(refine > k ? refine : k);
  // as knn_ivf_search_device: qb queries x P probe slots x RP keys under the flat search's candidate budget
  const int64_t budget_keys = (int64_t)(kCandBudgetBytes / sizeof(uint64_t));
  int64_t P = nprobe, qb = budget_keys / ((int64_t)nprobe * RP);
  if (qb < 1) {
    qb = 1;
    P = budget_keys / RP;
  }
  if (qb > num_queries) qb = num_queries;
  const int64_t knob_qb = glx_side_knobs().knn_query_block.load(std::memory_order_relaxed);
  if (knob_qb > 0 && knob_qb < qb) qb = knob_qb;

  // workspace (slot 2; knn_search_device leases slot 1 for the coarse step): qn[num_queries] | xn[num_rows] (L2 refine on
  // a view) | probe[qb, nprobe] | pdist[qb, nprobe] | cip[qb, P] (IP) | cand[qb, RP] | part[qb, P, RP] | run[qb, KP]
  const bool exact_l2 = metric == GLX_KNN_L2 && refine > 0;
  const bool view_norms = exact_l2 && !f->owns_x;
  const size_t off_xn = knn_align((size_t)num_queries * sizeof(float));
  const size_t off_probe = off_xn + (view_norms ? knn_align((size_t)a.t.num_rows * sizeof(float)) : 0);
  const size_t off_pdist = off_probe + (coarse ? knn_align((size_t)qb * nprobe * sizeof(int64_t)) : 0);
  const size_t off_cip = off_pdist + (coarse ? knn_align((size_t)qb * nprobe * sizeof(float)) : 0);
  const size_t off_cand = off_cip + (metric == GLX_KNN_IP ? knn_align((size_t)qb * P * sizeof(float)) : 0);
  const size_t off_part = off_cand + knn_align((size_t)qb * RP * sizeof(uint64_t));
  const size_t off_run = off_part + knn_align((size_t)qb * P * RP * sizeof(uint64_t));
  const size_t total = off_run + (refine > 0 ? (size_t)qb * a.KP * sizeof(uint64_t) : 0);
  GlxScratch ws;
  int rc = ws.alloc(total, s, 2);
  if (rc != GLX_OK) return rc;
  char* const base = ws.as<char>();
  float* const qn = reinterpret_cast<float*>(base);
  int64_t* const probe = coarse ? reinterpret_cast<int64_t*>(base + off_probe) : nullptr;
  float* const pdist = coarse ? reinterpret_cast<float*>(base + off_pdist) : nullptr;
  float* const cip = metric == GLX_KNN_IP ? reinterpret_cast<float*>(base + off_cip) : nullptr;
  uint64_t* const cand = reinterpret_cast<uint64_t*>(base + off_cand);
  a.run = refine > 0 ? reinterpret_cast<uint64_t*>(base + off_run) : nullptr;
  if (exact_l2) {
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
  KnnPqScan sc;
  memset(&sc, 0, sizeof(sc));
  sc.t = a.t;
  sc.centroids = ix->centroids;
  sc.cbt = px->cbt;
  sc.cnorm = px->cnorm;
  sc.codes = px->codes;
  sc.cip = cip;
  sc.list_ptr = ix->list_ptr;
  sc.list_rows = ix->list_rows;
  sc.probe = probe;
  sc.part = reinterpret_cast<uint64_t*>(base + off_part);
  sc.nlist = ix->nlist;
  sc.nprobe = nprobe;
  sc.RP = RP;
  sc.metric = metric;
  sc.m = px->m;
  sc.dsub = px->dsub;
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
    knn_ivf_fill_kernel<<<(unsigned)(((int64_t)a.nq * RP + 255) / 256), 256, 0, s>>>(cand, (int64_t)a.nq * RP);
    sc.queries = a.queries;
    for (int64_t p0 = 0; p0 < nprobe; p0 += P) {
      sc.p0 = (int32_t)p0;
      sc.P = (int32_t)(nprobe - p0 < P ? nprobe - p0 : P);
      const int64_t slots = (int64_t)a.nq * sc.P;
      if (cip) knn_ivfpq_cip_kernel<<<(unsigned)((slots + 255) / 256), 256, 0, s>>>(sc, a.nq, cip);
      knn_ivfpq_scan_kernel<<<(unsigned)slots, kSelThreads, 0, s>>>(sc);
      knn_ivf_fold_kernel<<<(unsigned)a.nq, kSelThreads, 0, s>>>(cand, sc.part, sc.P, RP);
    }
    const unsigned out_grid = (unsigned)(((int64_t)a.nq * k + 255) / 256);
    const int64_t id_base = arith ? f->idmap.base : 0, id_step = arith ? f->idmap.step : 0;
    if (refine == 0) {
      knn_ivfpq_finish_kernel<<<out_grid, 256, 0, s>>>(sc, cand, a.nq, k, px->codebooks, row_ids, id_base, id_step,
                                                       d_ids + q0 * k, d_dist + q0 * k);
      continue;
    }
    if (a.t.dtype == GLX_DTYPE_F32) knn_ivfpq_refine_kernel<GLX_DTYPE_F32><<<(unsigned)a.nq, kSelThreads, 0, s>>>(a, cand, RP, refine, a.run);
    else if (a.t.dtype == GLX_DTYPE_BF16) knn_ivfpq_refine_kernel<GLX_DTYPE_BF16><<<(unsigned)a.nq, kSelThreads, 0, s>>>(a, cand, RP, refine, a.run);
    else knn_ivfpq_refine_kernel<GLX_DTYPE_F16><<<(unsigned)a.nq, kSelThreads, 0, s>>>(a, cand, RP, refine, a.run);
    knn_finish_kernel<<<out_grid, 256, 0, s>>>(a, row_ids, id_base, id_step, d_ids + q0 * k, d_dist + q0 * k);
  }
  return GLX_OK;
}

int knn_ivfpq_build_device(glx_knn_ivfpq* px, int32_t niter, int64_t train_rows, const float* codebooks_init,
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
  const KnnTable t = knn_ivf_table(ix->f);
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
  // a float32 table of T rows x dsub columns over `resid`, and an index of 256 lists over it whose centroids are
  // codebook j in place
  glx_features rf;
  memset(static_cast<void*>(&rf), 0, sizeof(rf));
  rf.device = px->device;
  rf.num_rows = T;
  rf.dim = dsub;
  rf.stride = dsub;
  rf.X = resid.p;
  rf.dtype = GLX_DTYPE_F32;
  rf.elem_size = 4;
  glx_knn_ivf sub;
  sub.f = &rf;
  sub.device = px->device;
  sub.nlist = kPqCodewords;
  sub.dim = dsub;
  sub.num_rows = T;
  sub.longest = 0;
  sub.list_ptr = nullptr;
  sub.list_rows = nullptr;
  const bool train = niter > 0 || codebooks_init == nullptr;
  if (!train) {
    GLX_HIP(hipMemcpyAsync(px->codebooks, codebooks_init, (size_t)m * book * sizeof(float),
                           ptr_kind == GLX_PTR_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
  }
  for (int32_t j = 0; j < m; ++j) {
    sub.centroids = px->codebooks + (size_t)j * book;
    knn_ivf_set_view(&sub);
    if (train) {
      knn_ivfpq_stage_kernel<<<(unsigned)((T * dsub + 255) / 256), 256, 0, s>>>(
          t, ix->centroids, row_list.as<int32_t>(), ix->list_rows, 0, 0, T, T, j, dsub, ix->nlist, resid.as<float>());
      const int rc = knn_ivf_train_device(&sub, niter, T, codebooks_init ? codebooks_init + (size_t)j * book : nullptr,
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

}  // namespace

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
  GLX_REQUIRE(guard.ok, "cannot select device %d", ivf->device);
  const int cap_rc = knn_not_capturing(glx_stream(stream));
  if (cap_rc != GLX_OK) return cap_rc;
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
  GLX_REQUIRE(guard.ok, "cannot select device %d", px->device);
  if (ptr_kind == GLX_PTR_DEVICE) {
    const int cap_rc = knn_not_capturing(glx_stream(stream));
    if (cap_rc != GLX_OK) return cap_rc;
  }
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
  GLX_REQUIRE(nprobe >= 1, "nprobe must be at least 1, got %d", nprobe);
  GLX_REQUIRE(px != nullptr, "index is NULL");
  const glx_knn_ivf* const ix = px->ivf;
  GLX_REQUIRE(nprobe <= ix->nlist, "nprobe %d exceeds the index's %d lists", nprobe, ix->nlist);
  GLX_REQUIRE(nprobe == ix->nlist || nprobe <= kIvfMaxProbe, "nprobe must be nlist (%d) or in [1, %d], got %d", ix->nlist,
              kIvfMaxProbe, nprobe);
  GLX_REQUIRE((int64_t)num_queries * nprobe < INT32_MAX, "num_queries * nprobe must be < 2^31");
  GLX_REQUIRE(num_queries == 0 || queries != nullptr, "queries is NULL");
  GLX_REQUIRE(num_queries == 0 || ids_out != nullptr, "ids_out is NULL");
  GLX_REQUIRE(num_queries == 0 || dist_out != nullptr, "dist_out is NULL");
  if (num_queries == 0) return GLX_OK;
  GlxDeviceGuard guard(px->device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", px->device);
  if (ptr_kind == GLX_PTR_DEVICE) {
    const int cap_rc = knn_not_capturing(glx_stream(stream));
    if (cap_rc != GLX_OK) return cap_rc;
  }
  GlxHostStage st(px->device, ptr_kind, stream, GlxHostStage::ADMIT);
  const float* d_q;
  int64_t* d_ids;
  float* d_dist;
  st.in(&d_q, queries, (size_t)num_queries * px->dim);
  st.out(&d_ids, ids_out, (size_t)num_queries * k);
  st.out(&d_dist, dist_out, (size_t)num_queries * k);
  int rc = st.begin();
  if (rc == GLX_OK) rc = knn_ivfpq_search_device(px, metric, d_q, num_queries, k, nprobe, refine, d_ids, d_dist, st.s);
  return st.finish(rc);
}

#endif  // GLX_KNN_IVFPQ_H_
