// glx IVF-Flat search, list-major schedule (GLX_KNN_SCHED_LIST of glx_knn_ivf_search_ex): one list tile is scored
// against ALL the queries that probe the list, on the matrix cores, instead of once per (query, list) on the VALU
// (glx_knn_ivf.hip).  The answer is the query-major schedule's in every bit: a score is the contract's one ascending
// fmaf chain (DESIGN.md 4, K-knn), which is what v_mfma_f32_32x32x2_f32 computes step by step, and "the k best" is "the
// k smallest 64-bit keys", whatever order or path the candidates arrive by.
//
// Pipeline, per block of queries (knn_slot_plan's blocks):
//   coarse  knn_search_device over the centroid view names probe[nq, nprobe] (nprobe == nlist: slot p is list p).
//   seed    every query's best list (probe rank 0) goes through the query-major knn_ivf_scan_kernel straight into
//           run[q]; thr[q] = the image of the query's k-th key, "none yet" when that list held fewer than k rows.
//   invert  the (list, query) pairs of ranks >= 1 are written query-major and sorted by list with rocprim's stable radix
//           sort: sorted by (list, query).  start[l] is the first pair of list l (a binary search per list), tile_off[l]
//           the first query tile: ceil(pairs of l / 128) tiles of up to 128 queries each (one workgroup's scan).
//   score   knn_list_score_kernel, one workgroup per (list, query tile): below.  Survivors (image <= thr[q], equality
//           passes) are compacted into cand[q, cap] through the integer counter cnt[q]; a survivor past cap is not
//           written and sets over[q].  cnt[q] is a count, so it -- and with it over[q] -- is a function of the inputs
//           alone, not of the order atomics arrive in.
//   select  one workgroup per query folds cand[q, 0 .. cnt[q]) into run[q]; a query with over[q] is left alone.
//   redo    the query-major scan over ranks >= 1 with `only = over`: workgroups of queries that did not overflow return
//           at once, an overflowed query gets its list from its slot lists exactly as under the query-major schedule.
//   finish  knn_finish.
// No float atomics; the integer atomics compact and never decide a result; nothing is read back to the host.
//
// The score kernel.  256 lanes = four waves as 2 x 2, each wave four 32x32 accumulators (64 queries x 64 rows) that
// live across the whole column loop; A = 128 queries gathered through the pair list, B = 128 table rows gathered through
// list_rows (swizzle and stride honoured, elements upcast exactly).  The workgroup walks the list's rows in tiles of 128
// and each tile's columns in k-tiles of 32, as ONE sequence of stages over two LDS buffers: the gathered global loads
// of stage s + 1 (the next k-tile, or the first k-tile of the next row tile) are issued into registers before the MFMAs
// of stage s and stored to the other buffer after them, one barrier per stage.  The queries' indices and the rows'
// storage positions are kept in LDS, the next tile's rows a tile ahead.  An odd last column is a VALU fmaf on the accumulators (knn_score_kernel says why), padded queries, rows
// and columns load as zeros and never reach a kept score, and the epilogue is the exact kernel's: one ballot and one
// counter add per (half-wave, accumulator register).
#include "glx_knn.h"
#include "glx_prims.h"

#pragma clang fp contract(off)

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kListBQ = 128;           // queries per tile
constexpr int kListBR = 128;           // list rows per tile
constexpr int kListLd = kListBQ + 1;   // LDS pitch of a k-major tile: conflict-free column reads
constexpr int kListG = kListBQ / 8;    // queries (and rows) a lane gathers per k-tile
constexpr uint32_t kListNoThr = 0xffffffffu;  // "none yet": everything passes
constexpr int kListSortSlot = 3;       // workspace slot of the radix sort's temporary

struct KnnListArgs {
  KnnTable t;
  const float* queries;      // [nq, dim] of this query block
  const float* qn;           // [nq] (L2)
  const float* xn;           // [num_rows] (L2)
  const int32_t* list_ptr;   // [nlist + 1]
  const int32_t* list_rows;  // [num_rows]
  const int32_t* pair_q;     // [pairs] the query of every (list, query) pair of ranks >= 1, sorted by (list, query)
  const int32_t* start;      // [nlist + 1] the first pair of every list; start[nlist] = the pairs that name a list
  const int32_t* tile_off;   // [nlist + 1] the first query tile of every list; tile_off[nlist] = all tiles
  const uint32_t* thr;       // [nq] image of the k-th key after the seed round, kListNoThr = none yet
  uint32_t* cnt;             // [nq] survivors
  int32_t* over;             // [nq] 1: more survivors than cap
  uint64_t* cand;            // [nq, cap]
  int32_t nlist, cap, metric;
};

// after the seed round: the threshold of every query, counters and flags cleared
__global__ __launch_bounds__(256) void knn_list_seed_kernel(const uint64_t* __restrict__ run, int32_t nq, int32_t KP,
                                                            int32_t k, uint32_t* __restrict__ thr,
                                                            uint32_t* __restrict__ cnt, int32_t* __restrict__ over) {
  const int32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const uint64_t kth = run[(int64_t)q * KP + k - 1];
  thr[q] = kth == kNoKey ? kListNoThr : (uint32_t)(kth >> 32);
  cnt[q] = 0;
  over[q] = 0;
}

// pair p = q * (nprobe - 1) + (rank - 1): key = the list of the query's probe rank (nlist: the coarse step named none,
// sorted behind every list), value = q.  Query-major, so a stable sort by key orders equal lists by query.
__global__ __launch_bounds__(256) void knn_list_pairs_kernel(const int64_t* __restrict__ probe, int32_t nq,
                                                             int32_t nprobe, int32_t nlist, uint32_t* __restrict__ key,
                                                             int32_t* __restrict__ val) {
  const int64_t p = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (p >= (int64_t)nq * (nprobe - 1)) return;
  const int32_t q = (int32_t)(p / (nprobe - 1)), rank = 1 + (int32_t)(p % (nprobe - 1));
  int64_t list;
  key[p] = knn_ivf_slot_list(probe, q, nprobe, rank, nlist, &list) ? (uint32_t)list : (uint32_t)nlist;
  val[p] = q;
}

// start[l] = the first sorted pair whose key is >= l, l <= nlist
__global__ __launch_bounds__(256) void knn_list_start_kernel(const uint32_t* __restrict__ key, int32_t pairs,
                                                             int32_t nlist, int32_t* __restrict__ start) {
  const int32_t l = blockIdx.x * 256 + threadIdx.x;
  if (l > nlist) return;
  int32_t lo = 0, hi = pairs;
  while (lo < hi) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (key[mid] < (uint32_t)l) lo = mid + 1;
    else hi = mid;
  }
  start[l] = lo;
}

// tile_off = the exclusive scan of ceil((start[l + 1] - start[l]) / 128) over the lists; one workgroup, a contiguous
// run of lists per lane
__global__ __launch_bounds__(1024) void knn_list_tiles_kernel(const int32_t* __restrict__ start, int32_t nlist,
                                                              int32_t* __restrict__ tile_off) {
  __shared__ int32_t sum[1024];
  const int t = threadIdx.x;
  const int32_t per = (nlist + 1023) / 1024;
  const int32_t a = t * per < nlist ? t * per : nlist, b = a + per < nlist ? a + per : nlist;
  int32_t mine = 0;
  for (int32_t l = a; l < b; ++l) mine += (start[l + 1] - start[l] + kListBQ - 1) / kListBQ;
  sum[t] = mine;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int32_t v = t >= off ? sum[t - off] : 0;
    __syncthreads();
    sum[t] += v;
    __syncthreads();
  }
  int32_t at = sum[t] - mine;
  for (int32_t l = a; l < b; ++l) {
    tile_off[l] = at;
    at += (start[l + 1] - start[l] + kListBQ - 1) / kListBQ;
  }
  if (t == 1023) tile_off[nlist] = sum[1023];
}

// two workgroups per CU (two waves per SIMD): 66 KB of LDS each, at most 256 registers a lane
template <int DT>
__global__ __launch_bounds__(256, 2) void knn_list_score_kernel(KnnListArgs a) {
  typedef typename AggElem<DT>::raw raw_t;
  __shared__ float As[2][kBK][kListLd];
  __shared__ float Bs[2][kBK][kListLd];
  __shared__ int32_t sq[kListBQ];
  __shared__ uint32_t sthr[kListBQ];
  __shared__ float sqn[kListBQ];
  __shared__ int32_t srow[2][kListBR];  // where the table stores the rows of this tile and the next, -1 past the list
  const int32_t b = (int32_t)blockIdx.x;
  if (b >= a.tile_off[a.nlist]) return;  // the grid is a host-side upper bound
  int32_t list = 0;
  {  // the last list whose first tile is <= b: lists without tiles share their successor's offset
    int32_t lo = 0, hi = a.nlist - 1;
    while (lo < hi) {
      const int32_t mid = lo + (hi - lo + 1) / 2;
      if (a.tile_off[mid] <= b) lo = mid;
      else hi = mid - 1;
    }
    list = lo;
  }
  const int32_t l0 = a.list_ptr[list], l1 = a.list_ptr[list + 1];
  if (l1 <= l0) return;  // probed, but empty
  const int32_t p0 = a.start[list] + (b - a.tile_off[list]) * kListBQ;
  const int32_t p1 = a.start[list + 1] < p0 + kListBQ ? a.start[list + 1] : p0 + kListBQ;

  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int wq = (w & 1) * 64, wr = (w >> 1) * 64;
  const int lc = t & 31, lr = t >> 5;
  const int32_t dim = a.t.dim, dim_even = dim & ~1;
  const int64_t stride = a.t.stride, swz = a.t.swizzle_rows;
  const raw_t* const X = static_cast<const raw_t*>(a.t.X);
  const bool l2 = a.metric == GLX_KNN_L2;

  if (t < kListBQ) {
    const int32_t q = p0 + t < p1 ? a.pair_q[p0 + t] : -1;
    sq[t] = q;
    sthr[t] = q >= 0 ? a.thr[q] : 0u;
    sqn[t] = (q >= 0 && l2) ? a.qn[q] : 0.0f;
  }
  // srow[which][i] = where the table stores list position r0 + i
  auto load_rows = [&](int32_t r0, int which) {
    if (t < kListBR) {
      int32_t row = r0 + t < l1 ? a.list_rows[r0 + t] : -1;
      if (row >= a.t.num_rows) row = -1;
      srow[which][t] = row >= 0 ? (int32_t)glx_swizzle_row(row, swz) : -1;
    }
  };
  // column k0 + lc of the lane's 16 queries and 16 rows (the same ones in every k-tile), zeros where there is none
  auto fetch = [&](int32_t k0, int which, float (&qa)[kListG], float (&xb)[kListG]) {
    const int32_t c = k0 + lc;
    const bool cok = c < dim;
#pragma unroll
    for (int j = 0; j < kListG; ++j) {
      const int32_t q = sq[lr + 8 * j], row = srow[which][lr + 8 * j];
      qa[j] = (cok && q >= 0) ? a.queries[(int64_t)q * dim + c] : 0.0f;
      xb[j] = (cok && row >= 0) ? AggElem<DT>::up(X[(int64_t)row * stride + c]) : 0.0f;
    }
  };
  auto stash = [&](int buf, const float (&qa)[kListG], const float (&xb)[kListG]) {
#pragma unroll
    for (int j = 0; j < kListG; ++j) {
      As[buf][lc][lr + 8 * j] = qa[j];
      Bs[buf][lc][lr + 8 * j] = xb[j];
    }
  };

  const int32_t nkt = (dim + kBK - 1) / kBK;
  const int32_t ntile = (l1 - l0 + kListBR - 1) / kListBR;
  float qa[kListG], xb[kListG];
  load_rows(l0, 0);
  __syncthreads();  // sq / sthr / sqn and the first tile's rows are in LDS
  fetch(0, 0, qa, xb);
  stash(0, qa, xb);
  __syncthreads();  // stage 0 is in LDS
  int buf = 0;
  const uint32_t below = (1u << l31) - 1u;
  for (int32_t tile = 0; tile < ntile; ++tile) {
    const int32_t r0 = l0 + tile * kListBR;
    const bool more = tile + 1 < ntile;
    if (more) {  // read by the fetch of this tile's last stage: a barrier away unless the tile has one stage
      load_rows(r0 + kListBR, (tile + 1) & 1);
      if (nkt == 1) __syncthreads();
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    for (int32_t kt = 0; kt < nkt; ++kt) {
      const int32_t k0 = kt * kBK;
      const bool last = kt + 1 == nkt;
      const bool ahead = !last || more;  // uniform: there is a next stage
      if (ahead) {
        if (last) fetch(0, (tile + 1) & 1, qa, xb);
        else fetch(k0 + kBK, tile & 1, qa, xb);
      }
      const int32_t left = dim_even - k0;
      const int steps = (left < kBK ? (left > 0 ? left : 0) : kBK) / 2;
      for (int s = 0; s < steps; ++s) {
        const int kk = 2 * s + half;
        const float a0 = As[buf][kk][wq + l31], a1 = As[buf][kk][wq + 32 + l31];
        const float b0 = Bs[buf][kk][wr + l31], b1 = Bs[buf][kk][wr + 32 + l31];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      }
      if ((dim & 1) && last) {
        // the odd last column: a real fmaf on the accumulator, never a zero-padded MFMA step (knn_score_kernel)
        const int kk = dim - 1 - k0;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const float x = Bs[buf][kk][wr + j * 32 + l31];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float qv = As[buf][kk][wq + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half];
              acc[i][j][r] = __builtin_fmaf(qv, x, acc[i][j][r]);
            }
          }
      }
      if (ahead) stash(buf ^ 1, qa, xb);
      __syncthreads();  // the next stage is stored; this one has been consumed
      buf ^= 1;
    }
    // ---- epilogue of the row tile: threshold filter, survivors as keys into the per-query buffers
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int32_t at = r0 + wr + j * 32 + l31;
      int32_t row = at < l1 ? a.list_rows[at] : -1;
      if (row >= a.t.num_rows) row = -1;
      const bool rok = row >= 0;
      const float xn = (l2 && rok) ? a.xn[row] : 0.0f;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int slot = wq + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          const int32_t q = sq[slot];
          const bool qok = q >= 0;
          float dist = acc[i][j][r];
          if (qok && l2) dist = knn_l2(dist, sqn[slot], xn);
          const uint32_t ord = knn_ord(__float_as_uint(dist), a.metric);
          const bool pass = qok && rok && ord <= sthr[slot];
          const uint64_t ball = __ballot(pass);
          if (ball == 0) continue;  // wave-uniform
          const uint32_t mine = (uint32_t)(ball >> (32 * half));
          uint32_t base = 0;
          if (l31 == 0 && mine != 0) base = atomicAdd(&a.cnt[q], (uint32_t)__popc(mine));
          base = __shfl(base, half * 32);
          if (pass) {
            const uint32_t pos = base + (uint32_t)__popc(mine & below);
            if (pos < (uint32_t)a.cap) a.cand[(int64_t)q * a.cap + pos] = knn_key(ord, (uint32_t)row);
            else a.over[q] = 1;  // idempotent; the query is redone from its slot lists
          }
        }
      }
    }
  }
}

// run[q] = the KP smallest of run[q] and cand[q, 0 .. cnt[q]); a query that overflowed is left to the redo
__global__ __launch_bounds__(kSelThreads) void knn_list_select_kernel(uint64_t* __restrict__ run_all,
                                                                      const uint64_t* __restrict__ cand_all,
                                                                      const uint32_t* __restrict__ cnt,
                                                                      const int32_t* __restrict__ over, int32_t cap,
                                                                      int32_t KP) {
  __shared__ uint64_t srun[kSortN];
  __shared__ uint64_t v[kSortN];
  const int q = blockIdx.x, t = threadIdx.x;
  const uint32_t n = cnt[q];
  if (n == 0 || over[q] != 0) return;
  uint64_t* const run = run_all + (int64_t)q * KP;
  const uint64_t* const cand = cand_all + (int64_t)q * cap;
  for (int i = t; i < KP; i += kSelThreads) srun[i] = run[i];
  knn_fold(srun, v, KP, (int64_t)n, t, [&](int64_t i) { return cand[i]; });
  for (int i = t; i < KP; i += kSelThreads) run[i] = srun[i];
}

}  // namespace

void knn_list_starts(const uint32_t* key, int32_t pairs, int32_t nkeys, int32_t* start, int32_t* tile_off, hipStream_t s) {
  knn_list_start_kernel<<<(unsigned)((nkeys + 1 + 255) / 256), 256, 0, s>>>(key, pairs, nkeys, start);
  knn_list_tiles_kernel<<<1, 1024, 0, s>>>(start, nkeys, tile_off);
}

int knn_ivf_search_list_device(const glx_knn_ivf* ix, int metric, const float* d_q, int32_t num_queries, int32_t k,
                               int32_t nprobe, int64_t* d_ids, float* d_dist, hipStream_t s) {
  const glx_features* const f = ix->f;
  const bool coarse = nprobe != ix->nlist;
  const bool ranks = nprobe > 1;  // there is more than the seed round
  KnnArgs a;
  memset(&a, 0, sizeof(a));
  a.t = knn_table(f);
  a.k = k;
  a.KP = knn_pow2_at_least(k);
  a.metric = metric;
  const KnnSlotPlan plan = knn_slot_plan(nprobe, a.KP, num_queries);
  // cand[q, cap]: what the candidate budget holds per query of the block, never more than the table has rows (every row
  // is in one list, so a query cannot have more survivors); "knn_list_cand_cap" may shrink it
  int64_t cap = (int64_t)(kCandBudgetBytes / sizeof(uint64_t)) / plan.qb;
  if (cap > a.t.num_rows) cap = a.t.num_rows;
  const int64_t knob_cap = glx_side_knobs().knn_list_cand_cap.load(std::memory_order_relaxed);
  if (knob_cap > 0 && knob_cap < cap) cap = knob_cap;
  if (cap < 1) cap = 1;
  const int64_t max_pairs = plan.qb * (nprobe - 1);
  // the candidates are dead once the select has run: the redo's slot lists take the same keys
  const int64_t slot_keys = plan.qb * plan.P * a.KP, cand_keys = plan.qb * cap;
  KnnIvfScan sc;
  memset(&sc, 0, sizeof(sc));
  KnnListArgs la;
  memset(&la, 0, sizeof(la));
  // workspace slot 2: knn_search_device leases slot 1 for the coarse step, the radix sort slot 3
  float *qn, *xn_ws, *pdist;
  int64_t* probe;
  uint32_t *thr, *key_in, *key_out;
  int32_t *val_in, *val_out, *start, *tile_off;
  uint64_t* keys;
  auto layout = [&](KnnCarve c) {
    qn = c.take<float>(num_queries);
    xn_ws = c.take<float>(a.t.num_rows, metric == GLX_KNN_L2 && !f->owns_x);
    probe = c.take<int64_t>(plan.qb * nprobe, coarse);
    pdist = c.take<float>(plan.qb * nprobe, coarse);
    a.run = c.take<uint64_t>(plan.qb * a.KP);
    thr = c.take<uint32_t>(plan.qb, ranks);
    la.cnt = c.take<uint32_t>(plan.qb, ranks);
    la.over = c.take<int32_t>(plan.qb, ranks);
    key_in = c.take<uint32_t>(max_pairs, ranks);
    key_out = c.take<uint32_t>(max_pairs, ranks);
    val_in = c.take<int32_t>(max_pairs, ranks);
    val_out = c.take<int32_t>(max_pairs, ranks);
    start = c.take<int32_t>((size_t)ix->nlist + 1, ranks);
    tile_off = c.take<int32_t>((size_t)ix->nlist + 1, ranks);
    keys = c.take<uint64_t>(slot_keys > cand_keys ? slot_keys : cand_keys, ranks);
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
  la.t = a.t;
  la.xn = a.xn;
  la.list_ptr = ix->list_ptr;
  la.list_rows = ix->list_rows;
  la.pair_q = val_out;
  la.start = start;
  la.tile_off = tile_off;
  la.thr = thr;
  la.cand = keys;
  la.nlist = ix->nlist;
  la.cap = (int32_t)cap;
  la.metric = metric;
  int sort_bits = 1;  // keys are lists and the value nlist
  while (((int64_t)1 << sort_bits) <= ix->nlist) ++sort_bits;
  for (int64_t q0 = 0; q0 < num_queries; q0 += plan.qb) {
    const int32_t nq = (int32_t)(num_queries - q0 < plan.qb ? num_queries - q0 : plan.qb);
    if (probe) {
      rc = knn_search_device(&ix->cview, metric, d_q + q0 * ix->dim, nq, nprobe, probe, pdist, s);
      if (rc != GLX_OK) return rc;
    }
    sc.queries = la.queries = a.queries = d_q + q0 * f->dim;
    sc.qn = la.qn = a.qn = qn + q0;
    a.nq = nq;
    // seed: one slot per query, P = 1, so the scan's slot lists ARE the running lists
    sc.only = nullptr;
    sc.part = a.run;
    sc.p0 = 0;
    sc.P = 1;
    rc = knn_ivf_scan(sc, nq, s);
    if (rc != GLX_OK) return rc;
    if (ranks) {
      const int32_t pairs = (int32_t)((int64_t)nq * (nprobe - 1));
      knn_list_seed_kernel<<<(unsigned)((nq + 255) / 256), 256, 0, s>>>(a.run, nq, a.KP, k, thr, la.cnt, la.over);
      knn_list_pairs_kernel<<<(unsigned)((pairs + 255) / 256), 256, 0, s>>>(probe, nq, nprobe, ix->nlist, key_in, val_in);
      rc = glx_prim_leased(s, kListSortSlot, "list-major search: sort the (list, query) pairs", [&](void* tmp, size_t& bytes) {
        return rocprim::radix_sort_pairs(tmp, bytes, key_in, key_out, val_in, val_out, (size_t)pairs, 0, sort_bits, s);
      });
      if (rc != GLX_OK) return rc;
      knn_list_starts(key_out, pairs, ix->nlist, start, tile_off, s);
      // sum of ceil(c_l / 128) over the lists with pairs <= pairs / 128 + the lists with pairs; surplus workgroups exit
      const int64_t grid = pairs / kListBQ + (ix->nlist < pairs ? ix->nlist : pairs);
      GLX_KNN_LAUNCH_DT(&rc, a.t.dtype, knn_list_score_kernel, (unsigned)grid, 256, s, la);
      if (rc != GLX_OK) return rc;
      knn_list_select_kernel<<<(unsigned)nq, kSelThreads, 0, s>>>(a.run, keys, la.cnt, la.over, la.cap, a.KP);
      sc.only = la.over;
      sc.part = keys;
      for (int64_t p0 = 1; p0 < nprobe; p0 += plan.P) {
        sc.p0 = (int32_t)p0;
        sc.P = (int32_t)(nprobe - p0 < plan.P ? nprobe - p0 : plan.P);
        rc = knn_ivf_scan(sc, nq, s);
        if (rc != GLX_OK) return rc;
        knn_ivf_fold(a.run, keys, nq, sc.P, a.KP, s, la.over);
      }
    }
    knn_finish(a, f, d_ids + q0 * k, d_dist + q0 * k, s);
  }
  return GLX_OK;
}
