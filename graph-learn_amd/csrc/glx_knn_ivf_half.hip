// glx IVF-Flat search, half-precision list-major scan (GLX_KNN_PREC_HALF of glx_knn_ivf_search_prec): the list-major
// schedule of glx_knn_ivf_list.hip meets the half-precision scan of glx_knn_half.hip.  One list tile is scored against
// all the queries that probe the list on the 16-bit matrix cores, v_mfma_f32_32x32x16_bf16 / _f16, from the table's words
// as they lie in HBM: a bfloat16 / float16 row is never widened, a float8 row is widened to bfloat16 in registers.
//
// Contract (DESIGN.md 4, K-knn-ivf-half; include/glx.h).  The probe sets are glx_knn_ivf_search's (the float32 coarse
// step over the float32 queries as given).  The score of a (query, row) is K-knn-half's word for word: q^ = the query
// rounded once to the scan type, ip = +0.0f and then one 32x32x16 step per block of 16 columns, ascending, zero from dim
// on, L2 = knn_l2(ip, qn, xn).  The steps of a pair do not depend on the tile, list or round that scored it, so neither
// do its bits: nprobe == nlist returns what glx_knn_search_ex HALF returns, bit for bit.
//
// Schedule, per block of queries.  No seed kernel, no overflow flag, no redo: a half score cannot be redone on the VALU
// (a 32x32x16 step is not an fmaf chain), so the candidate buffer must not overflow -- and by construction cannot.
//   coarse  knn_search_device over the centroid view names probe[nq, nprobe] (nprobe == nlist: slot p is list p).
//   round   knn_round_queries writes q^ as [nq, dim rounded up to 8] 16-bit words; knn_prepare_norms as the flat scan.
//   groups  the probe ranks are cut into groups: group 0 is rank 0, group g >= 1 is ranks [1 + (g - 1) R, 1 + g R) with
//           R = max(1, cap / longest list).  A query meets at most R * longest <= cap rows in a group.
//   invert  ONE stable radix sort of the (group * (nlist + 1) + list, query) pairs of all ranks; start[] and tile_off[]
//           over groups * (nlist + 1) keys ("no list" sorts last within its group and is never scored).
//   score   per group, in order: knn_list_score_half_kernel over the group's (list, query tile) range compacts the
//           scores not worse than thr[q] (equality passes) into cand[q, cap] through the integer counter cnt[q];
//   select  knn_select folds cand[q, 0 .. cnt[q]) into run[q], refreshes thr[q] (the image of the k-th key -- of the
//           refine-th under refine; "none yet" while fewer are held) and clears cnt[q].  Group 0 runs with thr = none.
//   finish  knn_half_finish, or knn_refine + knn_finish under refine, as knn_search_half_device does it.
// No float atomics; the integer atomics compact and never decide a result (the k smallest keys of a set do not depend
// on the order they arrive in); nothing is read back to the host.
//
// The score kernel.  256 lanes = four waves as 2 x 2, each wave four 32x32 float32 accumulators (64 queries x 64 rows)
// across the whole column loop: the float32 list kernel's shape.  Operands and LDS are the flat half kernel's: a stage
// is 64 columns, tiles are 128 rows x 64 16-bit words, row-major at the 144-byte pitch whose bank argument
// glx_knn_half.hip derives, two buffers of (A, B) = 73,728 bytes, one 16-byte LDS read per operand and step.  The gather
// is new: A rows are q^ rows reached through the sorted pair list, one aligned 16-byte load per group of eight columns;
// B rows are table rows reached through list_rows (swizzle and stride honoured) by the row fronts of glx_knn.h --
// 16-byte groups of a 16-bit table, 8-byte groups of a float8 table widened with v_cvt_pk_f32_fp8 / _bf8 + v_perm_b32
// on the way into LDS, element loads for an unaligned view and for the tail group; no load touches a byte outside
// [row, row + dim).  A lane keeps its four queries (pointers in registers) and four rows (storage positions in LDS,
// srow[2][128], the next tile's loaded a tile ahead) across all column stages of a row tile.  Column stages and row
// tiles form ONE sequence of stages over the two buffers: the next stage's global loads are issued into registers
// before the current stage's MFMA steps and stored to the other buffer after them, one barrier per stage.  Padded
// queries, rows and columns are zero operands whose outputs never reach a kept key; the 16-bit step pads to 16
// columns by contract, so there is no odd-column VALU step.  The epilogue is the float32 list kernel's: per accumulator
// register the image, one ballot, one counter add per half-wave, survivors as keys into cand[q, cap].
#include "glx_knn.h"
#include "glx_prims.h"

#pragma clang fp contract(off)

namespace {

constexpr int kLhBQ = 128;                 // queries per tile
constexpr int kLhBR = 128;                 // list rows per tile
constexpr int kLhBK = 64;                  // columns per stage
constexpr int kLhGroups = kLhBK / 8;       // 16-byte groups per tile row
constexpr int kLhLd = kLhGroups + 1;       // LDS pitch in 16-byte units: 144 bytes
constexpr int kLhLoads = kLhBR * kLhGroups / 256;  // groups a lane moves per tile and stage
constexpr int kLhRowStep = 256 / kLhGroups;        // tile rows between a lane's groups
constexpr int kLhSortSlot = 3;             // workspace slot of the radix sort's temporary
constexpr int64_t kLhBlock = 8192;         // queries per block unless "knn_query_block" or the longest list shrink it
constexpr int64_t kLhMaxKeys = (int64_t)1 << 24;  // groups * (nlist + 1): start[] and tile_off[] stay under 128 MiB

struct KnnListHalfArgs {
  KnnTable t;
  const uint16_t* qh;        // [nq, qld] q^ of this query block
  const float* qn;           // [nq] (L2) the norms of q^
  const float* xn;           // [num_rows] (L2)
  const int32_t* list_ptr;   // [nlist + 1]
  const int32_t* list_rows;  // [num_rows]
  const int32_t* pair_q;     // [pairs] the query of every pair, sorted by (group, list, query)
  const int32_t* start;      // [keys + 1] the first pair of every key = group * (nlist + 1) + list
  const int32_t* tile_off;   // [keys + 1] the first query tile of every key
  const uint32_t* thr;       // [nq] image of the k-th key the earlier groups left, kNoThr = none yet
  uint32_t* cnt;             // [nq] survivors of this group
  uint64_t* cand;            // [nq, cap]
  int32_t qld, nlist, cap, metric;
  int32_t kbase;             // the group's first key
};

// pair p = q * nprobe + rank: key = group(rank) * (nlist + 1) + the list of the query's probe rank (nlist: the coarse
// step named none, sorted behind every list of the group), value = q.  Query-major, so a stable sort by key orders
// equal keys by query.
__global__ __launch_bounds__(256) void knn_list_half_pairs_kernel(const int64_t* __restrict__ probe, int32_t nq,
                                                                  int32_t nprobe, int32_t nlist, int32_t R,
                                                                  uint32_t* __restrict__ key, int32_t* __restrict__ val) {
  const int64_t p = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (p >= (int64_t)nq * nprobe) return;
  const int32_t q = (int32_t)(p / nprobe), rank = (int32_t)(p % nprobe);
  const uint32_t group = rank == 0 ? 0u : 1u + (uint32_t)((rank - 1) / R);
  int64_t list;
  if (!knn_ivf_slot_list(probe, q, nprobe, rank, nlist, &list)) list = nlist;
  key[p] = group * (uint32_t)(nlist + 1) + (uint32_t)list;
  val[p] = q;
}

// two workgroups per CU (two waves per SIMD): 76,288 bytes of LDS each, at most 256 registers a lane
template <int DT>
__global__ __launch_bounds__(256, 2) void knn_list_score_half_kernel(KnnListHalfArgs a) {
  typedef typename HalfRow<DT>::elem elem_t;
  typedef typename HalfRow<DT>::group group_t;
  __shared__ uint4 As[2][kLhBQ][kLhLd];
  __shared__ uint4 Bs[2][kLhBR][kLhLd];
  __shared__ int32_t sq[kLhBQ];
  __shared__ uint32_t sthr[kLhBQ];
  __shared__ float sqn[kLhBQ];
  __shared__ int32_t srow[2][kLhBR];  // where the table stores the rows of this tile and the next, -1 past the list
  const int32_t* const toff = a.tile_off + a.kbase;
  const int32_t b = toff[0] + (int32_t)blockIdx.x;
  if (b >= toff[a.nlist]) return;  // the grid is a host-side upper bound; the "no list" key's tiles are not scored
  int32_t list = 0;
  {  // the last list of the group whose first tile is <= b: lists without tiles share their successor's offset
    int32_t lo = 0, hi = a.nlist - 1;
    while (lo < hi) {
      const int32_t mid = lo + (hi - lo + 1) / 2;
      if (toff[mid] <= b) lo = mid;
      else hi = mid - 1;
    }
    list = lo;
  }
  const int32_t l0 = a.list_ptr[list], l1 = a.list_ptr[list + 1];
  if (l1 <= l0) return;  // probed, but empty
  const int32_t p0 = a.start[a.kbase + list] + (b - toff[list]) * kLhBQ;
  const int32_t pend = a.start[a.kbase + list + 1];
  const int32_t p1 = pend < p0 + kLhBQ ? pend : p0 + kLhBQ;

  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int wq = (w & 1) * 64, wr = (w >> 1) * 64;
  const int g = t & (kLhGroups - 1), lr = t / kLhGroups;  // the lane's group, and its first tile row
  const int32_t dim = a.t.dim, qld = a.qld;
  const int64_t stride = a.t.stride, swz = a.t.swizzle_rows;
  const elem_t* const X = static_cast<const elem_t*>(a.t.X);
  const bool vec = (reinterpret_cast<uintptr_t>(X) & (sizeof(group_t) - 1)) == 0 && (stride & 7) == 0;
  const bool l2 = a.metric == GLX_KNN_L2;

  if (t < kLhBQ) {
    const int32_t q = p0 + t < p1 ? a.pair_q[p0 + t] : -1;
    sq[t] = q;
    sthr[t] = q >= 0 ? a.thr[q] : 0u;
    sqn[t] = (q >= 0 && l2) ? a.qn[q] : 0.0f;
  }
  // the lane's queries are the same in every stage of every row tile
  const uint16_t* qp[kLhLoads];
#pragma unroll
  for (int j = 0; j < kLhLoads; ++j) {
    const int32_t at = p0 + lr + kLhRowStep * j;
    qp[j] = at < p1 ? a.qh + (int64_t)a.pair_q[at] * qld : nullptr;
  }
  // srow[which][i] = where the table stores list position r0 + i
  auto load_rows = [&](int32_t r0, int which) {
    if (t < kLhBR) {
      int32_t row = r0 + t < l1 ? a.list_rows[r0 + t] : -1;
      if (row >= a.t.num_rows) row = -1;
      srow[which][t] = row >= 0 ? (int32_t)glx_swizzle_row(row, swz) : -1;
    }
  };
  // columns [k0 + 8 g, + 8) of the lane's four queries and four rows, zeros where there is none
  auto fetch = [&](int32_t k0, int which, uint4 (&qa)[kLhLoads], group_t (&xb)[kLhLoads]) {
    const int32_t c0 = k0 + 8 * g;
#pragma unroll
    for (int j = 0; j < kLhLoads; ++j) {
      const int32_t row = srow[which][lr + kLhRowStep * j];
      qa[j] = (qp[j] && c0 < qld) ? *reinterpret_cast<const uint4*>(qp[j] + c0) : make_uint4(0u, 0u, 0u, 0u);
      xb[j] = (row >= 0 && c0 < dim) ? knn_half_group<group_t>(X + (int64_t)row * stride, c0, dim, vec) : group_t{};
    }
  };
  auto stash = [&](int buf, const uint4 (&qa)[kLhLoads], const group_t (&xb)[kLhLoads]) {
#pragma unroll
    for (int j = 0; j < kLhLoads; ++j) {
      As[buf][lr + kLhRowStep * j][g] = qa[j];
      Bs[buf][lr + kLhRowStep * j][g] = HalfRow<DT>::words(xb[j]);
    }
  };

  const int32_t nkt = (dim + kLhBK - 1) / kLhBK;
  const int32_t ntile = (l1 - l0 + kLhBR - 1) / kLhBR;
  uint4 qa[kLhLoads];
  group_t xb[kLhLoads];
  load_rows(l0, 0);
  __syncthreads();  // sq / sthr / sqn and the first tile's rows are in LDS
  fetch(0, 0, qa, xb);
  stash(0, qa, xb);
  __syncthreads();  // stage 0 is in LDS
  int buf = 0;
  const uint32_t below = (1u << l31) - 1u;
  for (int32_t tile = 0; tile < ntile; ++tile) {
    const int32_t r0 = l0 + tile * kLhBR;
    const bool more = tile + 1 < ntile;
    if (more) {  // read by the fetch of this tile's last stage: a barrier away unless the tile has one stage
      load_rows(r0 + kLhBR, (tile + 1) & 1);
      if (nkt == 1) __syncthreads();
    }
    knn_f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    for (int32_t kt = 0; kt < nkt; ++kt) {
      const int32_t k0 = kt * kLhBK;
      const bool last = kt + 1 == nkt;
      const bool ahead = !last || more;  // uniform: there is a next stage
      if (ahead) {
        if (last) fetch(0, (tile + 1) & 1, qa, xb);
        else fetch(k0 + kLhBK, tile & 1, qa, xb);
      }
      const int32_t left = dim - k0;
      const int steps = left < kLhBK ? (left + 15) / 16 : kLhBK / 16;  // one step per block of 16 columns, no more
      for (int s = 0; s < steps; ++s) {
        const uint4 a0 = As[buf][wq + l31][2 * s + half], a1 = As[buf][wq + 32 + l31][2 * s + half];
        const uint4 b0 = Bs[buf][wr + l31][2 * s + half], b1 = Bs[buf][wr + 32 + l31][2 * s + half];
        acc[0][0] = knn_half_mfma<HalfRow<DT>::kScan>(a0, b0, acc[0][0]);
        acc[0][1] = knn_half_mfma<HalfRow<DT>::kScan>(a0, b1, acc[0][1]);
        acc[1][0] = knn_half_mfma<HalfRow<DT>::kScan>(a1, b0, acc[1][0]);
        acc[1][1] = knn_half_mfma<HalfRow<DT>::kScan>(a1, b1, acc[1][1]);
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
            // a query meets at most R * longest <= cap rows in a group, so pos < cap always; the test only keeps a
            // broken plan from writing out of bounds and is no result path
            const uint32_t pos = base + (uint32_t)__popc(mine & below);
            if (pos < (uint32_t)a.cap) a.cand[(int64_t)q * a.cap + pos] = knn_key(ord, (uint32_t)row);
          }
        }
      }
    }
  }
}

void knn_list_score_half(const KnnListHalfArgs& la, unsigned grid, hipStream_t s) {
  switch (la.t.dtype) {
    case GLX_DTYPE_BF16: knn_list_score_half_kernel<GLX_DTYPE_BF16><<<grid, 256, 0, s>>>(la); break;
    case GLX_DTYPE_F16: knn_list_score_half_kernel<GLX_DTYPE_F16><<<grid, 256, 0, s>>>(la); break;
    case GLX_DTYPE_F8E4M3: knn_list_score_half_kernel<GLX_DTYPE_F8E4M3><<<grid, 256, 0, s>>>(la); break;
    default: knn_list_score_half_kernel<GLX_DTYPE_F8E5M2><<<grid, 256, 0, s>>>(la); break;
  }
}

// The query block, the candidate capacity per query and the probe-rank groups.  cand[q, cap] holds what the candidate
// budget gives a query of the block, never more than the table has rows; a block whose cap would be below the longest
// list shrinks until it is not.  "knn_query_block" may shrink the block and "knn_list_cand_cap" the capacity, the latter
// never below the longest list; no bit depends on either.
struct KnnIvfHalfPlan {
  int64_t qb, cap, R;
  int32_t groups;
};
int knn_ivf_half_plan(const glx_knn_ivf* ix, int32_t nprobe, int32_t num_queries, KnnIvfHalfPlan* out) {
  const int64_t budget = (int64_t)(kCandBudgetBytes / sizeof(uint64_t));
  const int64_t longest = ix->longest > 0 ? ix->longest : 1;
  GLX_REQUIRE(longest <= budget,
              "precision GLX_KNN_PREC_HALF: the longest list (%lld rows) exceeds the %lld keys one query's candidate "
              "buffer holds under the 256 MiB budget",
              (long long)longest, (long long)budget);
  const GlxSideKnobs& knobs = glx_side_knobs();
  const int64_t knob_qb = knobs.knn_query_block.load(std::memory_order_relaxed);
  const int64_t knob_cap = knobs.knn_list_cand_cap.load(std::memory_order_relaxed);
  KnnIvfHalfPlan p;
  p.qb = num_queries < kLhBlock ? (num_queries > 0 ? num_queries : 1) : kLhBlock;
  if (knob_qb > 0 && knob_qb < p.qb) p.qb = knob_qb;
  if (budget / p.qb < longest) p.qb = budget / longest;
  int64_t keys;
  for (;;) {
    p.cap = budget / p.qb;
    if (p.cap > ix->num_rows) p.cap = ix->num_rows;
    if (knob_cap > 0 && knob_cap < p.cap) p.cap = knob_cap;
    if (p.cap < longest) p.cap = longest;
    p.R = p.cap / longest;
    const int64_t groups = nprobe > 1 ? 1 + (nprobe - 1 + p.R - 1) / p.R : 1;
    p.groups = (int32_t)groups;
    keys = groups * ((int64_t)ix->nlist + 1);
    if (keys <= kLhMaxKeys || p.qb == 1) break;
    p.qb = (p.qb + 1) / 2;  // a larger cap per query: more ranks per group, fewer groups
  }
  GLX_REQUIRE(keys <= kLhMaxKeys,
              "precision GLX_KNN_PREC_HALF: %d probe-rank groups x (nlist + 1 = %d) keys exceed the limit of %lld",
              p.groups, ix->nlist + 1, (long long)kLhMaxKeys);
  *out = p;
  return GLX_OK;
}

// the search on device pointers (workspace slots 2 and 3; the coarse step leases slot 1)
int knn_ivf_search_half_device(const glx_knn_ivf* ix, const KnnIvfHalfPlan& plan, int metric, const float* d_q,
                               int32_t num_queries, int32_t k, int32_t nprobe, int32_t refine, int64_t* d_ids,
                               float* d_dist, hipStream_t s) {
  const glx_features* const f = ix->f;
  const bool coarse = nprobe != ix->nlist;
  const bool l2 = metric == GLX_KNN_L2;
  KnnArgs a;  // the scan: the refine best (k without refine) by the half score
  memset(&a, 0, sizeof(a));
  a.t = knn_table(f);
  a.k = refine > 0 ? refine : k;
  a.KP = knn_pow2_at_least(a.k);
  a.metric = metric;
  a.cap = (int32_t)plan.cap;
  KnnArgs x = a;  // the re-rank: the k best of those by the exact search's chain
  x.k = k;
  x.KP = knn_pow2_at_least(k);
  const int32_t qld = (a.t.dim + 7) & ~7;
  const int32_t nkey1 = ix->nlist + 1, keys = plan.groups * nkey1;
  const int64_t max_pairs = plan.qb * nprobe;

  uint16_t* qh;
  float *qn_half, *qn_exact, *xn_ws, *pdist;
  int64_t* probe;
  uint32_t *key_in, *key_out;
  int32_t *val_in, *val_out, *start, *tile_off;
  auto layout = [&](KnnCarve c) {
    qh = c.take<uint16_t>((size_t)num_queries * qld);
    qn_half = c.take<float>(num_queries);
    qn_exact = c.take<float>(num_queries, l2 && refine > 0);
    xn_ws = c.take<float>(a.t.num_rows, l2 && !f->owns_x);
    probe = c.take<int64_t>(plan.qb * nprobe, coarse);
    pdist = c.take<float>(plan.qb * nprobe, coarse);
    a.thr = c.take<uint32_t>(plan.qb);
    a.cnt = c.take<uint32_t>(plan.qb);
    a.run = c.take<uint64_t>(plan.qb * a.KP);
    a.cand = c.take<uint64_t>(plan.qb * plan.cap);
    x.run = c.take<uint64_t>(plan.qb * x.KP, refine > 0);
    key_in = c.take<uint32_t>(max_pairs);
    key_out = c.take<uint32_t>(max_pairs);
    val_in = c.take<int32_t>(max_pairs);
    val_out = c.take<int32_t>(max_pairs);
    start = c.take<int32_t>((size_t)keys + 1);
    tile_off = c.take<int32_t>((size_t)keys + 1);
    return c.off;
  };
  GlxScratch ws;
  int rc = ws.alloc(layout(KnnCarve{nullptr}), s, 2);
  if (rc != GLX_OK) return rc;
  layout(KnnCarve{ws.as<char>()});
  const int scan = a.t.dtype == GLX_DTYPE_F16 ? GLX_DTYPE_F16 : GLX_DTYPE_BF16;  // a float8 table scans as bfloat16
  knn_round_queries(d_q, num_queries, a.t.dim, qld, scan, qh, s);
  rc = knn_prepare_norms(f, l2, qh, num_queries, qn_half, xn_ws, s, &a.xn, scan, qld);
  if (rc != GLX_OK) return rc;
  x.xn = a.xn;
  if (qn_exact) knn_norms(KnnTable{d_q, a.t.dim, 0, num_queries, a.t.dim, GLX_DTYPE_F32}, qn_exact, s);

  KnnListHalfArgs la;
  memset(&la, 0, sizeof(la));
  la.t = a.t;
  la.xn = a.xn;
  la.list_ptr = ix->list_ptr;
  la.list_rows = ix->list_rows;
  la.pair_q = val_out;
  la.start = start;
  la.tile_off = tile_off;
  la.thr = a.thr;
  la.cnt = a.cnt;
  la.cand = a.cand;
  la.qld = qld;
  la.nlist = ix->nlist;
  la.cap = a.cap;
  la.metric = metric;
  int sort_bits = 1;  // the largest key is keys - 1
  while (((int64_t)1 << sort_bits) < keys) ++sort_bits;
  for (int64_t q0 = 0; q0 < num_queries; q0 += plan.qb) {
    const int32_t nq = (int32_t)(num_queries - q0 < plan.qb ? num_queries - q0 : plan.qb);
    if (probe) {
      rc = knn_search_device(&ix->cview, metric, d_q + q0 * ix->dim, nq, nprobe, probe, pdist, s);
      if (rc != GLX_OK) return rc;
    }
    a.nq = x.nq = nq;
    a.queries = x.queries = d_q + q0 * f->dim;
    a.qn = la.qn = qn_half + q0;
    la.qh = qh + q0 * qld;
    knn_init(a, s);
    const int32_t pairs = (int32_t)((int64_t)nq * nprobe);
    knn_list_half_pairs_kernel<<<(unsigned)((pairs + 255) / 256), 256, 0, s>>>(probe, nq, nprobe, ix->nlist,
                                                                               (int32_t)plan.R, key_in, val_in);
    rc = glx_prim_leased(s, kLhSortSlot, "half list-major search: sort the (group, list, query) pairs",
                         [&](void* tmp, size_t& bytes) {
                           return rocprim::radix_sort_pairs(tmp, bytes, key_in, key_out, val_in, val_out, (size_t)pairs,
                                                            0, sort_bits, s);
                         });
    if (rc != GLX_OK) return rc;
    knn_list_starts(key_out, pairs, keys, start, tile_off, s);
    for (int32_t g = 0; g < plan.groups; ++g) {
      const int64_t rank0 = g == 0 ? 0 : 1 + (g - 1) * plan.R;
      const int64_t rank1 = g == 0 ? 1 : (rank0 + plan.R < nprobe ? rank0 + plan.R : nprobe);
      // sum of ceil(c_l / 128) over the group's lists <= its pairs / 128 + its lists with pairs; surplus workgroups exit
      const int64_t gp = (int64_t)nq * (rank1 - rank0);
      const int64_t grid = gp / kLhBQ + (ix->nlist < gp ? ix->nlist : gp);
      la.kbase = g * nkey1;
      knn_list_score_half(la, (unsigned)grid, s);
      knn_select(a, s);
    }
    if (refine == 0) {
      knn_half_finish(a, f, d_ids + q0 * k, d_dist + q0 * k, s);
    } else {
      x.qn = qn_exact ? qn_exact + q0 : nullptr;
      rc = knn_refine(x, a.run, a.KP, refine, s);
      if (rc != GLX_OK) return rc;
      knn_finish(x, f, d_ids + q0 * k, d_dist + q0 * k, s);
    }
  }
  return GLX_OK;
}

}  // namespace

extern "C" int glx_knn_ivf_search_prec(const glx_knn_ivf* ix, int metric, const float* queries, int32_t num_queries,
                                       int32_t k, int32_t nprobe, int schedule, int precision, int32_t refine,
                                       int64_t* ids_out, float* dist_out, int ptr_kind, void* stream) {
  GLX_REQUIRE(precision == GLX_KNN_PREC_F32 || precision == GLX_KNN_PREC_HALF,
              "precision must be GLX_KNN_PREC_F32 (0) or GLX_KNN_PREC_HALF (1), got %d", precision);
  if (precision == GLX_KNN_PREC_F32) {
    GLX_REQUIRE(refine == 0, "refine must be 0 with precision GLX_KNN_PREC_F32, got %d", refine);
    return glx_knn_ivf_search_ex(ix, metric, queries, num_queries, k, nprobe, schedule, ids_out, dist_out, ptr_kind,
                                 stream);
  }
  GLX_KNN_REQUIRE();
  int rc = knn_ivf_check_nprobe(ix, nprobe, num_queries);
  if (rc != GLX_OK) return rc;
  GLX_REQUIRE(schedule == GLX_KNN_SCHED_LIST,
              "precision GLX_KNN_PREC_HALF needs schedule GLX_KNN_SCHED_LIST (1), got schedule %d", schedule);
  const glx_features* const f = ix->f;
  GLX_REQUIRE(f->dtype == GLX_DTYPE_BF16 || f->dtype == GLX_DTYPE_F16 || glx_dtype_is_f8(f->dtype),
              "precision GLX_KNN_PREC_HALF needs a bfloat16, float16 or float8 table, this one stores %s",
              glx_dtype_name(f->dtype));
  GLX_REQUIRE(refine == 0 || (refine >= k && refine <= kSortN), "refine must be 0 or in [k = %d, %d], got %d", k, kSortN,
              refine);
  GLX_REQUIRE((int64_t)num_queries * (refine > k ? refine : k) < INT32_MAX, "num_queries * max(k, refine) must be < 2^31");
  KnnIvfHalfPlan plan;
  rc = knn_ivf_half_plan(ix, nprobe, num_queries, &plan);
  if (rc != GLX_OK) return rc;
  return knn_search_entry(ix->device, ix->dim, queries, num_queries, k, ids_out, dist_out, ptr_kind, stream,
                          [&](const float* d_q, int64_t* d_ids, float* d_dist, hipStream_t s) {
                            return knn_ivf_search_half_device(ix, plan, metric, d_q, num_queries, k, nprobe, refine,
                                                              d_ids, d_dist, s);
                          });
}
