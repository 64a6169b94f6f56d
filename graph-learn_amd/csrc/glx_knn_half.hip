// glx KNN search, half-precision scan (GLX_KNN_PREC_HALF of glx_knn_search_ex): a bfloat16 / float16 table is scored on
// the 16-bit matrix cores, v_mfma_f32_32x32x16_bf16 / _f16, from the words as they lie in HBM -- no upcast, no second
// copy.  A float8 table (e4m3fn / e5m2) is scored by the same bfloat16 loop behind a row front that widens its bytes in
// registers.  An opt-in second precision next to the exact search (glx_knn.hip), which keeps its bits.
//
// Contract (DESIGN.md 4, K-knn-half; include/glx.h).  The float32 queries are rounded once per search to the scan type
// -- the table's type, bfloat16 for a float8 table (nearest even, the uploads' converter): q^.  ip(q, r) is the matrix
// cores' float32 accumulator: +0.0f, then one 32x32x16 step per block of 16 columns, ascending, over the exact products
// q^[c] * x[r][c]; columns from dim up are zero in both operands.  The steps of a (query, row) never depend on the
// schedule, so neither do its bits.  IP: dist = ip.  L2: knn_l2(ip, qn, xn), qn the VALU norm chain over q^, xn the
// table's cached norms.  Order, key, ids and padding are the exact search's; a zero distance comes back as +0.0f and a
// NaN as 0x7fc00000.  refine > 0: the scan keeps the refine best, knn_refine (IVF-PQ's re-rank) re-scores them with the
// exact search's fmaf chain against the float32 queries as given, and the k best of those are returned with the exact
// search's distances.
// float8: every e4m3fn and e5m2 code is a bfloat16 number (3 / 2 mantissa bits in 7, float32's exponent range), so the
// widening rounds nothing and the MFMA sees the operands of the bfloat16 table T16 that holds the same values; xn is the
// float32 chain over the same upcast values.  A search of a float8 table therefore returns what the same search of T16
// returns -- ids, distance bits, tie order, padding, NaN last by row -- on every call and under every chunking, and
// with refine > 0 the exact search's distances of those rows, which the two tables share as well.  The queries are not
// rounded to float8 and the float8 / scaled MFMA instructions are not used: 3 or 2 mantissa bits in q^ would add an error
// of 2^-4 / 2^-3 per element to the table's own, and the scores are not what bounds the scan.
//
// Schedule.  knn_chunk_passes: the exact search's chunks, query blocks, init and select.  Per chunk,
// knn_score_half_kernel computes the exact search's tile: 128 queries x 128 rows, four waves as 2 x 2, four 32x32
// accumulators per wave across the whole column loop, and the shared epilogue (knn_tile_epilogue).  The row fronts
// (HalfRow, knn_half_group) and the MFMA step live in glx_knn.h: the narrow tile (glx_knn_narrow.hip) uses them too.
// In front of the tile:
//   queries   knn_round_queries_kernel writes q^ as [num_queries, dim rounded up to 8] 16-bit words, zero past dim, so
//             every query load is one aligned 16-byte load.
//   rows      raw elements go global -> registers -> LDS, a group of eight columns a lane and load: 16 bytes of a 16-bit
//             table where its base and pitch are 16-byte aligned, 8 bytes of a float8 table where its base and pitch
//             (the pitch is in elements = bytes) are 8-byte aligned; element by element otherwise (a view at an odd
//             offset or pitch) and in the tail group of dim % 8 columns, which is zero-filled.  No load touches a byte
//             outside [row, row + dim) elements of a row in [row0, row1): a vector load over the tail would bring the
//             next row's first columns into a padded operand, where a NaN gives 0 * NaN, and on the last row it would
//             leave the allocation.
//   float8    a lane keeps the group -> (tile row, group) map of the 16-bit front: group t & 7 of tile rows t >> 3 + 32 j,
//             j < 4.  A row's stage is then 64 contiguous bytes read by eight consecutive lanes, 8 bytes each, and a
//             wave's load covers eight rows; the four loads of a stage stay raw (8 VGPRs, half the 16-bit front's)
//             while the current stage's MFMA steps run and are widened on the way into LDS: v_cvt_pk_f32_fp8 / _bf8
//             per pair of codes, then v_perm_b32 takes the two high halves as one dword.  The float32 of a number or an
//             infinity has a zero low half, so that is exact.  Both converters return 0xFFC00000 for every NaN code
//             (e4m3fn 0x7F / 0xFF, e5m2 0x7D-0x7F / 0xFD-0xFF; read back from an MI355X over all 256 codes): the high
//             half 0xFFC0 is a quiet NaN word already, so nothing is forced.  A 16-byte load that feeds two groups was
//             not taken: it halves the load instructions of a front that is not the bound
//             (profiles/knn_half/probe.txt: epilogue and select are), needs 16-byte alignment plus an 8-byte and an
//             element path behind it for the stage's last piece, and gives a lane two adjacent 16-byte LDS stores per
//             load, which the bank analysis below does not cover.  Keeping the bytes in LDS and widening at operand
//             read was not built either: every operand is read by two waves, so it doubles the conversions and puts
//             them between the MFMA steps, to save LDS that already fits two workgroups per CU.
//   LDS       a stage is 64 columns: tiles of 128 rows x 64 words, row-major at a pitch of 144 bytes (128 + 16).  The
//             operand of step s is lane l: row l & 31, columns 16 s + 8 (l >> 5) .. + 7 -- one 16-byte read.  Rows 144
//             bytes apart start 16 bytes further round a 128-byte line each, so eight consecutive lanes (the lanes a
//             16-byte access serves together) read eight different 16-byte bank groups, and so do sixteen lanes over a
//             256-byte line; a stage's writes put eight consecutive lanes on one row's 128 contiguous bytes.  Derived
//             from the addresses, not measured.  Two buffers of (A, B): 2 * 2 * 128 * 144 = 73,728 bytes, two
//             workgroups (eight waves) per CU of 160 KB.  The next stage's global loads are issued before the current
//             stage's MFMA steps and stored to the other buffer after them: one barrier per stage.  A float8 table
//             stores the same words at the same addresses.
#include "glx_knn.h"

#pragma clang fp contract(off)

namespace {

constexpr int kHalfBK = 64;                 // columns per stage
constexpr int kHalfGroups = kHalfBK / 8;    // 16-byte groups per tile row
constexpr int kHalfLd = kHalfGroups + 1;    // LDS pitch in 16-byte units: 144 bytes
constexpr int kHalfLoads = kBR * kHalfGroups / 256;  // groups a lane moves per tile and stage

// q^: out[q, c] = queries[q, c] rounded to DT for c < dim, zero for dim <= c < ld
template <int DT>
__global__ __launch_bounds__(256) void knn_round_queries_kernel(const float* __restrict__ queries, int64_t n, int32_t dim,
                                                                int32_t ld, uint16_t* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i >= n * ld) return;
  const int64_t q = i / ld;
  const int32_t c = (int32_t)(i % ld);
  uint16_t v = 0;
  if (c < dim) {
    const uint32_t u = __float_as_uint(queries[q * dim + c]);
    v = DT == GLX_DTYPE_BF16 ? glx_f32_to_bf16_bits(u) : glx_f32_to_f16_bits(u);
  }
  out[i] = v;
}

// One (128 queries x 128 rows) tile of half-precision scores for rows [row0, row1), filtered into the candidate
// buffers.  qh: the rounded queries of this block, [a.nq, qld].  Rows past row1 and queries past a.nq are zero operands
// whose outputs the epilogue masks.
template <int DT>
__global__ __launch_bounds__(256, 2) void knn_score_half_kernel(KnnArgs a, const uint16_t* __restrict__ qh, int32_t qld,
                                                                int32_t row0, int32_t row1) {
  __shared__ uint4 As[2][kBQ][kHalfLd];
  __shared__ uint4 Bs[2][kBR][kHalfLd];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int wq = (w & 1) * 64, wr = (w >> 1) * 64;
  const int32_t qbase = blockIdx.y * kBQ;
  const int32_t rbase = row0 + blockIdx.x * kBR;
  const int32_t dim = a.t.dim;
  typedef typename HalfRow<DT>::elem elem_t;
  typedef typename HalfRow<DT>::group group_t;
  const elem_t* const X = static_cast<const elem_t*>(a.t.X);
  const bool vec = (reinterpret_cast<uintptr_t>(X) & (sizeof(group_t) - 1)) == 0 && (a.t.stride & 7) == 0;
  const int g = t & (kHalfGroups - 1), lr = t / kHalfGroups;  // the lane's group, and its first tile row

  // the lane's kHalfLoads queries and rows are the same in every stage
  const uint16_t* qp[kHalfLoads];
  const elem_t* xp[kHalfLoads];
#pragma unroll
  for (int j = 0; j < kHalfLoads; ++j) {
    const int r = lr + (256 / kHalfGroups) * j;
    const int32_t q = qbase + r, row = rbase + r;
    qp[j] = q < a.nq ? qh + (int64_t)q * qld : nullptr;
    xp[j] = row < row1 ? X + glx_swizzle_row(row, a.t.swizzle_rows) * a.t.stride : nullptr;
  }
  auto fetch = [&](int32_t k0, uint4 (&qa)[kHalfLoads], group_t (&xb)[kHalfLoads]) {
    const int32_t c0 = k0 + 8 * g;
#pragma unroll
    for (int j = 0; j < kHalfLoads; ++j) {
      qa[j] = (qp[j] && c0 < qld) ? *reinterpret_cast<const uint4*>(qp[j] + c0) : make_uint4(0u, 0u, 0u, 0u);
      xb[j] = (xp[j] && c0 < dim) ? knn_half_group<group_t>(xp[j], c0, dim, vec) : group_t{};
    }
  };
  auto stash = [&](int buf, const uint4 (&qa)[kHalfLoads], const group_t (&xb)[kHalfLoads]) {
#pragma unroll
    for (int j = 0; j < kHalfLoads; ++j) {
      As[buf][lr + (256 / kHalfGroups) * j][g] = qa[j];
      Bs[buf][lr + (256 / kHalfGroups) * j][g] = HalfRow<DT>::words(xb[j]);
    }
  };

  knn_f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
  uint4 qa[kHalfLoads];
  group_t xb[kHalfLoads];
  fetch(0, qa, xb);
  stash(0, qa, xb);
  __syncthreads();  // stage 0 is in LDS
  int buf = 0;
  for (int32_t k0 = 0; k0 < dim; k0 += kHalfBK) {
    const bool ahead = k0 + kHalfBK < dim;  // uniform: there is a next stage
    if (ahead) fetch(k0 + kHalfBK, qa, xb);
    const int32_t left = dim - k0;
    const int steps = left < kHalfBK ? (left + 15) / 16 : kHalfBK / 16;  // one step per block of 16 columns, no more
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
  knn_tile_epilogue(a, acc, qbase, rbase, row1, wq, wr, l31, half);
}

// keys -> (node id, dist); one lane per output slot.  The image in a key gives back every number's bits with a zero as
// +0.0f; a NaN is the quiet NaN.
__global__ __launch_bounds__(256) void knn_half_finish_kernel(KnnArgs a, const int64_t* __restrict__ row_ids,
                                                              int64_t id_base, int64_t id_step,
                                                              int64_t* __restrict__ ids_out, float* __restrict__ dist_out) {
  const int64_t o = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (o >= (int64_t)a.nq * a.k) return;
  const int32_t q = (int32_t)(o / a.k), j = (int32_t)(o % a.k);
  const uint64_t key = a.run[(int64_t)q * a.KP + j];
  if (key == kNoKey) return knn_emit_absent(o, a.metric, ids_out, dist_out);
  const uint32_t ord = (uint32_t)(key >> 32);
  dist_out[o] = __uint_as_float(ord == 0xffffffffu ? 0x7fc00000u : knn_unord(ord, a.metric));
  ids_out[o] = knn_row_id((int64_t)(uint32_t)key, row_ids, id_base, id_step);
}

}  // namespace

// knn_score_half_kernel of the table's storage type
static void knn_score_half(const KnnArgs& a, const uint16_t* qh, int32_t qld, int32_t row0, int32_t row1, dim3 grid,
                           hipStream_t s) {
  switch (a.t.dtype) {
    case GLX_DTYPE_BF16: knn_score_half_kernel<GLX_DTYPE_BF16><<<grid, 256, 0, s>>>(a, qh, qld, row0, row1); break;
    case GLX_DTYPE_F16: knn_score_half_kernel<GLX_DTYPE_F16><<<grid, 256, 0, s>>>(a, qh, qld, row0, row1); break;
    case GLX_DTYPE_F8E4M3: knn_score_half_kernel<GLX_DTYPE_F8E4M3><<<grid, 256, 0, s>>>(a, qh, qld, row0, row1); break;
    default: knn_score_half_kernel<GLX_DTYPE_F8E5M2><<<grid, 256, 0, s>>>(a, qh, qld, row0, row1); break;
  }
}

void knn_round_queries(const float* d_q, int64_t num_queries, int32_t dim, int32_t ld, int scan, uint16_t* out,
                       hipStream_t s) {
  const unsigned grid = (unsigned)((num_queries * ld + 255) / 256);
  if (scan == GLX_DTYPE_BF16) {
    knn_round_queries_kernel<GLX_DTYPE_BF16><<<grid, 256, 0, s>>>(d_q, num_queries, dim, ld, out);
  } else {
    knn_round_queries_kernel<GLX_DTYPE_F16><<<grid, 256, 0, s>>>(d_q, num_queries, dim, ld, out);
  }
}

void knn_half_finish(const KnnArgs& a, const glx_features* f, int64_t* d_ids, float* d_dist, hipStream_t s) {
  const bool arith = f->idmap.keys == nullptr && f->idmap.step > 0;
  knn_half_finish_kernel<<<(unsigned)(((int64_t)a.nq * a.k + 255) / 256), 256, 0, s>>>(
      a, f->knn_row_ids, arith ? f->idmap.base : 0, arith ? f->idmap.step : 0, d_ids, d_dist);
}

int knn_search_half_device(const glx_features* f, int metric, const float* d_q, int32_t num_queries, int32_t k,
                           int32_t refine, int64_t* d_ids, float* d_dist, hipStream_t s, int tile) {
  const bool narrow = tile == GLX_KNN_TILE_NARROW;
  const bool l2 = metric == GLX_KNN_L2;
  KnnArgs a;  // the scan: the refine best (k without refine) by the half score
  memset(&a, 0, sizeof(a));
  a.t = knn_table(f);
  a.k = refine > 0 ? refine : k;
  a.KP = knn_pow2_at_least(a.k);
  a.metric = metric;
  const KnnChunkPlan plan = narrow ? knn_chunk_plan(a.t.num_rows, num_queries, kNarrowBQ, kNarrowBR)
                                   : knn_chunk_plan(a.t.num_rows, num_queries);
  a.cap = (int32_t)plan.chunk;
  KnnArgs x = a;  // the re-rank: the k best of those by the exact search's chain
  x.k = k;
  x.KP = knn_pow2_at_least(k);
  const int32_t qld = (a.t.dim + 7) & ~7;

  // workspace slot 1
  uint16_t* qh;
  float *qn_half, *qn_exact, *xn_ws;
  auto layout = [&](KnnCarve c) {
    qh = c.take<uint16_t>((size_t)num_queries * qld);
    qn_half = c.take<float>(num_queries);
    qn_exact = c.take<float>(num_queries, l2 && refine > 0);
    xn_ws = c.take<float>(a.t.num_rows, l2 && !f->owns_x);
    a.thr = c.take<uint32_t>(plan.qb);
    a.cnt = c.take<uint32_t>(plan.qb);
    a.run = c.take<uint64_t>(plan.qb * a.KP);
    a.cand = c.take<uint64_t>(plan.qb * a.cap);
    x.run = c.take<uint64_t>(plan.qb * x.KP, refine > 0);
    return c.off;
  };
  GlxScratch ws;
  int rc = ws.alloc(layout(KnnCarve{nullptr}), s, 1);
  if (rc != GLX_OK) return rc;
  layout(KnnCarve{ws.as<char>()});
  const int scan = a.t.dtype == GLX_DTYPE_F16 ? GLX_DTYPE_F16 : GLX_DTYPE_BF16;  // a float8 table scans as bfloat16
  knn_round_queries(d_q, num_queries, a.t.dim, qld, scan, qh, s);
  rc = knn_prepare_norms(f, l2, qh, num_queries, qn_half, xn_ws, s, &a.xn, scan, qld);
  if (rc != GLX_OK) return rc;
  x.xn = a.xn;
  if (qn_exact) knn_norms(KnnTable{d_q, a.t.dim, 0, num_queries, a.t.dim, GLX_DTYPE_F32}, qn_exact, s);
  int refine_rc = GLX_OK;
  rc = knn_chunk_passes(
      a, plan, d_q, qn_half, num_queries, s,
      [&](int64_t q0, int32_t row0, int32_t row1, dim3 grid) {
        if (narrow) return knn_score_narrow_half(a, qh + q0 * qld, qld, row0, row1, grid, s);
        knn_score_half(a, qh + q0 * qld, qld, row0, row1, grid, s);
        return GLX_OK;
      },
      [&](int64_t q0) {
        if (refine == 0) {
          knn_half_finish(a, f, d_ids + q0 * k, d_dist + q0 * k, s);
          return;
        }
        x.nq = a.nq;
        x.queries = a.queries;
        x.qn = qn_exact ? qn_exact + q0 : nullptr;
        if (refine_rc == GLX_OK) refine_rc = knn_refine(x, a.run, a.KP, refine, s);
        knn_finish(x, f, d_ids + q0 * k, d_dist + q0 * k, s);
      });
  return rc != GLX_OK ? rc : refine_rc;
}

extern "C" int glx_knn_search_ex(const glx_features* f, int metric, const float* queries, int32_t num_queries, int32_t k,
                                 int precision, int32_t refine, int64_t* ids_out, float* dist_out, int ptr_kind,
                                 void* stream) {
  return glx_knn_search_tiled(f, metric, queries, num_queries, k, precision, refine, GLX_KNN_TILE_WIDE, ids_out, dist_out,
                              ptr_kind, stream);
}
