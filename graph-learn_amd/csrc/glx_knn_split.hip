// glx KNN search, split scan (GLX_KNN_PREC_SPLIT of glx_knn_search_ex): a float32 table is scored on the bfloat16
// matrix cores, v_mfma_f32_32x32x16_bf16, from the float32 words as they lie in HBM -- no second copy, no rounded
// queries.  A float32 number is the sum of three bfloat16 numbers and a bfloat16 x bfloat16 product is exact in the
// float32 accumulator, so six steps over the piece pairs that matter give float32-grade scores for 16 columns, where the
// exact search (glx_knn.hip) spends eight v_mfma_f32_32x32x2_f32 steps.  An opt-in third precision; the exact search
// and the half-precision scan (glx_knn_half.hip) keep their bits.
//
// Contract (DESIGN.md 4, K-knn-split; include/glx.h).  Every float32 v of the table and of the queries is split as
// h = bf16(v), m = bf16(v - h), l = bf16(v - h - m), each to nearest even with the uploads' converter; both differences
// are exact and v == h + m + l unless a piece falls below 2^-133.  A finite v whose h would round to +-inf keeps the
// truncated word, +-inf is (v, 0, 0) and a NaN is (the quiet NaN of its sign, 0, 0).  ip(q, r) is the matrix cores'
// float32 accumulator: +0.0f, then per block of 16 columns, ascending, six 32x32x16 steps over the piece pairs
// (ql, xh), (qh, xl), (qm, xm), (qm, xh), (qh, xm), (qh, xh) -- the smallest magnitudes first; (qm, xl), (ql, xm) and
// (ql, xl) are dropped.  Columns from dim up are zero in every plane.  The steps of a (query, row) never depend on the
// schedule, so neither do its bits.  IP: dist = ip.  L2: knn_l2(ip, qn, xn) with the exact search's own qn and xn.
// Order, key, ids, padding, the +0.0f zero, the canonical NaN and refine are the half-precision scan's.  An infinite
// element meets the zero m and l pieces of the other operand as 0 * inf: its (query, row) scores NaN and ranks last.
//
// Schedule.  knn_chunk_passes with the exact search's chunk plan.  Per chunk knn_score_split_kernel computes the tile of
// knn_score_half_kernel: 128 queries x 128 rows, four waves as 2 x 2, four 32x32 accumulators per wave across the whole
// column loop, and the shared epilogue (knn_tile_epilogue).  In front of the tile:
//   queries   knn_split_queries_kernel writes the three planes once per search as [3][num_queries, dim rounded up to 8]
//             16-bit words, zero past dim, so every query load is one aligned 16-byte load of a plane.
//   rows      raw float32 words go global -> registers -> LDS, a group of eight columns a lane: two 16-byte loads where
//             base and pitch are 16-byte aligned, element by element otherwise and in the tail (knn_f32_quad).  No load
//             touches a byte outside [row, row + dim) elements of a row in [row0, row1).  The words stay raw (8 VGPRs)
//             while the current stage's MFMA steps run and are split on the way into LDS, not at operand read: every
//             operand is read by two waves, so splitting there would double the conversions and put them between the
//             MFMA steps (the argument the float8 front of glx_knn_half.hip records).
//   LDS       six planes per buffer, A{h,m,l} and B{h,m,l}, of 128 rows.  A stage is 16 columns: 32 bytes of a plane
//             row at a pitch of 48 bytes.  The operand of the stage is lane l: row l & 31, columns 8 (l >> 5) .. + 7 --
//             one 16-byte read per plane.  Rows 48 bytes apart put eight consecutive lanes (the lanes a 16-byte access
//             serves together) on offsets 0, 48, 96, 16, 64, 112, 32, 80 of a 128-byte line: eight different 16-byte
//             bank groups.  Derived from the addresses, not measured.  Two buffers: 2 * 6 * 128 * 48 = 73,728 bytes,
//             the half scan's footprint, two workgroups (eight waves) per CU.  The next stage's global loads are issued
//             before the current stage's 24 MFMA steps and split and stored to the other buffer after them: one barrier
//             per stage, no LDS transpose.
//             A stage of 32 columns (pitch 80 bytes, 122,880 bytes, one workgroup per CU) compiles from the same code
//             with -DGLX_KNN_SPLIT_BK=32; DESIGN.md 11 says why it is not the one built.
#include "glx_knn.h"

#pragma clang fp contract(off)

namespace {

#ifndef GLX_KNN_SPLIT_BK
#define GLX_KNN_SPLIT_BK 16
#endif
constexpr int kSplitBK = GLX_KNN_SPLIT_BK;        // columns per stage
constexpr int kSplitGroups = kSplitBK / 8;        // 16-byte groups per plane row
constexpr int kSplitLd = kSplitGroups + 1;        // LDS pitch in 16-byte units: 48 bytes
constexpr int kSplitPass = 256 / kSplitGroups;    // tile rows the workgroup moves per load
constexpr int kSplitLoads = kBR / kSplitPass;     // groups a lane moves per tile and stage
constexpr int kSplitWgPerCu = kSplitBK == 16 ? 2 : 1;
static_assert(kSplitBK == 16 || kSplitBK == 32, "a stage is 16 or 32 columns");

// the three bfloat16 pieces of a float32 word, as 16-bit words
struct KnnPieces {
  uint32_t h, m, l;
};
__device__ __forceinline__ KnnPieces knn_split3(uint32_t u) {
  const uint32_t a = u & 0x7fffffffu;
  if (a >= 0x7f800000u) return KnnPieces{a > 0x7f800000u ? ((u >> 16) & 0x8000u) | 0x7fc0u : u >> 16, 0u, 0u};
  const uint32_t h = a >= 0x7f7f8000u ? u >> 16 : glx_f32_to_bf16_bits(u);  // never rounded up to inf
  const float r1 = __uint_as_float(u) - __uint_as_float(h << 16);           // exact
  const uint32_t m = glx_f32_to_bf16_bits(__float_as_uint(r1));
  const float r2 = r1 - __uint_as_float(m << 16);                           // exact
  return KnnPieces{h, m, glx_f32_to_bf16_bits(__float_as_uint(r2))};
}

// eight float32 words -> the eight 16-bit words of each plane's operand group
__device__ __forceinline__ void knn_split_group(uint4 lo, uint4 hi, uint4 (&out)[3]) {
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  uint32_t p[3][4];
#pragma unroll
  for (int e = 0; e < 8; e += 2) {
    const KnnPieces x = knn_split3(w[e]), y = knn_split3(w[e + 1]);
    p[0][e >> 1] = x.h | (y.h << 16);
    p[1][e >> 1] = x.m | (y.m << 16);
    p[2][e >> 1] = x.l | (y.l << 16);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) out[i] = make_uint4(p[i][0], p[i][1], p[i][2], p[i][3]);
}

// out[p][q, c] = piece p (h, m, l) of queries[q, c] for c < dim, zero for dim <= c < ld
__global__ __launch_bounds__(256) void knn_split_queries_kernel(const float* __restrict__ queries, int64_t n, int32_t dim,
                                                                int32_t ld, uint16_t* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i >= n * ld) return;
  const int64_t q = i / ld;
  const int32_t c = (int32_t)(i % ld);
  KnnPieces v{0u, 0u, 0u};
  if (c < dim) v = knn_split3(__float_as_uint(queries[q * dim + c]));
  out[i] = (uint16_t)v.h;
  out[n * ld + i] = (uint16_t)v.m;
  out[2 * n * ld + i] = (uint16_t)v.l;
}

// One (128 queries x 128 rows) tile of split scores for rows [row0, row1), filtered into the candidate buffers.  qs:
// plane h of this block's queries, [a.nq, qld]; planes m and l lie `plane` and 2 * `plane` words further.  Rows past
// row1 and queries past a.nq are zero operands whose outputs the epilogue masks.
__global__ __launch_bounds__(256, kSplitWgPerCu) void knn_score_split_kernel(KnnArgs a, const uint16_t* __restrict__ qs,
                                                                             int64_t plane, int32_t qld, int32_t row0,
                                                                             int32_t row1) {
  __shared__ uint4 As[2][3][kBQ][kSplitLd];
  __shared__ uint4 Bs[2][3][kBR][kSplitLd];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int wq = (w & 1) * 64, wr = (w >> 1) * 64;
  const int32_t qbase = blockIdx.y * kBQ;
  const int32_t rbase = row0 + blockIdx.x * kBR;
  const int32_t dim = a.t.dim;
  const float* const X = static_cast<const float*>(a.t.X);
  const bool vec = (reinterpret_cast<uintptr_t>(X) & 15) == 0 && (a.t.stride & 3) == 0;
  const int g = t & (kSplitGroups - 1), lr = t / kSplitGroups;  // the lane's group, and its first tile row

  // the lane's kSplitLoads queries and rows are the same in every stage
  const uint16_t* qp[kSplitLoads];
  const float* xp[kSplitLoads];
#pragma unroll
  for (int j = 0; j < kSplitLoads; ++j) {
    const int r = lr + kSplitPass * j;
    const int32_t q = qbase + r, row = rbase + r;
    qp[j] = q < a.nq ? qs + (int64_t)q * qld : nullptr;
    xp[j] = row < row1 ? X + glx_swizzle_row(row, a.t.swizzle_rows) * a.t.stride : nullptr;
  }
  auto fetch = [&](int32_t k0, uint4 (&qa)[kSplitLoads][3], uint4 (&xb)[kSplitLoads][2]) {
    const int32_t c0 = k0 + 8 * g;
#pragma unroll
    for (int j = 0; j < kSplitLoads; ++j) {
#pragma unroll
      for (int p = 0; p < 3; ++p)
        qa[j][p] = (qp[j] && c0 < qld) ? *reinterpret_cast<const uint4*>(qp[j] + p * plane + c0) : make_uint4(0u, 0u, 0u, 0u);
      xb[j][0] = xp[j] ? knn_f32_quad(xp[j], c0, dim, vec) : make_uint4(0u, 0u, 0u, 0u);
      xb[j][1] = xp[j] ? knn_f32_quad(xp[j], c0 + 4, dim, vec) : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  auto stash = [&](int buf, const uint4 (&qa)[kSplitLoads][3], const uint4 (&xb)[kSplitLoads][2]) {
#pragma unroll
    for (int j = 0; j < kSplitLoads; ++j) {
      uint4 xs[3];
      knn_split_group(xb[j][0], xb[j][1], xs);
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        As[buf][p][lr + kSplitPass * j][g] = qa[j][p];
        Bs[buf][p][lr + kSplitPass * j][g] = xs[p];
      }
    }
  };

  knn_f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
  uint4 qa[kSplitLoads][3], xb[kSplitLoads][2];
  fetch(0, qa, xb);
  stash(0, qa, xb);
  __syncthreads();  // stage 0 is in LDS
  int buf = 0;
  for (int32_t k0 = 0; k0 < dim; k0 += kSplitBK) {
    const bool ahead = k0 + kSplitBK < dim;  // uniform: there is a next stage
    if (ahead) fetch(k0 + kSplitBK, qa, xb);
    const int32_t left = dim - k0;
    const int steps = left < kSplitBK ? (left + 15) / 16 : kSplitBK / 16;  // six steps per block of 16 columns, no more
    for (int s = 0; s < steps; ++s) {
      const int u = 2 * s + half;
      const uint4 qh[2] = {As[buf][0][wq + l31][u], As[buf][0][wq + 32 + l31][u]};
      const uint4 qm[2] = {As[buf][1][wq + l31][u], As[buf][1][wq + 32 + l31][u]};
      const uint4 ql[2] = {As[buf][2][wq + l31][u], As[buf][2][wq + 32 + l31][u]};
      const uint4 xh[2] = {Bs[buf][0][wr + l31][u], Bs[buf][0][wr + 32 + l31][u]};
      const uint4 xm[2] = {Bs[buf][1][wr + l31][u], Bs[buf][1][wr + 32 + l31][u]};
      const uint4 xl[2] = {Bs[buf][2][wr + l31][u], Bs[buf][2][wr + 32 + l31][u]};
      // one piece pair into the wave's four accumulators; six pairs in the contract's order
      auto pair = [&](const uint4 (&q)[2], const uint4 (&x)[2]) {
        acc[0][0] = knn_half_mfma<GLX_DTYPE_BF16>(q[0], x[0], acc[0][0]);
        acc[0][1] = knn_half_mfma<GLX_DTYPE_BF16>(q[0], x[1], acc[0][1]);
        acc[1][0] = knn_half_mfma<GLX_DTYPE_BF16>(q[1], x[0], acc[1][0]);
        acc[1][1] = knn_half_mfma<GLX_DTYPE_BF16>(q[1], x[1], acc[1][1]);
      };
      pair(ql, xh);
      pair(qh, xl);
      pair(qm, xm);
      pair(qm, xh);
      pair(qh, xm);
      pair(qh, xh);
    }
    if (ahead) stash(buf ^ 1, qa, xb);
    __syncthreads();  // the next stage is stored; this one has been consumed
    buf ^= 1;
  }
  knn_tile_epilogue(a, acc, qbase, rbase, row1, wq, wr, l31, half);
}

}  // namespace

int knn_search_split_device(const glx_features* f, int metric, const float* d_q, int32_t num_queries, int32_t k,
                            int32_t refine, int64_t* d_ids, float* d_dist, hipStream_t s) {
  const bool l2 = metric == GLX_KNN_L2;
  KnnArgs a;  // the scan: the refine best (k without refine) by the split score
  memset(&a, 0, sizeof(a));
  a.t = knn_table(f);
  a.k = refine > 0 ? refine : k;
  a.KP = knn_pow2_at_least(a.k);
  a.metric = metric;
  const KnnChunkPlan plan = knn_chunk_plan(a.t.num_rows, num_queries);
  a.cap = (int32_t)plan.chunk;
  KnnArgs x = a;  // the re-rank: the k best of those by the exact search's chain
  x.k = k;
  x.KP = knn_pow2_at_least(k);
  const int32_t qld = (a.t.dim + 7) & ~7;
  const int64_t plane = (int64_t)num_queries * qld;

  // workspace slot 1
  uint16_t* qs;
  float *qn, *xn_ws;
  auto layout = [&](KnnCarve c) {
    qs = c.take<uint16_t>((size_t)(3 * plane));
    qn = c.take<float>(num_queries);
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
  knn_split_queries_kernel<<<(unsigned)((plane + 255) / 256), 256, 0, s>>>(d_q, num_queries, a.t.dim, qld, qs);
  rc = knn_prepare_norms(f, l2, d_q, num_queries, qn, xn_ws, s, &a.xn);  // the exact search's norms: the queries as given
  if (rc != GLX_OK) return rc;
  x.xn = a.xn;
  int refine_rc = GLX_OK;
  rc = knn_chunk_passes(
      a, plan, d_q, qn, num_queries, s,
      [&](int64_t q0, int32_t row0, int32_t row1, dim3 grid) {
        knn_score_split_kernel<<<grid, 256, 0, s>>>(a, qs + q0 * qld, plane, qld, row0, row1);
        return GLX_OK;
      },
      [&](int64_t q0) {
        if (refine == 0) {
          knn_half_finish(a, f, d_ids + q0 * k, d_dist + q0 * k, s);
          return;
        }
        x.nq = a.nq;
        x.queries = a.queries;
        x.qn = l2 ? a.qn : nullptr;
        if (refine_rc == GLX_OK) refine_rc = knn_refine(x, a.run, a.KP, refine, s);
        knn_finish(x, f, d_ids + q0 * k, d_dist + q0 * k, s);
      });
  return rc != GLX_OK ? rc : refine_rc;
}
