// glx KNN search, narrow tile (GLX_KNN_TILE_NARROW of glx_knn_search_tiled): the score kernels of the exact search
// (glx_knn.hip) and of the half-precision scan (glx_knn_half.hip) over a tile of 32 queries x 256 rows.  The wide tile
// pads a request to 128 queries; with a handful of queries three quarters or more of its matrix-core work is padding,
// and that work, not the table's bytes, is what its search takes.  Here a request of up to 32 queries streams the table
// once and multiplies a quarter of the padding; more than 32 queries are legal and re-read the chunk per 32.  Opt-in:
// where the wide tile wins again is a measurement (profiles/knn_narrow/probe.txt), not a rule in this file.
//
// Contract (DESIGN.md 4, K-knn-narrow; include/glx.h): the bits of the wide tile at the same precision and refine.  A
// (query, row)'s score is the wide kernels' own arithmetic --
//   exact   +0.0f, then v_mfma_f32_32x32x2_f32 over ascending column pairs; an odd last column is a VALU fmaf on the
//           accumulator (knn_score_kernel says why it is not a zero-padded step); any storage type through AggElem::up
//   half    +0.0f, then one v_mfma_f32_32x32x16_bf16 / _f16 step per 16 columns, ascending, the tail zero-filled; float8
//           widened exactly to bfloat16 on its way into LDS (HalfRow)
// -- and a score never depends on its place in a tile, so the keys are the wide kernels' keys; the threshold filter only
// drops keys that cannot be among the k best, and everything behind the score kernel (knn_init, knn_select, knn_finish,
// knn_refine, the norms) is shared.
//
// One kernel template, knn_score_narrow_kernel<DT, HALF>, four waves:
//   tile      each wave owns 64 rows against the same 32 queries: two 32x32 accumulators (32 registers; the wide tile
//             holds 64).  A holds queries and B rows as in knn_score_kernel, so one accumulator register still gives a
//             half-wave one query and knn_tile_epilogue<1, 2> is the wide kernels' epilogue.
//   walk      a workgroup takes row tiles blockIdx.x, + gridDim.x, ... of the chunk; the grid is two workgroups per CU
//             over all query tiles (blockIdx.y).  (row tile, column stage) pairs form ONE pipeline: the first stage of
//             the next row tile is in flight under the last stage of this one and its epilogue.
//   LDS       a stage is 128 bytes of every tile row: eight 16-byte units, 32 float32 columns (exact) or 64 16-bit
//             columns (half).  Row tiles: 2 buffers x 256 rows x 128 bytes = 65,536 bytes; queries: 4 stages x 32 x 128
//             = 16,384 bytes; 81,920 together, half a CU's 160 KB, so two workgroups per CU.  No room for a padded
//             pitch: unit u of tile row r lies at u ^ ((r ^ (r >> 3)) & 7) instead.  Derived from the addresses of
//             the accesses, not counted: the MFMA operand read of unit 2 x + half by lanes of rows r .. r + 7 (the
//             lanes a 16-byte access serves together over a 128-byte line) touches eight different 16-byte bank groups,
//             since r & 7 takes every value; over a 256-byte line (sixteen lanes, rows r .. r + 15) the rows of one
//             parity share a 128-byte half, and r ^ (r >> 3) gives the eight of them eight different values as well
//             (rows 8 .. 15 are rows 0 .. 7 with bit 0 flipped).  A stage's stores put eight consecutive lanes on one
//             row's eight units (half) or on the even and the odd units of two neighbouring rows, whose images differ
//             in bit 0 (exact).
//   exact     the MFMA step of columns (2 s, 2 s + 1) wants column 2 s + half from lane (l31, half).  A group of eight
//             columns c .. c + 7 is therefore stored as two units, {c, c+2, c+4, c+6} and {c+1, c+3, c+5, c+7}: a lane's
//             one 16-byte read of unit 2 x + half holds its operands of four steps.
//   queries   the workgroup's 32 query rows are staged once and kept for every row tile it walks: float32 in the exact
//             kernel, the rounded q^ of knn_round_queries_kernel in the half kernel.  That holds up to four stages:
//             dim <= 128 (exact), dim <= 256 (half).  A larger dim stages the queries per column stage into two of
//             the four slots, next to the rows' stage.
//   rows      the stream.  A lane moves groups of eight columns: one 16-byte load of a 16-bit table, one 8-byte load
//             of a float8 table (knn_half_group: both kernels), two 16-byte loads of a float32 table; element loads
//             where the base or the pitch is not aligned to the load and in the tail group, which is zero-filled.  No
//             load touches a byte outside [row, row + dim) elements of a row in [row0, row1).  The next stage's loads
//             are issued before the current stage's MFMA steps and stored to the other buffer after them: one barrier
//             per stage.
// Resource figures of the four kinds of instantiation are in DESIGN.md 11 item 8.
#include "glx_knn.h"

#pragma clang fp contract(off)

namespace {

constexpr int kUnits = 8;     // 16-byte units per tile row and stage
constexpr int kQStages = 4;   // query stages the LDS keeps
constexpr int kWgPerCu = 2;   // what the 81,920 bytes of LDS allow

__device__ __forceinline__ int narrow_sw(int r) { return (r ^ (r >> 3)) & 7; }

// eight float32 columns: two quads of knn_f32_quad
struct NarrowF32Group {
  uint4 lo, hi;
};

// The row front of the exact kernel: group = eight stored elements as loaded, up8 = their float32 values.
template <int DT>
struct NarrowExactRow {
  typedef typename HalfRow<DT>::elem elem;
  typedef typename HalfRow<DT>::group group;
  static __device__ __forceinline__ group load(const elem* p, int32_t c0, int32_t dim, bool vec) {
    return knn_half_group<group>(p, c0, dim, vec);
  }
  static __device__ __forceinline__ void up8(group g, float (&f)[8]) {
    constexpr int kBits = 8 * (int)sizeof(elem), kPer = 32 / kBits;
    struct Words {
      uint32_t w[sizeof(group) / 4];
    };
    const Words v = __builtin_bit_cast(Words, g);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const elem x = (elem)(v.w[e / kPer] >> (kBits * (e % kPer)));
      f[e] = AggElem<DT>::up(__builtin_bit_cast(typename AggElem<DT>::raw, x));
    }
  }
};
template <>
struct NarrowExactRow<GLX_DTYPE_F32> {
  typedef float elem;
  typedef NarrowF32Group group;
  static __device__ __forceinline__ group load(const float* p, int32_t c0, int32_t dim, bool vec) {
    return group{knn_f32_quad(p, c0, dim, vec), knn_f32_quad(p, c0 + 4, dim, vec)};
  }
  static __device__ __forceinline__ void up8(group g, float (&f)[8]) {
    const uint32_t w[8] = {g.lo.x, g.lo.y, g.lo.z, g.lo.w, g.hi.x, g.hi.y, g.hi.z, g.hi.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = __uint_as_float(w[e]);
  }
};

// Scores of the 32 queries of tile blockIdx.y against rows [row0, row1), filtered into the candidate buffers.  qsrc: the
// block's queries -- a.queries, float32 [a.nq, dim] (exact); q^, 16-bit [a.nq, qld] (half).  Rows past row1, queries past
// a.nq and columns past dim are zero operands; the epilogue masks their outputs.
template <int DT, bool HALF>
__global__ __launch_bounds__(256, kWgPerCu) void knn_score_narrow_kernel(KnnArgs a, const void* __restrict__ qsrc,
                                                                         int32_t qld, int32_t row0, int32_t row1) {
  typedef typename std::conditional<HALF, HalfRow<DT>, NarrowExactRow<DT>>::type Row;
  typedef typename Row::elem elem_t;
  typedef typename Row::group group_t;
  constexpr int kCols = HALF ? 64 : 32;          // columns per stage
  constexpr int kGroups = kCols / 8;             // groups of eight columns per tile row and stage
  constexpr int kPass = 256 / kGroups;           // tile rows the workgroup moves per load
  constexpr int kLoads = kNarrowBR / kPass;      // groups a lane moves per stage
  __shared__ uint4 Bs[2][kNarrowBR][kUnits];
  __shared__ uint4 Qs[kQStages][kNarrowBQ][kUnits];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int wr = w * 64;
  const int32_t qbase = blockIdx.y * kNarrowBQ;
  const int32_t dim = a.t.dim;
  const int64_t ntiles = ((int64_t)row1 - row0 + kNarrowBR - 1) / kNarrowBR;
  const elem_t* const X = static_cast<const elem_t*>(a.t.X);
  constexpr int kVecBytes = sizeof(group_t) < 16 ? (int)sizeof(group_t) : 16, kVecElems = kVecBytes / (int)sizeof(elem_t);
  const bool vec = (reinterpret_cast<uintptr_t>(X) & (kVecBytes - 1)) == 0 && (a.t.stride & (kVecElems - 1)) == 0;
  const int g = t & (kGroups - 1), lr = t / kGroups;  // the lane's group, and its first tile row
  const bool resident = dim <= kQStages * kCols;

  // slot of Qs = columns [k0, k0 + kCols) of the 32 queries: one unit a lane
  auto stage_queries = [&](int slot, int32_t k0) {
    const int qi = t >> 3, u = t & 7;
    const int32_t q = qbase + qi;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (q < a.nq) {
      if constexpr (HALF) {
        const int32_t c0 = k0 + 8 * u;
        if (c0 < qld) v = *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(qsrc) + (int64_t)q * qld + c0);
      } else {
        const float* const qv = static_cast<const float*>(qsrc) + (int64_t)q * dim;
        const int32_t c = k0 + 8 * (u >> 1) + (u & 1);  // the unit holds columns c, c + 2, c + 4, c + 6
        if (c < dim) v.x = __float_as_uint(qv[c]);
        if (c + 2 < dim) v.y = __float_as_uint(qv[c + 2]);
        if (c + 4 < dim) v.z = __float_as_uint(qv[c + 4]);
        if (c + 6 < dim) v.w = __float_as_uint(qv[c + 6]);
      }
    }
    Qs[slot][qi][u ^ narrow_sw(qi)] = v;
  };
  const elem_t* xp[kLoads];  // the lane's rows of the tile being fetched
  auto set_rows = [&](int64_t tile) {
#pragma unroll
    for (int j = 0; j < kLoads; ++j) {
      const int64_t row = row0 + tile * kNarrowBR + lr + kPass * j;
      xp[j] = row < row1 ? X + glx_swizzle_row(row, a.t.swizzle_rows) * a.t.stride : nullptr;
    }
  };
  auto fetch = [&](int32_t k0, group_t (&xb)[kLoads]) {
    const int32_t c0 = k0 + 8 * g;
#pragma unroll
    for (int j = 0; j < kLoads; ++j) {
      if (xp[j] && c0 < dim) {
        if constexpr (HALF) xb[j] = knn_half_group<group_t>(xp[j], c0, dim, vec);
        else xb[j] = Row::load(xp[j], c0, dim, vec);
      } else {
        xb[j] = group_t{};
      }
    }
  };
  auto stash = [&](int buf, const group_t (&xb)[kLoads]) {
#pragma unroll
    for (int j = 0; j < kLoads; ++j) {
      const int r = lr + kPass * j, sw = narrow_sw(r);
      if constexpr (HALF) {
        Bs[buf][r][g ^ sw] = Row::words(xb[j]);
      } else {
        float f[8];
        Row::up8(xb[j], f);
        Bs[buf][r][(2 * g) ^ sw] =
            make_uint4(__float_as_uint(f[0]), __float_as_uint(f[2]), __float_as_uint(f[4]), __float_as_uint(f[6]));
        Bs[buf][r][(2 * g + 1) ^ sw] =
            make_uint4(__float_as_uint(f[1]), __float_as_uint(f[3]), __float_as_uint(f[5]), __float_as_uint(f[7]));
      }
    }
  };

  knn_f32x16 acc[1][2];
  auto clear = [&]() {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[0][j][r] = 0.0f;
  };
  clear();
  int64_t tile = blockIdx.x;
  if (tile >= ntiles) return;  // uniform
  group_t xb[kLoads];
  set_rows(tile);
  fetch(0, xb);
  if (resident) {
    for (int32_t k0 = 0, slot = 0; k0 < dim; k0 += kCols, ++slot) stage_queries(slot, k0);
  } else {
    stage_queries(0, 0);
  }
  stash(0, xb);
  __syncthreads();  // stage 0 and the queries are in LDS
  const int br0 = wr + l31, br1 = wr + 32 + l31;  // the lane's two B rows, and their and the query row's unit images
  const int sw0 = narrow_sw(br0), sw1 = narrow_sw(br1), swq = narrow_sw(l31);
  int buf = 0;
  int32_t k0 = 0;
  while (tile < ntiles) {
    int64_t next_tile = tile;
    int32_t next_k0 = k0 + kCols;
    if (next_k0 >= dim) {
      next_tile = tile + gridDim.x;
      next_k0 = 0;
    }
    const bool ahead = next_tile < ntiles;  // uniform: there is a next stage
    if (ahead) {
      if (next_k0 == 0) set_rows(next_tile);
      fetch(next_k0, xb);
    }
    const uint4(*const Qt)[kUnits] = Qs[resident ? k0 / kCols : buf];
    const int32_t left = dim - k0;
    if constexpr (HALF) {
      const int steps = left < kCols ? (left + 15) / 16 : kCols / 16;  // one step per block of 16 columns, no more
      for (int s = 0; s < steps; ++s) {
        const uint4 qa = Qt[l31][(2 * s + half) ^ swq];
        const uint4 b0 = Bs[buf][br0][(2 * s + half) ^ sw0], b1 = Bs[buf][br1][(2 * s + half) ^ sw1];
        acc[0][0] = knn_half_mfma<Row::kScan>(qa, b0, acc[0][0]);
        acc[0][1] = knn_half_mfma<Row::kScan>(qa, b1, acc[0][1]);
      }
    } else {
      const int32_t even = (dim & ~1) - k0;
      const int pairs = even < kCols ? (even > 0 ? even / 2 : 0) : kCols / 2;  // column pairs of this stage, no more
      for (int x = 0; 4 * x < pairs; ++x) {
        const uint4 qa = Qt[l31][(2 * x + half) ^ swq];
        const uint4 b0 = Bs[buf][br0][(2 * x + half) ^ sw0], b1 = Bs[buf][br1][(2 * x + half) ^ sw1];
        const uint32_t qw[4] = {qa.x, qa.y, qa.z, qa.w}, w0[4] = {b0.x, b0.y, b0.z, b0.w}, w1[4] = {b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int ss = 0; ss < 4; ++ss) {
          if (4 * x + ss < pairs) {  // uniform
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(qw[ss]), __uint_as_float(w0[ss]), acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(qw[ss]), __uint_as_float(w1[ss]), acc[0][1], 0, 0, 0);
          }
        }
      }
      if ((dim & 1) && k0 + kCols >= dim) {
        // the odd last column (an even offset kk into the stage: word kk >> 1 & 3 of unit 2 (kk >> 3)): a real fmaf on the
        // accumulator, as in knn_score_kernel
        const int kk = dim - 1 - k0, u = 2 * (kk >> 3), wd = (kk >> 1) & 3;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const float xv = reinterpret_cast<const float*>(&Bs[buf][j ? br1 : br0][u ^ (j ? sw1 : sw0)])[wd];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int qi = (r & 3) + 8 * (r >> 2) + 4 * half;
            const float qv = reinterpret_cast<const float*>(&Qt[qi][u ^ narrow_sw(qi)])[wd];
            acc[0][j][r] = __builtin_fmaf(qv, xv, acc[0][j][r]);
          }
        }
      }
    }
    if (ahead) {
      if (!resident) stage_queries(buf ^ 1, next_k0);
      stash(buf ^ 1, xb);
    }
    __syncthreads();  // the next stage is stored; this one has been consumed
    buf ^= 1;
    if (next_k0 == 0) {  // uniform: the tile's last stage
      knn_tile_epilogue(a, acc, qbase, (int32_t)(row0 + tile * kNarrowBR), row1, 0, wr, l31, half);
      clear();
    }
    tile = next_tile;
    k0 = next_k0;
  }
}

// grid of a narrow launch: the row tiles a workgroup walks start at blockIdx.x; kWgPerCu workgroups per CU over all
// query tiles
int narrow_grid(dim3 tiles, dim3* grid) {
  int cus = 0;
  const int rc = glx_device_cus(&cus);
  if (rc != GLX_OK) return rc;
  unsigned x = (unsigned)cus * kWgPerCu / tiles.y;
  if (x < 1) x = 1;
  if (x > tiles.x) x = tiles.x;
  *grid = dim3(x, tiles.y);
  return GLX_OK;
}

}  // namespace

int knn_score_narrow(const KnnArgs& a, int32_t row0, int32_t row1, dim3 tiles, hipStream_t s) {
  dim3 grid;
  const int rc = narrow_grid(tiles, &grid);
  if (rc != GLX_OK) return rc;
  switch (a.t.dtype) {
    case GLX_DTYPE_F32: knn_score_narrow_kernel<GLX_DTYPE_F32, false><<<grid, 256, 0, s>>>(a, a.queries, 0, row0, row1); break;
    case GLX_DTYPE_BF16: knn_score_narrow_kernel<GLX_DTYPE_BF16, false><<<grid, 256, 0, s>>>(a, a.queries, 0, row0, row1); break;
    case GLX_DTYPE_F16: knn_score_narrow_kernel<GLX_DTYPE_F16, false><<<grid, 256, 0, s>>>(a, a.queries, 0, row0, row1); break;
    case GLX_DTYPE_F8E4M3: knn_score_narrow_kernel<GLX_DTYPE_F8E4M3, false><<<grid, 256, 0, s>>>(a, a.queries, 0, row0, row1); break;
    case GLX_DTYPE_F8E5M2: knn_score_narrow_kernel<GLX_DTYPE_F8E5M2, false><<<grid, 256, 0, s>>>(a, a.queries, 0, row0, row1); break;
    default:
      glx_set_error("knn_score_narrow_kernel: no instantiation for storage dtype %d", a.t.dtype);
      return GLX_INTERNAL;
  }
  return GLX_OK;
}

int knn_score_narrow_half(const KnnArgs& a, const uint16_t* qh, int32_t qld, int32_t row0, int32_t row1, dim3 tiles,
                          hipStream_t s) {
  dim3 grid;
  const int rc = narrow_grid(tiles, &grid);
  if (rc != GLX_OK) return rc;
  switch (a.t.dtype) {
    case GLX_DTYPE_BF16: knn_score_narrow_kernel<GLX_DTYPE_BF16, true><<<grid, 256, 0, s>>>(a, qh, qld, row0, row1); break;
    case GLX_DTYPE_F16: knn_score_narrow_kernel<GLX_DTYPE_F16, true><<<grid, 256, 0, s>>>(a, qh, qld, row0, row1); break;
    case GLX_DTYPE_F8E4M3: knn_score_narrow_kernel<GLX_DTYPE_F8E4M3, true><<<grid, 256, 0, s>>>(a, qh, qld, row0, row1); break;
    default: knn_score_narrow_kernel<GLX_DTYPE_F8E5M2, true><<<grid, 256, 0, s>>>(a, qh, qld, row0, row1); break;
  }
  return GLX_OK;
}

extern "C" int glx_knn_search_tiled(const glx_features* f, int metric, const float* queries, int32_t num_queries,
                                    int32_t k, int precision, int32_t refine, int tile, int64_t* ids_out, float* dist_out,
                                    int ptr_kind, void* stream) {
  GLX_REQUIRE(tile == GLX_KNN_TILE_WIDE || tile == GLX_KNN_TILE_NARROW,
              "tile must be GLX_KNN_TILE_WIDE (0) or GLX_KNN_TILE_NARROW (1), got %d", tile);
  GLX_REQUIRE(f != nullptr, "features is NULL");
  GLX_KNN_REQUIRE();
  GLX_REQUIRE(precision == GLX_KNN_PREC_F32 || precision == GLX_KNN_PREC_HALF || precision == GLX_KNN_PREC_SPLIT,
              "precision must be GLX_KNN_PREC_F32 (0), GLX_KNN_PREC_HALF (1) or GLX_KNN_PREC_SPLIT (2), got %d", precision);
  if (precision == GLX_KNN_PREC_F32) {
    GLX_REQUIRE(refine == 0, "refine must be 0 with precision GLX_KNN_PREC_F32, got %d", refine);
    GLX_REQUIRE(f->num_rows < INT32_MAX, "num_rows must be < 2^31");
    return knn_search_entry(f->device, f->dim, queries, num_queries, k, ids_out, dist_out, ptr_kind, stream,
                            [&](const float* d_q, int64_t* d_ids, float* d_dist, hipStream_t s) {
                              return knn_search_device(f, metric, d_q, num_queries, k, d_ids, d_dist, s, tile);
                            });
  }
  const bool split = precision == GLX_KNN_PREC_SPLIT;
  if (split) {
    GLX_REQUIRE(f->dtype == GLX_DTYPE_F32, "precision GLX_KNN_PREC_SPLIT needs a float32 table, this one stores %s",
                glx_dtype_name(f->dtype));
    GLX_REQUIRE(tile == GLX_KNN_TILE_WIDE, "tile must be GLX_KNN_TILE_WIDE (0) with precision GLX_KNN_PREC_SPLIT, got %d",
                tile);
  } else {
    GLX_REQUIRE(f->dtype == GLX_DTYPE_BF16 || f->dtype == GLX_DTYPE_F16 || glx_dtype_is_f8(f->dtype),
                "precision GLX_KNN_PREC_HALF needs a bfloat16, float16 or float8 table, this one stores %s",
                glx_dtype_name(f->dtype));
  }
  GLX_REQUIRE(refine == 0 || (refine >= k && refine <= kSortN), "refine must be 0 or in [k = %d, %d], got %d", k, kSortN,
              refine);
  GLX_REQUIRE((int64_t)num_queries * (refine > k ? refine : k) < INT32_MAX, "num_queries * max(k, refine) must be < 2^31");
  GLX_REQUIRE(f->num_rows < INT32_MAX, "num_rows must be < 2^31");
  return knn_search_entry(f->device, f->dim, queries, num_queries, k, ids_out, dist_out, ptr_kind, stream,
                          [&](const float* d_q, int64_t* d_ids, float* d_dist, hipStream_t s) {
                            if (split) return knn_search_split_device(f, metric, d_q, num_queries, k, refine, d_ids, d_dist, s);
                            return knn_search_half_device(f, metric, d_q, num_queries, k, refine, d_ids, d_dist, s, tile);
                          });
}
