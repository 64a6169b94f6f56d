// What the training-path kernels share below any knowledge of segments: the lane-group widths and their dispatch, the
// alignment tests of the vector paths, the product that never contracts, and the float zero-fill of an output nobody
// computes.  The segment layout and the per-segment lane mappings build on it in glx_segment_lanes.h.
#ifndef GLX_LANE_GROUPS_H_
#define GLX_LANE_GROUPS_H_
#include <type_traits>

#include "glx_common.h"

// the smallest group of 8 .. 64 lanes that covers `lanes`
inline int glx_group_for(int64_t lanes) { return lanes <= 8 ? 8 : lanes <= 16 ? 16 : lanes <= 32 ? 32 : 64; }

// f(std::integral_constant<int, G>()) for the G of glx_group_for: a kernel template takes decltype(g)::value
template <typename F>
inline void glx_for_group(int G, F&& f) {
  switch (G) {
    case 8: f(std::integral_constant<int, 8>()); break;
    case 16: f(std::integral_constant<int, 16>()); break;
    case 32: f(std::integral_constant<int, 32>()); break;
    default: f(std::integral_constant<int, 64>()); break;
  }
}

// a float4 / int4 access needs it
inline bool glx_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// a 4-ELEMENT access of a float32 / bfloat16 matrix needs it: 16 bytes for float32, 8 for bfloat16.  Every matrix of
// dim % 4 == 0 from an allocator that hands out 16-byte aligned blocks passes in both types, so a bfloat16 call takes
// the VEC -- and with it the lane-to-column mapping -- the float32 call takes.
inline bool glx_aligned_vec4(const void* p, int dtype) {
  return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(4 * glx_dtype_size(dtype) - 1)) == 0;
}

// the pieces of one workspace lease start on 256-byte boundaries
inline size_t glx_align256(size_t b) { return (b + 255) & ~(size_t)255; }

// Opaque to the optimiser: no instruction, and nothing contracts across it.
__device__ __forceinline__ float glx_pin(float t) {
  asm("" : "+v"(t));
  return t;
}

// acc + w * x in two roundings: the multiply must never contract into the add, whatever -ffp-contract the build passes.
// Neither __fmul_rn / __fadd_rn (plain `x * y` / `x + y` in this toolchain's headers, parsed before any pragma of ours)
// nor `#pragma clang fp contract(off)` alone guarantees that: an explicit -ffp-contract=fast lets the backend fuse any
// multiply with any add.  So the product goes through an empty asm that pins it in a register: the add that follows
// takes an opaque operand and cannot become an FMA under any flag.  The files that fold keep the pragma for the
// front end.
__device__ __forceinline__ float glx_fold_rn(float acc, float w, float x) {
  return acc + glx_pin(w * x);  // the product is rounded, pinned, and the sum rounded again
}

// The list walk of the row gradients (glx_aggregate_grad.hip, glx_aggregate_weighted.hip): a group of G lanes (lane c)
// folds entries [l0, l1) of a transposed list -- a whole row's list in the default order, one chunk of it in the chunked
// order -- into out[0 .. dim), which holds DT elements.  Lane c owns columns [VEC c, VEC c + VEC) of each column tile
// of G * VEC columns.  It fetches list entry base + c (its position, that position's segment and, where the term
// divides, the divisor) and every lane of the group reads entry j from lane j: the group walks its list together, so
// the cross-lane reads stay inside a group whose lanes all run the same iterations.  U term loads are issued before the
// first is folded.  The sum starts at +0.0f and is float32 whatever DT; a bfloat16 `out` rounds the finished sum once,
// in the store (agg_store).  An empty list writes zeros.
// term_of(col) makes the term of one column tile (col: the lane's first column, 0 for a lane past the last one):
//   TERM::kDiv                    does the term divide (Mean)?
//   divisor(seg)                  the divisor of an entry of segment seg, fetched once per entry
//   load(&ld, p, seg)             issues the loads of entry (position p, segment seg) into a TERM::Loaded
//   fold(&acc, ld, p, dv)         adds the entry's term to the VEC accumulators, in one rounding per add
struct GlxPosList {
  const int32_t* pos;     // request positions by (row, position): GlxAggTranspose's
  const int32_t* seg_of;  // segment of a position, or nullptr: position / fanout
  int32_t fanout;
};

template <int G, int VEC, int U, int DT, typename TERM_OF>
__device__ __forceinline__ void glx_list_fold(const GlxPosList& L, int32_t l0, int32_t l1, int c, int32_t dim,
                                              typename AggElem<DT>::raw* out, TERM_OF&& term_of) {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  for (int32_t col_pass = 0; col_pass < dim; col_pass += G * VEC) {
    const int32_t col = col_pass + c * VEC;
    const bool col_ok = col < dim;
    const auto term = term_of(col_ok ? col : 0);  // lanes past the end re-read the first columns, unused
    typedef typename std::remove_const<decltype(term)>::type TERM;
    vec_t acc;
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.0f;
    for (int32_t base = l0; base < l1; base += G) {
      int32_t my_pos = 0, my_seg = 0;
      float my_div = 1.0f;
      if (base + c < l1) {
        my_pos = L.pos[base + c];
        my_seg = L.seg_of ? L.seg_of[my_pos] : my_pos / L.fanout;
        if (TERM::kDiv) my_div = term.divisor(my_seg);
      }
      const int32_t m = (l1 - base) < G ? (l1 - base) : G;
      for (int32_t j = 0; j < m; j += U) {
        int32_t p[U], sg[U];
        float dv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int src = (j + u) & (G - 1);
          p[u] = __shfl(my_pos, src, G);
          sg[u] = __shfl(my_seg, src, G);
          dv[u] = TERM::kDiv ? __shfl(my_div, src, G) : 1.0f;
        }
        typename TERM::Loaded ld[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (j + u < m) term.load(&ld[u], p[u], sg[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (j + u < m) term.fold(&acc, ld[u], p[u], dv[u]);
        }
      }
    }
    if (col_ok) agg_store<DT, VEC>(out + col, acc);  // lanes past the last column store nothing
  }
}

// A gathered row of a table of DT elements (float32, or bfloat16 upcast exactly as it is loaded); an index outside the
// table reads a row of default_attr instead (ok == false: `at` is never read).
template <int DT>
struct GlxRowOf {
  const typename AggElem<DT>::raw* at;
  bool ok;
};
typedef GlxRowOf<GLX_DTYPE_F32> GlxRow;

template <int DT = GLX_DTYPE_F32>
__device__ __forceinline__ GlxRowOf<DT> glx_row(const typename AggElem<DT>::raw* x, int64_t r, int64_t num_rows,
                                                int32_t dim) {
  const bool in = r >= 0 && r < num_rows;
  return GlxRowOf<DT>{x + (in ? r : 0) * (int64_t)dim, in};
}

// VEC columns of it from `col` on, as float32: one load of VEC elements
template <int VEC, int DT>
__device__ __forceinline__ float __attribute__((ext_vector_type(VEC))) glx_row_load(GlxRowOf<DT> row, int32_t col,
                                                                                     float default_attr) {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  vec_t v;
  if (row.ok) {
    v = agg_load<DT, VEC>(row.at + col);
  } else {
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = default_attr;
  }
  return v;
}

// The per-head dot products of two rows of `dim` = heads * C columns by a group of G lanes (lane c): out[h] = the sum
// over the columns of head h of ra[col] * rb[col], divided by `div` when DIV (Mean).  The lane-to-column mapping and
// the cross-lane tree are fixed by (dim, heads, alignment) alone, so the same inputs give the same bits on every run.
//   SUB  (L = C / VEC is a power of two)  lane c owns columns [VEC c, VEC c + VEC) of each tile of G * VEC columns; a
//        head is a sub-group of min(L, G) consecutive lanes (times L / G tiles when L > G), reduced with __shfl_xor
//        over the sub-group; its first lane writes.
//   !SUB a loop over the heads: lane c owns elements c, c + G, .. of the head's L vectors, the whole group reduces,
//        lane 0 writes.
// hd: glx_head_dot_plan's, for the same G and VEC.  Every lane of the group calls it.
struct GlxHeadDots {
  int32_t sub;    // SUB: lanes of a sub-group (min(C / VEC, G))
  int32_t steps;  // SUB: column tiles a head spans (C / VEC / G, at least 1)
};

// la(col) / lb(col): the VEC columns of either operand from `col` on -- a gathered row, or anything computed from one.
template <int G, int VEC, bool SUB, bool DIV, typename LA, typename LB>
__device__ __forceinline__ void glx_head_dots_of(LA&& la, LB&& lb, int32_t dim, int32_t heads, int32_t C, GlxHeadDots hd,
                                                 float div, int c, float* out) {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  if (SUB) {
    const int32_t span = G * VEC * hd.steps;  // columns per reduce: G / sub whole heads, or one
    for (int32_t col_pass = 0; col_pass < dim; col_pass += span) {
      float part = 0.0f;
      for (int32_t k = 0; k < hd.steps; ++k) {
        const int32_t col = col_pass + (k * G + c) * VEC;
        if (col < dim) {
          const vec_t u = la(col);
          const vec_t w = lb(col);
#pragma unroll
          for (int v = 0; v < VEC; ++v) part += u[v] * w[v];
        }
      }
      for (int off = hd.sub >> 1; off > 0; off >>= 1) part += __shfl_xor(part, off, G);
      const int32_t col0 = col_pass + c * VEC;
      if ((c & (hd.sub - 1)) == 0 && col0 < dim) out[col0 / C] = DIV ? part / div : part;
    }
  } else {
    const int32_t L = C / VEC;
    for (int32_t h = 0; h < heads; ++h) {
      float part = 0.0f;
      for (int32_t i = c; i < L; i += G) {
        const int32_t col = h * C + i * VEC;
        const vec_t u = la(col);
        const vec_t w = lb(col);
#pragma unroll
        for (int v = 0; v < VEC; ++v) part += u[v] * w[v];
      }
#pragma unroll
      for (int off = G >> 1; off > 0; off >>= 1) part += __shfl_xor(part, off, G);
      if (c == 0) out[h] = DIV ? part / div : part;
    }
  }
}

// the two operands are gathered rows, each of its own element type
template <int G, int VEC, bool SUB, bool DIV, int DTA, int DTB>
__device__ __forceinline__ void glx_head_dots(GlxRowOf<DTA> ra, GlxRowOf<DTB> rb, float default_attr, int32_t dim,
                                              int32_t heads, int32_t C, GlxHeadDots hd, float div, int c, float* out) {
  glx_head_dots_of<G, VEC, SUB, DIV>([&](int32_t col) { return glx_row_load<VEC>(ra, col, default_attr); },
                                     [&](int32_t col) { return glx_row_load<VEC>(rb, col, default_attr); }, dim, heads,
                                     C, hd, div, c, out);
}

// The host side of glx_head_dots for rows of `dim` columns, C to a head, read VEC at a time: which mapping, the group
// width and the sub-group shape.  SUB's sub-groups tile the row, so the group covers all of it (up to 64 lanes); the
// loop over heads takes a group that covers one head.
struct GlxHeadDotPlan {
  bool sub_groups;  // the kernel's SUB
  int G;
  GlxHeadDots hd;
};

inline GlxHeadDotPlan glx_head_dot_plan(int32_t dim, int32_t C, int VEC) {
  const int L = C / VEC;
  GlxHeadDotPlan p;
  p.sub_groups = (L & (L - 1)) == 0;
  p.G = glx_group_for(p.sub_groups ? dim / VEC : L);
  p.hd.sub = p.sub_groups ? (L < p.G ? L : p.G) : 1;
  p.hd.steps = p.sub_groups && L > p.G ? L / p.G : 1;
  return p;
}

// +0.0 into `count` ELEMENTS of a float32 / bfloat16 output that no kernel will write (all bits clear is +0.0 in both;
// the bytes are the buffer's own: a bfloat16 buffer has half of float32's); nothing to do for an absent or empty one
inline int glx_zero_elems_async(void* p, size_t count, int dtype, hipStream_t s) {
  if (p == nullptr || count == 0) return GLX_OK;
  hipError_t e = hipMemsetAsync(p, 0, count * (size_t)glx_dtype_size(dtype), s);
  if (e != hipSuccess) {
    glx_set_error("hipMemsetAsync failed: %s", hipGetErrorString(e));
    return GLX_INTERNAL;
  }
  return GLX_OK;
}
inline int glx_zero_f32_async(float* p, size_t count, hipStream_t s) {
  return glx_zero_elems_async(p, count, GLX_DTYPE_F32, s);
}

// f(std::integral_constant<int, DT>()) for the two element types of the training path (GLX_REQUIRE_TRAIN_DTYPE has
// passed): a kernel template takes decltype(t)::value
template <typename F>
inline void glx_for_train_dtype(int dtype, F&& f) {
  if (dtype == GLX_DTYPE_BF16) f(std::integral_constant<int, GLX_DTYPE_BF16>());
  else f(std::integral_constant<int, GLX_DTYPE_F32>());
}

#endif  // GLX_LANE_GROUPS_H_
