// glx fused dot-product attention over the segments of a counts= request, with an edge term on the key and on the
// value, and its gradients: the logit of every (neighbour, head), the softmax over each segment, dropout on the
// coefficients and the weighted sum of the value rows in one kernel going forward, one per-segment kernel going back.
// The layer of the reference's GPU PyTorch model: TransformerConv(in, out // 2, heads=2, dropout=0.1, edge_dim=...)
// (graphlearn/examples/pytorch/tgn/train_and_eval.py:38-50).
//
// Contract (include/glx.h).  Segments as in glx_aggregate_weighted.  For a consumed position
// p of segment sg, head h and a column c of it (C = dim / heads columns to a head):
//   rows      kk(p)[c] = krow(p)[c] (+ edge[p, c] in one float32 add when edge is given), vv(p)[c] the same from v; a
//             row outside [0, num_rows) reads default_attr in both tables
//   logit     dot[p, h] = sum_c q[sg, c] * kk(p)[c] (glx_pair_dot's tolerance contract: the order is the mapping's);
//             e = fmul_rn(dot, scale)
//   softmax   soft = expf(e - max) / sum, glx_segment_softmax's definition, bound and exact rules
//   dropout   glx_gat_attention's, element i = p * heads + h: alpha = keep ? soft * dropscale : +0.0f
//   out       out[sg, c] = +0.0f, then fadd_rn(out, fmul_rn(alpha[p, h], vv(p)[c])) in ascending p: bit-exact, so no
//             online-softmax rescale; the k rows are read in the logit pass, the v rows in this one, each once
//   backward  ga = keep ? (sum_c grad_out[sg, c] * vv(p)[c]) * dropscale : +0.0f;
//             d = soft * (ga - sum_q soft_q * ga_q); grad_e = fmul_rn(d, scale);
//             grad_q[sg, c] = +0.0f, then fadd_rn(., fmul_rn(grad_e[p, h], kk(p)[c])) in ascending p;
//             grad_edge[p, c] = fadd_rn(fmul_rn(grad_e[p, h], q[sg, c]), fmul_rn(alpha[p, h], grad_out[sg, c]));
//             grad_k / grad_v: glx_aggregate_weighted_backward_x(Sum) with (w, grad_out) = (grad_e, q) /
//             (alpha, grad_out), on one transpose
// One lane group per segment, of any length: a hub segment is walked by its one group.  EVERY element of every output
// that is asked for is written; a position that is not consumed gets +0.0f, an empty segment +0.0f in every column.
// No float atomics: the lane mapping and the trees are fixed, so the same inputs give the same bits on every call.
//
// The CHUNKED order (K5-dot-attn-chunked: glx_dot_attention_chunked, glx_dot_attention_backward_chunked; opt-in).  A
// segment of more than GLX_COALESCE_CHUNK = 256 positions is LONG and is cut into chunks of 256 positions; every other
// segment goes through the kernels above, restricted to short segments, and keeps the default order's bits.  The chunk
// directory is glx_chunks.h's, over the SEGMENTS (GlxSegLists).  Then, per direction:
//   pass       one lane group per chunk: the dot products of its positions (the logits' / ga_raw), by the default
//              order's own dot_pass, so logit_out has the default's bits
//   normalise  one workgroup per long segment (SmBlockWalker): the softmax / its gradient in a fixed tree over the
//              256 threads -- the definition, exact rules and bound of K5-sm, other bits than one lane group's tree
//   fold       one lane group per chunk: partial_j = +0.0f, then the chunk's terms in ascending p (backward: grad_q's
//              terms, and the chunk's rows of grad_edge)
//   combine    one lane group per long segment: +0.0f, then one fadd_rn per partial in ascending j
//              (glx_chunks_combine)
// A chunk's passes meet across kernel boundaries; inside a kernel a group still lies in one wavefront.  grad_k / grad_v
// are the chunked row gradient as it stands (glx_weighted_bwd_x, chunked).
#include <math.h>

#include "glx_chunks.h"

// Two roundings per term of the folds: glx_fold_rn (glx_lane_groups.h) pins the product; the pragma is for the front
// end.
#pragma clang fp contract(off)

namespace {

constexpr int kWU = 4;  // row loads in flight per lane

struct DotArgs {
  const float* q;          // [num_segments, dim]
  const float* k;          // [num_rows, dim]
  const float* v;          // [num_rows, dim]
  const int64_t* rows;     // [num_ids]
  const float* edge;       // [num_ids, dim], or nullptr
  GlxSegLayout seg;
  const float* soft;       // backward: the forward's softmax                      [num_ids, heads]
  const float* grad_out;   // backward                                             [num_segments, dim]
  const float* w;          // the accumulate passes' alpha: `alpha` under dropout, soft otherwise
  float* alpha;            // dropout only: alpha, in the workspace                [num_ids, heads]
  float* logit;            // forward: logit_out, or nullptr
  float* soft_out;         // forward
  float* out;              // forward                                              [num_segments, dim]
  float* grad_e;           // backward                                             [num_ids, heads]
  float* grad_q;           // backward: [num_segments, dim], or nullptr
  float* grad_edge;        // backward: [num_ids, dim], or nullptr
  int64_t num_rows;
  int32_t dim, heads, C;
  GlxHeadDots hd;
  float scale, default_attr;
  int32_t drop;            // drop_p != 0
  SmDropout dropout;
};

// Between two passes of a segment the lanes of a group hand values to EACH OTHER through global memory (logit_out /
// soft_out / grad_e / alpha): plain stores by one lane, plain loads of the same address by another -- unlike K5-sm and
// K5-gat, where a lane only re-reads what it wrote itself.  What makes that sound is an invariant of the mapping, not
// of the memory model: a group never spans a wavefront (G <= 64 lanes, 64 % G == 0, groups aligned to G), so writer and
// reader execute the same instructions in lock step; the workgroup-scope fence keeps the compiler from moving accesses
// across it and drains the wavefront's stores (s_waitcnt vmcnt(0)) before its loads issue; and the loads go through the
// L1 of the CU the stores went through (the default, non-tgsplit mode: a wavefront never leaves its CU).  Both kernels
// assert the first condition through this function.
template <int G>
__device__ __forceinline__ void dot_handoff() {
  static_assert(G <= 64 && 64 % G == 0, "a lane group must lie inside one wavefront: its lanes hand over in memory");
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
}

__device__ __forceinline__ float dot_drop(const DotArgs& a, float x, int32_t idx) {
  return a.drop ? sm_dropout(x, idx, a.dropout) : x;
}

// the row of position base + c, tested against the table: -1 reads default_attr
__device__ __forceinline__ int32_t dot_my_row(const DotArgs& a, int32_t p, int32_t s1) {
  if (p >= s1) return -1;
  const int64_t r = a.rows[p];
  return (r >= 0 && r < a.num_rows) ? (int32_t)r : -1;
}

// VEC columns of kk(p) or vv(p) from `col` on: the table row (or default_attr) plus the edge row in one float32 add
template <int VEC>
__device__ __forceinline__ float __attribute__((ext_vector_type(VEC))) dot_row_vec(const DotArgs& a, const float* tab,
                                                                                    int32_t row, int32_t p,
                                                                                    int32_t col) {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  vec_t x;
  if (row >= 0) {
    x = *reinterpret_cast<const vec_t*>(tab + row * (int64_t)a.dim + col);
  } else {
#pragma unroll
    for (int t = 0; t < VEC; ++t) x[t] = a.default_attr;
  }
  if (a.edge) x = x + *reinterpret_cast<const vec_t*>(a.edge + p * (int64_t)a.dim + col);
  return x;
}

// dst[p, 0 .. heads) = glx_head_dots of the segment's own row `fix` with kk(p) / vv(p) (tab = k / v), p = s0 .. s1.
// Lane c fetches the row of position base + c and every lane reads entry j from lane j.
template <int G, int VEC, bool SUB>
__device__ __forceinline__ void dot_pass(const DotArgs& a, const float* fix, const float* tab, int32_t s0, int32_t s1,
                                         int c, float* dst) {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  for (int32_t base = s0; base < s1; base += G) {
    const int32_t my_row = dot_my_row(a, base + c, s1);
    const int32_t m = (s1 - base) < G ? (s1 - base) : G;
    for (int32_t j = 0; j < m; ++j) {
      const int32_t row = __shfl(my_row, j, G);
      const int32_t p = base + j;
      glx_head_dots_of<G, VEC, SUB, false>([&](int32_t col) { return *reinterpret_cast<const vec_t*>(fix + col); },
                                           [&](int32_t col) { return dot_row_vec<VEC>(a, tab, row, p, col); }, a.dim,
                                           a.heads, a.C, a.hd, 1.0f, c, dst + (int64_t)p * a.heads);
    }
  }
}

// What sm_forward / sm_backward (glx_segment_lanes.h) read and write here.  Forward: lg holds the dot products
// (logit_out, or soft_out when the caller wants no logits); a register item writes its logit only when logit_out is
// given, a spilled one parks it in lg, then its exponential in soft_out.  Backward: grad_e holds ga_raw on entry and
// grad_e on exit.  Both restate alpha for the passes that follow.
struct DotIo {
  const DotArgs& a;
  const SmItems& it;
  float* lg;
  static constexpr bool kSum = false;
  __device__ __forceinline__ float logit(int32_t i) const {
    const int32_t at = it.idx(i);
    const float e = glx_pin(lg[at] * a.scale);
    if (a.logit) a.logit[at] = e;
    return e;
  }
  __device__ __forceinline__ float spill_logit(int32_t i) const {
    const int32_t at = it.idx(i);
    return lg[at] = glx_pin(lg[at] * a.scale);
  }
  __device__ __forceinline__ float parked_logit(int32_t i) const { return lg[it.idx(i)]; }
  __device__ __forceinline__ void park_exp(int32_t i, float t) const { a.soft_out[it.idx(i)] = t; }
  __device__ __forceinline__ float parked_exp(int32_t i) const { return a.soft_out[it.idx(i)]; }
  __device__ __forceinline__ void emit_soft(int32_t i, float soft) const {
    const int32_t at = it.idx(i);
    a.soft_out[at] = soft;
    if (a.drop) a.alpha[at] = dot_drop(a, soft, at);
  }
  __device__ __forceinline__ float soft(int32_t i) const { return a.soft[it.idx(i)]; }
  __device__ __forceinline__ float grad(int32_t i) const {
    const int32_t at = it.idx(i);
    return dot_drop(a, a.grad_e[at], at);
  }
  __device__ __forceinline__ float emit_grad(int32_t i, float soft, float d) const {
    const int32_t at = it.idx(i);
    a.grad_e[at] = glx_pin(d) * a.scale;
    if (a.drop) a.alpha[at] = dot_drop(a, soft, at);
    return 0.0f;
  }
};

// The normalisation of a segment by its one group, whatever its length: glx_segment_softmax's two mappings chosen at
// run time (flat: heads a power of two <= G).
template <int G, bool BWD>
__device__ __forceinline__ void dot_normalise(const DotArgs& a, int32_t s0, int32_t s1, int c, float* lg) {
  const SmGroupWalker<G> w = {c};
  SmItems it = sm_items((a.heads & (a.heads - 1)) == 0 && a.heads <= G, s0, s1, a.heads);
  for (it.o = 0; it.o < it.outer; ++it.o) {
    if (BWD) sm_backward(w, it, DotIo{a, it, lg});
    else sm_forward(w, it, DotIo{a, it, lg});
  }
}

// +0.0f into the positions nobody consumed, shared by all the workgroups: `width` floats per position
__device__ __forceinline__ void dot_zero_tail(const GlxSegLayout& seg, float* p, int32_t width) {
  if (p == nullptr) return;
  const int64_t end = (int64_t)seg.num_ids * width;
  const int64_t first = seg_tail(seg) * width + blockIdx.x * 256LL + threadIdx.x;
  for (int64_t i = first; i < end; i += gridDim.x * 256LL) p[i] = 0.0f;
}

// dst[0 .. dim) = +0.0f, then fadd_rn(., fmul_rn(w[p, h], vv(p)[c])) over positions [s0, s1) in ascending p: lane c
// owns columns [VEC c, VEC c + VEC) of each column tile of G * VEC columns.  The walk is repeated per column tile: for
// dim > G * VEC (512 columns at float4, or 100 read float by float) the rows indices, their shuffles and the alpha
// loads are repeated per tile -- [n, H]-sized traffic, small beside the rows, and one tile at the tested and measured
// shapes (dim <= 256 at float4).  An empty range writes +0.0f.
template <int G, int VEC>
__device__ __forceinline__ void dot_fold_out(const DotArgs& a, int32_t s0, int32_t s1, int c, float* dst) {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  for (int32_t col_pass = 0; col_pass < a.dim; col_pass += G * VEC) {
    const int32_t col = col_pass + c * VEC;
    const bool col_ok = col < a.dim;
    const int32_t col_ld = col_ok ? col : 0;  // lanes past the end re-read the first columns, unused
    const int32_t head = col_ld / a.C;
    vec_t acc;
#pragma unroll
    for (int t = 0; t < VEC; ++t) acc[t] = 0.0f;
    for (int32_t base = s0; base < s1; base += G) {
      const int32_t my_row = dot_my_row(a, base + c, s1);
      const int32_t m = (s1 - base) < G ? (s1 - base) : G;
      for (int32_t j = 0; j < m; j += kWU) {
        int32_t row[kWU];
#pragma unroll
        for (int u = 0; u < kWU; ++u) row[u] = __shfl(my_row, (j + u) & (G - 1), G);
        vec_t val[kWU];
        float wt[kWU];
#pragma unroll
        for (int u = 0; u < kWU; ++u) {
          if (j + u < m) {
            wt[u] = a.w[(int64_t)(base + j + u) * a.heads + head];
            val[u] = dot_row_vec<VEC>(a, a.v, row[u], base + j + u, col_ld);
          }
        }
#pragma unroll
        for (int u = 0; u < kWU; ++u) {
          if (j + u < m) {
#pragma unroll
            for (int t = 0; t < VEC; ++t) acc[t] = glx_fold_rn(acc[t], wt[u], val[u][t]);
          }
        }
      }
    }
    if (col_ok) *reinterpret_cast<vec_t*>(dst + col) = acc;  // an empty range: +0.0f
  }
}

// One pass over kk(p), p = s0 .. s1 of segment sg: gq[0 .. dim) (unless nullptr) = +0.0f, then
// fadd_rn(., fmul_rn(grad_e[p, h], kk(p)[c])) in ascending p, and the rows [s0, s1) of grad_edge when it is asked for.
// dot_fold_out's lane mapping.
template <int G, int VEC>
__device__ __forceinline__ void dot_fold_back(const DotArgs& a, int64_t sg, int32_t s0, int32_t s1, int c, float* gq) {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  const float* const go = a.grad_out + sg * (int64_t)a.dim;
  const float* const qr = a.q + sg * (int64_t)a.dim;
  for (int32_t col_pass = 0; col_pass < a.dim; col_pass += G * VEC) {
    const int32_t col = col_pass + c * VEC;
    const bool col_ok = col < a.dim;
    const int32_t col_ld = col_ok ? col : 0;  // lanes past the end re-read the first columns, unused
    const int32_t head = col_ld / a.C;
    const vec_t qv = *reinterpret_cast<const vec_t*>(qr + col_ld);
    const vec_t gov = *reinterpret_cast<const vec_t*>(go + col_ld);
    vec_t acc;
#pragma unroll
    for (int t = 0; t < VEC; ++t) acc[t] = 0.0f;
    for (int32_t base = s0; base < s1; base += G) {
      const int32_t my_row = gq ? dot_my_row(a, base + c, s1) : -1;
      const int32_t m = (s1 - base) < G ? (s1 - base) : G;
      for (int32_t j = 0; j < m; j += kWU) {
        int32_t row[kWU];
#pragma unroll
        for (int u = 0; u < kWU; ++u) row[u] = __shfl(my_row, (j + u) & (G - 1), G);
        vec_t val[kWU];
        float ge[kWU], al[kWU];
#pragma unroll
        for (int u = 0; u < kWU; ++u) {
          if (j + u < m) {
            const int64_t at = (int64_t)(base + j + u) * a.heads + head;
            ge[u] = a.grad_e[at];
            if (a.grad_edge) al[u] = a.w[at];
            if (gq) val[u] = dot_row_vec<VEC>(a, a.k, row[u], base + j + u, col_ld);
          }
        }
#pragma unroll
        for (int u = 0; u < kWU; ++u) {
          if (j + u < m) {
            if (gq) {
#pragma unroll
              for (int t = 0; t < VEC; ++t) acc[t] = glx_fold_rn(acc[t], ge[u], val[u][t]);
            }
            if (a.grad_edge && col_ok) {
              vec_t d;
#pragma unroll
              for (int t = 0; t < VEC; ++t) d[t] = glx_pin(ge[u] * qv[t]) + glx_pin(al[u] * gov[t]);
              *reinterpret_cast<vec_t*>(a.grad_edge + (base + j + u) * (int64_t)a.dim + col) = d;
            }
          }
        }
      }
    }
    if (gq && col_ok) *reinterpret_cast<vec_t*>(gq + col) = acc;
  }
}

// G lanes own one segment, a workgroup 256 / G consecutive segments.  Three passes, each by the whole group: the
// logits (one glx_head_dots per position over q and kk), the normalisation, and glx_aggregate_weighted's fold over
// alpha and vv (dot_fold_out).  SHORT (the chunked order): a segment of more than kGlxChunk positions is left to the
// chunk kernels below; every other segment gets exactly what the default order gives it.
template <int G, int VEC, bool SUB, bool SHORT>
__global__ __launch_bounds__(256) void glx_dot_attention_kernel(DotArgs a) {
  const int64_t sg = blockIdx.x * (int64_t)(256 / G) + threadIdx.x / G;
  const int c = threadIdx.x & (G - 1);
  int32_t s0 = 0, s1 = 0;
  bool mine = sg < a.seg.num_segments;  // the same answer in every lane of the group
  if (mine) {
    seg_bounds(a.seg, sg, &s0, &s1);
    if (SHORT) mine = s1 - s0 <= kGlxChunk;
  }
  if (mine) {
    if (s1 > s0) {
      float* const lg = a.logit ? a.logit : a.soft_out;
      dot_pass<G, VEC, SUB>(a, a.q + sg * (int64_t)a.dim, a.k, s0, s1, c, lg);
      dot_handoff<G>();
      dot_normalise<G, false>(a, s0, s1, c, lg);
      dot_handoff<G>();
    }
    dot_fold_out<G, VEC>(a, s0, s1, c, a.out + sg * (int64_t)a.dim);
  }
  dot_zero_tail(a.seg, a.logit, a.heads);
  dot_zero_tail(a.seg, a.soft_out, a.heads);
}

// The same mapping going back: ga_raw (one glx_head_dots per position over grad_out and vv, parked in grad_e), the
// softmax gradient in a fixed tree, then one pass over kk that folds grad_q and writes the rows of grad_edge
// (dot_fold_back).  SHORT as above.
template <int G, int VEC, bool SUB, bool SHORT>
__global__ __launch_bounds__(256) void glx_dot_attention_bwd_kernel(DotArgs a) {
  const int64_t sg = blockIdx.x * (int64_t)(256 / G) + threadIdx.x / G;
  const int c = threadIdx.x & (G - 1);
  int32_t s0 = 0, s1 = 0;
  bool mine = sg < a.seg.num_segments;  // the same answer in every lane of the group
  if (mine) {
    seg_bounds(a.seg, sg, &s0, &s1);
    if (SHORT) mine = s1 - s0 <= kGlxChunk;
  }
  if (mine) {
    if (s1 > s0) {
      dot_pass<G, VEC, SUB>(a, a.grad_out + sg * (int64_t)a.dim, a.v, s0, s1, c, a.grad_e);
      dot_handoff<G>();
      dot_normalise<G, true>(a, s0, s1, c, nullptr);
      dot_handoff<G>();
    }
    if (a.grad_q || a.grad_edge) {
      dot_fold_back<G, VEC>(a, sg, s0, s1, c, a.grad_q ? a.grad_q + sg * (int64_t)a.dim : nullptr);
    }
  }
  dot_zero_tail(a.seg, a.grad_e, a.heads);
  dot_zero_tail(a.seg, a.grad_edge, a.dim);
}

// ---- the chunked order ----------------------------------------------------------------------------------------
// The chunk directory (glx_chunks.h) is over the SEGMENTS, GlxSegLists{a.seg}: a work item is a chunk of a long
// segment's positions, its partial sum a row of out or grad_q.

// the segment of work item t and the positions [*c0, *c1) of its chunk (glx_chunk_of); false: t is past the directory
__device__ __forceinline__ bool dot_chunk_of(const DotArgs& a, const GlxChunkDir& ch, int64_t t, int32_t* sg,
                                             int32_t* c0, int32_t* c1) {
  if (GLX_CHUNK_IDLE(ch, t)) return false;
  glx_chunk_of(ch, GlxSegLists{a.seg}, t, sg, c0, c1);
  return true;
}

// G lanes own work item t: the dot products of its chunk's positions, where the per-segment kernels park theirs (the
// logits' in logit_out or soft_out; ga_raw in grad_e).  Whole groups leave past the directory.
template <int G, int VEC, bool SUB, bool BWD>
__global__ __launch_bounds__(256) void glx_dot_chunk_pass_kernel(DotArgs a, GlxChunkDir ch) {
  const int64_t t = blockIdx.x * (int64_t)(256 / G) + threadIdx.x / G;
  const int c = threadIdx.x & (G - 1);
  int32_t sg, c0, c1;
  if (!dot_chunk_of(a, ch, t, &sg, &c0, &c1)) return;
  if (BWD) dot_pass<G, VEC, SUB>(a, a.grad_out + sg * (int64_t)a.dim, a.v, c0, c1, c, a.grad_e);
  else dot_pass<G, VEC, SUB>(a, a.q + sg * (int64_t)a.dim, a.k, c0, c1, c, a.logit ? a.logit : a.soft_out);
}

// The workgroup owns work item t and leaves unless it is the first of its segment: the normalisation of one long
// segment by 256 threads, K5-sm's long-segment walk.  A thread parks and reads back its own items only; what the pass
// kernel wrote arrived with the kernel boundary.  Every condition is the same in all 256 threads.
template <bool BWD>
__global__ __launch_bounds__(256) void glx_dot_chunk_norm_kernel(DotArgs a, GlxChunkDir ch) {
  __shared__ float red[256];
  const int64_t t = blockIdx.x;
  if (GLX_CHUNK_IDLE(ch, t)) return;
  const int32_t sg = ch.item_list[t];
  if (!GLX_CHUNK_FIRST(ch, t, sg)) return;
  int32_t s0, s1;
  seg_bounds(a.seg, sg, &s0, &s1);
  const SmBlockWalker w = {red};
  float* const lg = a.logit ? a.logit : a.soft_out;
  SmItems it = sm_items((a.heads & (a.heads - 1)) == 0 && a.heads <= 64, s0, s1, a.heads);
  for (it.o = 0; it.o < it.outer; ++it.o) {
    if (BWD) sm_backward(w, it, DotIo{a, it, nullptr});
    else sm_forward(w, it, DotIo{a, it, lg});
  }
}

// G lanes own work item t: the fold of its chunk into the item's partial sum, by the per-segment kernels' own walk
// (backward: grad_q's terms -- unless grad_q is not asked for -- and the chunk's rows of grad_edge).
template <int G, int VEC, bool BWD>
__global__ __launch_bounds__(256) void glx_dot_chunk_fold_kernel(DotArgs a, GlxChunkDir ch) {
  const int64_t t = blockIdx.x * (int64_t)(256 / G) + threadIdx.x / G;
  const int c = threadIdx.x & (G - 1);
  int32_t sg, c0, c1;
  if (!dot_chunk_of(a, ch, t, &sg, &c0, &c1)) return;
  float* const part = ch.partial + t * (int64_t)a.dim;
  if (BWD) dot_fold_back<G, VEC>(a, sg, c0, c1, c, a.grad_q ? part : nullptr);
  else dot_fold_out<G, VEC>(a, c0, c1, c, part);
}

// ch == nullptr: the default order, one launch; otherwise the chunked one over that directory
template <bool BWD, int VEC>
void dot_launch_vec(DotArgs a, const GlxChunkDir* ch, hipStream_t s) {
  const GlxHeadDotPlan plan = glx_head_dot_plan(a.dim, a.C, VEC);
  const int G = plan.G;
  a.hd = plan.hd;
  // 256 / G segments to a workgroup, and enough workgroups for a tail nobody consumed
  const unsigned blocks = sm_blocks(G, BWD && a.grad_edge ? a.dim : a.heads, a.seg.num_ids, a.seg.num_segments);
  glx_for_group(G, [&](auto g) {
    constexpr int kG = decltype(g)::value;
    const auto launch = [&](auto sub) {
      constexpr bool kSub = decltype(sub)::value;
      if (ch == nullptr) {
        if (BWD) glx_dot_attention_bwd_kernel<kG, VEC, kSub, false><<<blocks, 256, 0, s>>>(a);
        else glx_dot_attention_kernel<kG, VEC, kSub, false><<<blocks, 256, 0, s>>>(a);
        return;
      }
      if (BWD) glx_dot_attention_bwd_kernel<kG, VEC, kSub, true><<<blocks, 256, 0, s>>>(a);
      else glx_dot_attention_kernel<kG, VEC, kSub, true><<<blocks, 256, 0, s>>>(a);
      const unsigned cblocks = (unsigned)(((int64_t)ch->max_items + (256 / kG) - 1) / (256 / kG));
      glx_dot_chunk_pass_kernel<kG, VEC, kSub, BWD><<<cblocks, 256, 0, s>>>(a, *ch);
      glx_dot_chunk_norm_kernel<BWD><<<(unsigned)ch->max_items, 256, 0, s>>>(a, *ch);
      if (!BWD || a.grad_q || a.grad_edge) glx_dot_chunk_fold_kernel<kG, VEC, BWD><<<cblocks, 256, 0, s>>>(a, *ch);
    };
    if (plan.sub_groups) launch(std::true_type());
    else launch(std::false_type());
  });
  if (ch != nullptr && (!BWD || a.grad_q)) {
    glx_chunks_combine(*ch, BWD ? a.grad_q : a.out, GLX_DTYPE_F32, a.dim, VEC == 4, s);
  }
}

// float4 row accesses when every row pointer allows them and a lane's four columns share a head
template <bool BWD>
void dot_launch(const DotArgs& a, const GlxChunkDir* ch, hipStream_t s) {
  bool vec4 = a.C % 4 == 0 && glx_aligned16(a.q) && glx_aligned16(a.k) && glx_aligned16(a.v) && glx_aligned16(a.edge);
  if (BWD) vec4 = vec4 && glx_aligned16(a.grad_out) && glx_aligned16(a.grad_q) && glx_aligned16(a.grad_edge);
  else vec4 = vec4 && glx_aligned16(a.out);
  if (vec4) dot_launch_vec<BWD, 4>(a, ch, s);
  else dot_launch_vec<BWD, 1>(a, ch, s);
}

}  // namespace

// what the two entry points check alike, before any device use
#define GLX_DOT_ATTENTION_REQUIRE()                                                                             \
  GLX_REQUIRE(num_ids >= 0 && num_segments >= 0 && num_rows >= 0, "negative sizes");                            \
  GLX_REQUIRE(dim > 0, "dim must be positive, got %d", dim);                                                    \
  GLX_REQUIRE(heads >= 1, "heads must be positive, got %d", heads);                                             \
  GLX_REQUIRE(dim % heads == 0, "dim %d is not a multiple of heads %d", dim, heads);                            \
  GLX_REQUIRE(num_rows < INT32_MAX, "num_rows must be < 2^31");                                                 \
  GLX_REQUIRE((int64_t)num_ids * heads <= INT32_MAX, "num_ids * heads exceeds int32");                          \
  GLX_REQUIRE((int64_t)num_segments * dim <= INT32_MAX, "num_segments * dim exceeds int32");                    \
  GLX_REQUIRE(isfinite(scale), "scale must be finite");                                                         \
  GLX_REQUIRE(drop_p >= 0.0f && drop_p < 1.0f, "drop_p must lie in [0, 1)");                                    \
  GLX_REQUIRE(ptr_kind == GLX_PTR_HOST || ptr_kind == GLX_PTR_DEVICE, "bad ptr_kind");                          \
  GLX_REQUIRE(cnt != nullptr || num_segments == 0 || num_ids % num_segments == 0,                               \
              "cnt == NULL means equal segments: num_ids must be a multiple of num_segments");                  \
  GLX_REQUIRE(num_ids == 0 || rows != nullptr, "rows is NULL");                                                 \
  GLX_REQUIRE(num_segments == 0 || q != nullptr, "q is NULL");                                                  \
  GLX_REQUIRE(num_rows == 0 || (k != nullptr && v != nullptr), "k or v is NULL")

// The segment directory and the partial sums of one request: a lease of slot kSlotSegChunks (GlxTrainSlot,
// glx_chunks.h, which also says where alpha lives)
static int dot_chunk_dir(const GlxSegLayout& seg, int32_t dim, hipStream_t s, GlxScratch* lease, GlxChunkDir* out) {
  return glx_chunk_dir(GlxSegLists{seg}, seg.num_segments, seg.num_ids, dim, kSlotSegChunks,
                       "chunked dot attention: scan the long segments' chunk counts", s, lease, out);
}

// the body of glx_dot_attention (chunked == false: its launches, its bits) and of glx_dot_attention_chunked
static int dot_attention_forward(bool chunked, int device, const float* q, const float* k, const float* v,
                                 int64_t num_rows, int32_t dim, int32_t heads, const int64_t* rows, const float* edge,
                                 const int32_t* cnt, int32_t num_ids, int32_t num_segments, float scale,
                                 float default_attr, float drop_p, uint64_t seed, uint64_t call, float* logit_out,
                                 float* soft_out, float* out, int ptr_kind, void* stream) {
  GLX_DOT_ATTENTION_REQUIRE();
  GLX_REQUIRE(num_ids == 0 || soft_out != nullptr, "soft_out is NULL");
  GLX_REQUIRE(num_segments == 0 || out != nullptr, "out is NULL");
  int rc = glx_init_device(device);
  if (rc != GLX_OK) return rc;
  if (num_ids == 0 && num_segments == 0) return GLX_OK;
  GlxDeviceGuard guard(device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", device);
  GlxHostStage st(device, ptr_kind, stream, GlxHostStage::ADMIT);
  DotArgs a;
  const int32_t* d_cnt;
  const size_t count = (size_t)num_ids * heads, out_count = (size_t)num_segments * dim;
  st.in(&a.q, q, out_count);
  st.in(&a.k, k, (size_t)num_rows * dim);
  if (v != k) st.in(&a.v, v, (size_t)num_rows * dim);
  st.in(&a.rows, rows, (size_t)num_ids);
  st.in(&a.edge, edge, (size_t)num_ids * dim);
  st.in(&d_cnt, cnt, (size_t)num_segments);
  st.out(&a.logit, logit_out, count);
  st.out(&a.soft_out, soft_out, count);
  st.out(&a.out, out, out_count);
  rc = st.begin();
  if (v == k) a.v = a.k;  // one table: staged once
  GlxScratch lease, alpha, chunk_lease;
  GlxChunkDir chunks;
  if (rc == GLX_OK) {
    if (num_ids == 0 || num_segments == 0) {  // nothing was consumed: empty segments, positions of no segment
      rc = glx_zero_f32_async(a.out, out_count, st.s);
      if (rc == GLX_OK) rc = glx_zero_f32_async(a.soft_out, count, st.s);
      if (rc == GLX_OK) rc = glx_zero_f32_async(a.logit, count, st.s);
    } else {
      rc = glx_seg_layout(cnt ? d_cnt : nullptr, num_ids, num_segments, st.s, &lease, &a.seg);
      if (rc == GLX_OK && drop_p != 0.0f) {
        rc = alpha.alloc(count * sizeof(float), st.s, chunked ? kSlotAlphaChunked : kSlotAlpha);
      }
      if (rc == GLX_OK && chunked) rc = dot_chunk_dir(a.seg, dim, st.s, &chunk_lease, &chunks);
      if (rc == GLX_OK) {
        a.num_rows = num_rows;
        a.dim = dim;
        a.heads = heads;
        a.C = dim / heads;
        a.scale = scale;
        a.default_attr = default_attr;
        a.drop = drop_p != 0.0f;
        a.dropout = SmDropout(drop_p, seed, call);
        a.alpha = alpha.as<float>();
        a.w = a.drop ? a.alpha : a.soft_out;
        a.soft = a.grad_out = nullptr;
        a.grad_e = a.grad_q = a.grad_edge = nullptr;
        dot_launch<false>(a, chunked ? &chunks : nullptr, st.s);
      }
    }
  }
  return st.finish(rc);
}

extern "C" int glx_dot_attention(int device, const float* q, const float* k, const float* v, int64_t num_rows,
                                 int32_t dim, int32_t heads, const int64_t* rows, const float* edge,
                                 const int32_t* cnt, int32_t num_ids, int32_t num_segments, float scale,
                                 float default_attr, float drop_p, uint64_t seed, uint64_t call, float* logit_out,
                                 float* soft_out, float* out, int ptr_kind, void* stream) {
  return dot_attention_forward(false, device, q, k, v, num_rows, dim, heads, rows, edge, cnt, num_ids, num_segments,
                               scale, default_attr, drop_p, seed, call, logit_out, soft_out, out, ptr_kind, stream);
}

extern "C" int glx_dot_attention_chunked(int device, const float* q, const float* k, const float* v, int64_t num_rows,
                                         int32_t dim, int32_t heads, const int64_t* rows, const float* edge,
                                         const int32_t* cnt, int32_t num_ids, int32_t num_segments, float scale,
                                         float default_attr, float drop_p, uint64_t seed, uint64_t call,
                                         float* logit_out, float* soft_out, float* out, int ptr_kind, void* stream) {
  return dot_attention_forward(true, device, q, k, v, num_rows, dim, heads, rows, edge, cnt, num_ids, num_segments,
                               scale, default_attr, drop_p, seed, call, logit_out, soft_out, out, ptr_kind, stream);
}

// the body of glx_dot_attention_backward (chunked == false: its launches, its bits) and of
// glx_dot_attention_backward_chunked
static int dot_attention_backward(bool chunked, int device, const float* q, const float* k, const float* v,
                                  int64_t num_rows, int32_t dim, int32_t heads, const int64_t* rows, const float* edge,
                                  const int32_t* cnt, int32_t num_ids, int32_t num_segments, float scale,
                                  float default_attr, float drop_p, uint64_t seed, uint64_t call, const float* soft,
                                  const float* grad_out, float* grad_e_out, float* grad_q_out, float* grad_k_out,
                                  float* grad_v_out, float* grad_edge_out, int ptr_kind, void* stream) {
  GLX_DOT_ATTENTION_REQUIRE();
  GLX_REQUIRE(num_ids == 0 || soft != nullptr, "soft is NULL");
  GLX_REQUIRE(num_segments == 0 || grad_out != nullptr, "grad_out is NULL");
  GLX_REQUIRE(num_ids == 0 || grad_e_out != nullptr, "grad_e_out is NULL");
  GLX_REQUIRE(grad_edge_out == nullptr || edge != nullptr || num_ids == 0, "grad_edge_out needs edge");
  int rc = glx_init_device(device);
  if (rc != GLX_OK) return rc;
  const size_t count = (size_t)num_ids * heads, seg_count = (size_t)num_segments * dim;
  const size_t row_count = (size_t)num_rows * dim, edge_count = (size_t)num_ids * dim;
  if (count == 0 && (grad_q_out == nullptr || seg_count == 0) &&
      ((grad_k_out == nullptr && grad_v_out == nullptr) || row_count == 0)) {
    return GLX_OK;
  }
  GlxDeviceGuard guard(device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", device);
  GlxHostStage st(device, ptr_kind, stream, GlxHostStage::ADMIT);
  DotArgs a;
  const int32_t* d_cnt;
  float* d_gk;
  float* d_gv;
  st.in(&a.q, q, seg_count);
  st.in(&a.k, k, row_count);
  if (v != k) st.in(&a.v, v, row_count);
  st.in(&a.rows, rows, (size_t)num_ids);
  st.in(&a.edge, edge, edge_count);
  st.in(&d_cnt, cnt, (size_t)num_segments);
  st.in(&a.soft, soft, count);
  st.in(&a.grad_out, grad_out, seg_count);
  st.out(&a.grad_e, grad_e_out, count);
  st.out(&a.grad_q, grad_q_out, seg_count);
  st.out(&d_gk, grad_k_out, row_count);
  st.out(&d_gv, grad_v_out, row_count);
  st.out(&a.grad_edge, grad_edge_out, edge_count);
  rc = st.begin();
  if (v == k) a.v = a.k;  // one table: staged once
  GlxScratch lease, alpha;
  GlxChunkDir chunks;
  if (rc == GLX_OK) {
    if (num_ids == 0 || num_segments == 0) {  // nothing was consumed: every output is zeros
      rc = glx_zero_f32_async(a.grad_e, count, st.s);
      if (rc == GLX_OK) rc = glx_zero_f32_async(a.grad_q, seg_count, st.s);
      if (rc == GLX_OK) rc = glx_zero_f32_async(d_gk, row_count, st.s);
      if (rc == GLX_OK) rc = glx_zero_f32_async(d_gv, row_count, st.s);
      if (rc == GLX_OK) rc = glx_zero_f32_async(a.grad_edge, edge_count, st.s);
    } else {
      const bool want_rows = (d_gk != nullptr || d_gv != nullptr) && num_rows > 0;
      GlxAggTranspose tr;
      rc = glx_seg_layout_bwd(want_rows, a.rows, cnt ? d_cnt : nullptr, num_ids, num_segments, num_rows, st.s, &lease,
                              &tr, &a.seg);
      if (rc == GLX_OK && drop_p != 0.0f) {
        rc = alpha.alloc(count * sizeof(float), st.s, chunked ? kSlotAlphaChunked : kSlotAlpha);
      }
      if (rc == GLX_OK) {
        a.num_rows = num_rows;
        a.dim = dim;
        a.heads = heads;
        a.C = dim / heads;
        a.scale = scale;
        a.default_attr = default_attr;
        a.drop = drop_p != 0.0f;
        a.dropout = SmDropout(drop_p, seed, call);
        a.alpha = alpha.as<float>();
        a.w = a.drop ? a.alpha : a.soft;
        a.logit = a.soft_out = a.out = nullptr;
        if (chunked) {
          GlxScratch chunk_lease;  // ends with the block: the launches that use it are queued by then
          rc = dot_chunk_dir(a.seg, dim, st.s, &chunk_lease, &chunks);
          if (rc == GLX_OK) dot_launch<true>(a, &chunks, st.s);
        } else {
          dot_launch<true>(a, nullptr, st.s);
        }
        // the default mode of glx_weighted_bwd_x returns GLX_OK; the chunked one leases inside the call
        if (rc == GLX_OK && want_rows && d_gk) {
          rc = glx_weighted_bwd_x(GLX_AGG_SUM, tr, a.grad_e, a.q, d_gk, num_rows, dim, heads, num_ids, num_segments,
                                  st.s, GLX_DTYPE_F32, chunked);
        }
        if (rc == GLX_OK && want_rows && d_gv) {
          rc = glx_weighted_bwd_x(GLX_AGG_SUM, tr, a.w, a.grad_out, d_gv, num_rows, dim, heads, num_ids, num_segments,
                                  st.s, GLX_DTYPE_F32, chunked);
        }
      }
    }
  }
  return st.finish(rc);
}

extern "C" int glx_dot_attention_backward(int device, const float* q, const float* k, const float* v, int64_t num_rows,
                                          int32_t dim, int32_t heads, const int64_t* rows, const float* edge,
                                          const int32_t* cnt, int32_t num_ids, int32_t num_segments, float scale,
                                          float default_attr, float drop_p, uint64_t seed, uint64_t call,
                                          const float* soft, const float* grad_out, float* grad_e_out,
                                          float* grad_q_out, float* grad_k_out, float* grad_v_out, float* grad_edge_out,
                                          int ptr_kind, void* stream) {
  return dot_attention_backward(false, device, q, k, v, num_rows, dim, heads, rows, edge, cnt, num_ids, num_segments,
                                scale, default_attr, drop_p, seed, call, soft, grad_out, grad_e_out, grad_q_out,
                                grad_k_out, grad_v_out, grad_edge_out, ptr_kind, stream);
}

extern "C" int glx_dot_attention_backward_chunked(int device, const float* q, const float* k, const float* v,
                                                  int64_t num_rows, int32_t dim, int32_t heads, const int64_t* rows,
                                                  const float* edge, const int32_t* cnt, int32_t num_ids,
                                                  int32_t num_segments, float scale, float default_attr, float drop_p,
                                                  uint64_t seed, uint64_t call, const float* soft,
                                                  const float* grad_out, float* grad_e_out, float* grad_q_out,
                                                  float* grad_k_out, float* grad_v_out, float* grad_edge_out,
                                                  int ptr_kind, void* stream) {
  return dot_attention_backward(true, device, q, k, v, num_rows, dim, heads, rows, edge, cnt, num_ids, num_segments,
                                scale, default_attr, drop_p, seed, call, soft, grad_out, grad_e_out, grad_q_out,
                                grad_k_out, grad_v_out, grad_edge_out, ptr_kind, stream);
}
