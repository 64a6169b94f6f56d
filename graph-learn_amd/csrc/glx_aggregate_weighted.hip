// glx weighted segment aggregation: a per-position, optionally multi-head, weighted Sum / Mean over segments of
// gathered rows, with its gradients with respect to the rows and to the weights.  The reference's GCN layer scales every
// neighbour row by an edge coefficient before the segment sum (graphlearn/python/nn/tf/layers/gcn_conv.py:52-73), its
// GAT layers by a learned per-head attention coefficient (gat_conv.py:96-110, ego_gat_conv.py:98-103).
//
// Contract (include/glx.h).  x[num_rows, dim] float32, rows[num_ids] int64, w[num_ids, heads]
// float32, C = dim / heads, column c belongs to head c / C.  Segments as in glx_aggregate_backward: the prefix sums of
// the clamped cnt, or the implied layout of num_ids / num_segments positions each.  A row outside [0, num_rows) reads a
// row of default_attr.
//   forward      acc = +0.0f; for each position p of the segment in ascending order
//                acc = fadd_rn(acc, fmul_rn(w[p, head(c)], xrow(p)[c])); Mean: acc / float(count); empty: default_attr
//   grad_x       grad_x[r, c] = +0.0f, then for each consumed p with rows[p] == r in ascending p
//                fadd_rn(., fmul_rn(w[p, head(c)], t)), t = grad_out[s(p), c] (Sum) or grad_out[s(p), c] / float(count)
//   grad_w       grad_w[p, h] = sum over the columns of head h of grad_out[s(p), c] * xrow(p)[c] (Mean: / float(count));
//                a fixed lane-to-column mapping and a fixed cross-lane tree -- the same bits on every run, but the order
//                over the columns is the mapping's, so this one is checked against a bound, not bit for bit
// No float atomics anywhere.
//   grad_x, chunked  (glx_aggregate_weighted_backward_x_chunked; K5-bwd-chunked) the same terms in a second, opt-in
//                order, over the chunks of a row's list: glx_chunks.h has the order, the directory and the kernels.
//
// x is float32 or bfloat16 (the _ex entry points).  A bfloat16 x is upcast as it is loaded -- exact --
// and folded exactly as above, so emb and grad_w stay float32 and equal the float32 call on the upcast matrix bit for
// bit (grad_w: the same VEC, plan and tree).  A bfloat16 grad_x is the float32 sum above rounded once per element, to
// nearest even (glx_f32_to_bf16_bits), in the kernel's final store.  w, grad_out, emb and grad_w are always float32.
#include "glx_chunks.h"

// Two roundings per term: glx_fold_rn (glx_lane_groups.h) pins the product; the pragma is for the front end.
#pragma clang fp contract(off)

namespace {

constexpr int kWU = 4;  // row loads in flight per lane

// ---- forward -----------------------------------------------------------------------------------------------
struct WFwdArgs {
  const void* x;           // [num_rows, dim] of `dtype` elements
  int dtype;               // GLX_DTYPE_F32 or GLX_DTYPE_BF16
  const int64_t* rows;     // [num_ids]
  const float* w;          // [num_ids, heads]
  GlxSegLayout seg;
  const int32_t* cnt;      // [num_segments], or nullptr
  float* emb;              // [num_segments, dim]
  int64_t num_rows;
  int32_t dim, heads, C;
  float default_attr;
};

// G lanes own one segment; lane c owns columns [VEC c, VEC c + VEC) of each column tile of G * VEC columns (VEC = 4
// only when C % 4 == 0: a lane's columns then share one head).  Lane c fetches position base + c of the segment (its
// row, already tested against [0, num_rows)) and every lane of the group reads entry j from lane j; kWU row loads and
// their weights are issued before the first is folded.  The group walks its segment together, so the cross-lane reads
// stay inside a group whose lanes all run the same iterations.  A bfloat16 x is upcast as it is loaded (exact): the
// fold is the float32 kernel's on the upcast values, in its order.
template <int OP, int G, int VEC, int DT>
__global__ __launch_bounds__(256) void glx_aggregate_weighted_kernel(WFwdArgs a) {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  const typename AggElem<DT>::raw* __restrict__ x = static_cast<const typename AggElem<DT>::raw*>(a.x);
  const int64_t gid = blockIdx.x * (int64_t)(256 / G) + threadIdx.x / G;
  const int c = threadIdx.x & (G - 1);
  if (gid >= a.seg.num_segments) return;  // whole groups leave
  int32_t s0, s1;
  seg_bounds(a.seg, gid, &s0, &s1);
  float* const out = a.emb + gid * (int64_t)a.dim;
  for (int32_t col_pass = 0; col_pass < a.dim; col_pass += G * VEC) {
    const int32_t col = col_pass + c * VEC;
    const bool col_ok = col < a.dim;
    const int32_t col_ld = col_ok ? col : 0;  // lanes past the end re-read the first columns, unused
    const int32_t head = col_ld / a.C;
    vec_t acc;
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.0f;
    for (int32_t base = s0; base < s1; base += G) {
      int32_t my_row = -1;
      if (base + c < s1) {
        const int64_t r = a.rows[base + c];
        my_row = (r >= 0 && r < a.num_rows) ? (int32_t)r : -1;
      }
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
            if (row[u] >= 0) {
              val[u] = agg_load<DT, VEC>(x + row[u] * (int64_t)a.dim + col_ld);
            } else {
#pragma unroll
              for (int v = 0; v < VEC; ++v) val[u][v] = a.default_attr;
            }
          }
        }
#pragma unroll
        for (int u = 0; u < kWU; ++u) {
          if (j + u < m) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = glx_fold_rn(acc[v], wt[u], val[u][v]);
          }
        }
      }
    }
    if (s1 == s0) {  // FinalFunc: aggregator.cc:74-86 (empty -> default)
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] = a.default_attr;
    } else if (OP == GLX_AGG_MEAN) {
      const float fn = (float)(s1 - s0);  // the positions consumed
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] = acc[v] / fn;
    }
    if (col_ok) *reinterpret_cast<vec_t*>(out + col) = acc;
  }
}

template <int OP, int VEC>
void launch_wfwd_vec(const WFwdArgs& a, hipStream_t s) {
  const int G = glx_group_for((a.dim + VEC - 1) / VEC);
  const unsigned blocks = (unsigned)(((int64_t)a.seg.num_segments + (256 / G) - 1) / (256 / G));
  glx_for_group(G, [&](auto g) {
    glx_for_train_dtype(a.dtype, [&](auto t) {
      glx_aggregate_weighted_kernel<OP, decltype(g)::value, VEC, decltype(t)::value><<<blocks, 256, 0, s>>>(a);
    });
  });
}

template <int OP>
void launch_wfwd(const WFwdArgs& a, hipStream_t s) {
  const bool vec4 = a.dim % 4 == 0 && a.C % 4 == 0 && glx_aligned_vec4(a.x, a.dtype) && glx_aligned16(a.emb);
  if (vec4) launch_wfwd_vec<OP, 4>(a, s);
  else launch_wfwd_vec<OP, 1>(a, s);
}

// ---- gradient with respect to the rows ------------------------------------------------------------------------
struct WBwdXArgs {
  GlxAggTranspose t;
  const float* w;         // [num_ids, heads]
  const float* grad_out;  // [num_segments, dim]
  void* grad_x;           // [num_rows, dim] of `dtype` elements
  int dtype;              // GLX_DTYPE_F32 or GLX_DTYPE_BF16
  GlxSegLayout seg;       // the transpose's segment ends and fanout: Mean's divisor
  int64_t num_rows;
  int32_t dim, heads, C;
};

// The term of one list entry for the lane's VEC columns from `col` on (one head: VEC = 4 only when C % 4 == 0):
// fmul_rn(w[p, head], t), t = g (Sum) or g / float(count) (Mean), added through glx_fold_rn -- two roundings.
template <int OP, int VEC>
struct WBwdXTerm {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  static constexpr bool kDiv = OP == GLX_AGG_MEAN;
  struct Loaded {
    vec_t g;
    float wt;
  };
  const WBwdXArgs& a;
  int32_t col, head;
  __device__ __forceinline__ float divisor(int32_t seg) const { return (float)seg_count(a.seg, seg); }
  __device__ __forceinline__ void load(Loaded* ld, int32_t p, int32_t seg) const {
    ld->g = *reinterpret_cast<const vec_t*>(a.grad_out + ((int64_t)seg * a.dim + col));
    ld->wt = a.w[(int64_t)p * a.heads + head];
  }
  __device__ __forceinline__ void fold(vec_t* acc, const Loaded& ld, int32_t, float dv) const {
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const float t = kDiv ? ld.g[v] / dv : ld.g[v];
      (*acc)[v] = glx_fold_rn((*acc)[v], ld.wt, t);
    }
  }
};

// the request of glx_row_grad_launch (glx_chunks.h)
template <int OP>
struct WBwdXReq {
  static constexpr int kU = kWU;
  WBwdXArgs a;
  __host__ __device__ const int32_t* row_ptr() const { return a.t.row_ptr; }
  __device__ GlxPosList list() const { return {a.t.pos, a.t.seg_of, a.t.fanout}; }
  __host__ __device__ int64_t num_rows() const { return a.num_rows; }
  __host__ __device__ int32_t dim() const { return a.dim; }
  __host__ __device__ void* grad_x() const { return a.grad_x; }
  int dtype() const { return a.dtype; }
  template <int VEC>
  __device__ WBwdXTerm<OP, VEC> term(int32_t col) const { return {a, col, col / a.C}; }
};

// ch == nullptr: the default order; otherwise the chunked one over that directory
template <int OP>
void launch_wbwd_x(const WBwdXArgs& a, const GlxChunkDir* ch, hipStream_t s) {
  const bool vec4 =
      a.dim % 4 == 0 && a.C % 4 == 0 && glx_aligned16(a.grad_out) && glx_aligned_vec4(a.grad_x, a.dtype);
  if (vec4) glx_row_grad_launch<4>(WBwdXReq<OP>{a}, ch, s);
  else glx_row_grad_launch<1>(WBwdXReq<OP>{a}, ch, s);
}

// ---- gradient with respect to the weights ---------------------------------------------------------------------
struct WBwdWArgs {
  const void* x;           // [num_rows, dim] of `dtype` elements
  int dtype;               // GLX_DTYPE_F32 or GLX_DTYPE_BF16
  const int64_t* rows;     // [num_ids]
  GlxSegLayout seg;
  const int32_t* cnt;      // [num_segments], or nullptr
  const float* grad_out;   // [num_segments, dim]
  float* grad_w;           // [num_ids, heads]
  int64_t num_rows;
  int32_t dim, heads, C;
  GlxHeadDots hd;
  float default_attr;
};

// G lanes own one POSITION p and write grad_w[p, 0 .. heads): glx_head_dots (glx_lane_groups.h) of the segment's
// grad_out row and the position's table row.  A position that was not consumed writes +0.0f; an out-of-range row
// multiplies a row of default_attr.  A bfloat16 x is upcast as it is loaded: the same products in the same tree.
template <int OP, int G, int VEC, bool SUB, int DT>
__global__ __launch_bounds__(256) void glx_aggregate_weighted_bwd_w_kernel(WBwdWArgs a) {
  const int64_t p = blockIdx.x * (int64_t)(256 / G) + threadIdx.x / G;
  const int c = threadIdx.x & (G - 1);
  if (p >= a.seg.num_ids) return;  // whole groups leave
  float* const out = a.grad_w + p * (int64_t)a.heads;
  int32_t sg;
  if (!seg_of_position(a.seg, p, &sg)) {  // the same answer in every lane of the group
    for (int32_t h = c; h < a.heads; h += G) out[h] = 0.0f;
    return;
  }
  const float div = OP == GLX_AGG_MEAN ? (float)seg_count(a.seg, sg) : 1.0f;
  const GlxRow go = {a.grad_out + sg * (int64_t)a.dim, true};
  const GlxRowOf<DT> xr =
      glx_row<DT>(static_cast<const typename AggElem<DT>::raw*>(a.x), a.rows[p], a.num_rows, a.dim);
  glx_head_dots<G, VEC, SUB, OP == GLX_AGG_MEAN>(go, xr, a.default_attr, a.dim, a.heads, a.C, a.hd, div, c, out);
}

template <int OP, int VEC>
void launch_wbwd_w_vec(WBwdWArgs a, hipStream_t s) {
  const GlxHeadDotPlan plan = glx_head_dot_plan(a.dim, a.C, VEC);
  const int G = plan.G;
  a.hd = plan.hd;
  const unsigned blocks = (unsigned)(((int64_t)a.seg.num_ids + (256 / G) - 1) / (256 / G));
  glx_for_group(G, [&](auto g) {
    glx_for_train_dtype(a.dtype, [&](auto t) {
      constexpr int kG = decltype(g)::value, kDT = decltype(t)::value;
      if (plan.sub_groups) glx_aggregate_weighted_bwd_w_kernel<OP, kG, VEC, true, kDT><<<blocks, 256, 0, s>>>(a);
      else glx_aggregate_weighted_bwd_w_kernel<OP, kG, VEC, false, kDT><<<blocks, 256, 0, s>>>(a);
    });
  });
}

template <int OP>
void launch_wbwd_w(const WBwdWArgs& a, hipStream_t s) {
  // the same VEC, and so the same plan and reduction tree, for a bfloat16 x as for the float32 matrix of its values
  const bool vec4 = a.dim % 4 == 0 && a.C % 4 == 0 && glx_aligned_vec4(a.x, a.dtype) && glx_aligned16(a.grad_out);
  if (vec4) launch_wbwd_w_vec<OP, 4>(a, s);
  else launch_wbwd_w_vec<OP, 1>(a, s);
}

}  // namespace

// grad_x of a request whose transpose the caller holds (device pointers, op Sum or Mean): the body of
// glx_aggregate_weighted_backward_x, and the two row gradients of glx_dot_attention_backward on one transpose
int glx_weighted_bwd_x(int op, const GlxAggTranspose& t, const float* w, const float* grad_out, void* grad_x,
                       int64_t num_rows, int32_t dim, int32_t heads, int32_t num_ids, int32_t num_segments,
                       hipStream_t s, int grad_x_dtype, bool chunked) {
  GlxScratch chunk_lease;  // ends on return: the launches below are queued by then
  GlxChunkDir chunks;
  const GlxChunkDir* ch = nullptr;
  if (chunked) {
    const int rc = glx_row_chunk_dir(t, num_ids, num_rows, dim, s, &chunk_lease, &chunks);
    if (rc != GLX_OK) return rc;
    ch = &chunks;
  }
  WBwdXArgs a;
  a.t = t;
  a.w = w;
  a.grad_out = grad_out;
  a.grad_x = grad_x;
  a.dtype = grad_x_dtype;
  a.num_rows = num_rows;
  a.dim = dim;
  a.heads = heads;
  a.C = dim / heads;
  a.seg = glx_seg_layout_of(t, num_ids, num_segments);
  if (op == GLX_AGG_SUM) launch_wbwd_x<GLX_AGG_SUM>(a, ch, s);
  else launch_wbwd_x<GLX_AGG_MEAN>(a, ch, s);
  return GLX_OK;
}

// what the three entry points check alike, before any device use
#define GLX_WEIGHTED_REQUIRE(who)                                                                                       \
  GLX_REQUIRE(op >= GLX_AGG_SUM && op <= GLX_AGG_PROD, "unknown aggregator id %d", op);                                 \
  GLX_REQUIRE(op == GLX_AGG_SUM || op == GLX_AGG_MEAN, who " reduces with Sum or Mean only, not with %s",               \
              glx_agg_op_name(op));                                                                                     \
  GLX_REQUIRE(num_ids >= 0 && num_segments >= 0 && num_rows >= 0, "negative sizes");                                    \
  GLX_REQUIRE(dim > 0, "dim must be positive, got %d", dim);                                                            \
  GLX_REQUIRE(heads > 0, "heads must be positive, got %d", heads);                                                      \
  GLX_REQUIRE(dim % heads == 0, "dim %d is not a multiple of heads %d", dim, heads);                                    \
  GLX_REQUIRE(num_rows < INT32_MAX, "num_rows must be < 2^31");                                                         \
  GLX_REQUIRE((int64_t)num_ids * heads <= INT32_MAX, "num_ids * heads exceeds int32");                                  \
  GLX_REQUIRE((int64_t)num_segments * dim <= INT32_MAX, "num_segments * dim exceeds int32 (tensor.h:47)");              \
  GLX_REQUIRE(ptr_kind == GLX_PTR_HOST || ptr_kind == GLX_PTR_DEVICE, "bad ptr_kind")

extern "C" int glx_aggregate_weighted_ex(int device, int op, const void* x, int x_dtype, int64_t num_rows, int32_t dim,
                                         const int64_t* rows, const float* w, int32_t heads, const int32_t* cnt,
                                         int32_t num_ids, int32_t num_segments, float default_attr, float* emb_out,
                                         int ptr_kind, void* stream) {
  GLX_REQUIRE_TRAIN_DTYPE(x_dtype, "glx_aggregate_weighted_ex: x_dtype");
  GLX_WEIGHTED_REQUIRE("glx_aggregate_weighted");
  GLX_REQUIRE(num_rows == 0 || x != nullptr, "x is NULL");
  GLX_REQUIRE(num_ids == 0 || rows != nullptr, "rows is NULL");
  GLX_REQUIRE(num_ids == 0 || w != nullptr, "w is NULL");
  GLX_REQUIRE(num_segments == 0 || emb_out != nullptr, "emb_out is NULL");
  int rc = glx_init_device(device);
  if (rc != GLX_OK) return rc;
  if (num_segments == 0) return GLX_OK;
  GlxDeviceGuard guard(device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", device);
  GlxHostStage st(device, ptr_kind, stream, GlxHostStage::ADMIT);
  WFwdArgs a;
  a.dtype = x_dtype;
  st.in_bytes(&a.x, x, (size_t)num_rows * dim * (size_t)glx_dtype_size(x_dtype));
  st.in(&a.rows, rows, (size_t)num_ids);
  st.in(&a.w, w, (size_t)num_ids * heads);
  st.in(&a.cnt, cnt, (size_t)num_segments);
  st.out(&a.emb, emb_out, (size_t)num_segments * dim);
  rc = st.begin();
  GlxScratch lease;
  if (cnt == nullptr) a.cnt = nullptr;
  if (rc == GLX_OK) rc = glx_seg_layout(a.cnt, num_ids, num_segments, st.s, &lease, &a.seg);
  if (rc == GLX_OK) {
    a.num_rows = num_rows;
    a.dim = dim;
    a.heads = heads;
    a.C = dim / heads;
    a.default_attr = default_attr;
    if (op == GLX_AGG_SUM) launch_wfwd<GLX_AGG_SUM>(a, st.s);
    else launch_wfwd<GLX_AGG_MEAN>(a, st.s);
  }
  return st.finish(rc);
}

extern "C" int glx_aggregate_weighted(int device, int op, const float* x, int64_t num_rows, int32_t dim,
                                      const int64_t* rows, const float* w, int32_t heads, const int32_t* cnt,
                                      int32_t num_ids, int32_t num_segments, float default_attr, float* emb_out,
                                      int ptr_kind, void* stream) {
  return glx_aggregate_weighted_ex(device, op, x, GLX_DTYPE_F32, num_rows, dim, rows, w, heads, cnt, num_ids,
                                   num_segments, default_attr, emb_out, ptr_kind, stream);
}

// the body of glx_aggregate_weighted_backward_x_ex and glx_aggregate_weighted_backward_x_chunked, which have checked
// grad_x_dtype
static int weighted_backward_x(int device, int op, const int64_t* rows, const float* w, int32_t heads,
                               const int32_t* cnt, int32_t num_ids, int32_t num_segments, int64_t num_rows,
                               int32_t dim, const float* grad_out, void* grad_x, int grad_x_dtype, bool chunked,
                               int ptr_kind, void* stream) {
  GLX_WEIGHTED_REQUIRE("glx_aggregate_weighted_backward_x");
  GLX_REQUIRE(num_ids == 0 || rows != nullptr, "rows is NULL");
  GLX_REQUIRE(num_ids == 0 || w != nullptr, "w is NULL");
  GLX_REQUIRE(num_segments == 0 || grad_out != nullptr, "grad_out is NULL");
  GLX_REQUIRE(num_rows == 0 || grad_x != nullptr, "grad_x is NULL");
  int rc = glx_init_device(device);
  if (rc != GLX_OK) return rc;
  if (num_rows == 0) return GLX_OK;
  GlxDeviceGuard guard(device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", device);
  GlxHostStage st(device, ptr_kind, stream, GlxHostStage::ADMIT);
  const int64_t* d_rows;
  const int32_t* d_cnt;
  WBwdXArgs a;
  st.in(&d_rows, rows, (size_t)num_ids);
  st.in(&a.w, w, (size_t)num_ids * heads);
  st.in(&d_cnt, cnt, (size_t)num_segments);
  st.in(&a.grad_out, grad_out, (size_t)num_segments * dim);
  st.out_bytes(&a.grad_x, grad_x, (size_t)num_rows * dim * (size_t)glx_dtype_size(grad_x_dtype));
  rc = st.begin();
  GlxScratch lease;
  if (rc == GLX_OK) {
    if (num_ids == 0 || num_segments == 0) {  // nothing was consumed: every row is zeros
      rc = glx_zero_elems_async(a.grad_x, (size_t)num_rows * dim, grad_x_dtype, st.s);
    } else {
      rc = glx_agg_transpose(d_rows, cnt ? d_cnt : nullptr, num_ids, num_segments, num_rows, st.s, &lease, &a.t);
      if (rc == GLX_OK) {
        rc = glx_weighted_bwd_x(op, a.t, a.w, a.grad_out, a.grad_x, num_rows, dim, heads, num_ids, num_segments, st.s,
                                grad_x_dtype, chunked);
      }
    }
  }
  return st.finish(rc);
}

extern "C" int glx_aggregate_weighted_backward_x_ex(int device, int op, const int64_t* rows, const float* w,
                                                    int32_t heads, const int32_t* cnt, int32_t num_ids,
                                                    int32_t num_segments, int64_t num_rows, int32_t dim,
                                                    const float* grad_out, void* grad_x, int grad_x_dtype,
                                                    int ptr_kind, void* stream) {
  GLX_REQUIRE_TRAIN_DTYPE(grad_x_dtype, "glx_aggregate_weighted_backward_x_ex: grad_x_dtype");
  return weighted_backward_x(device, op, rows, w, heads, cnt, num_ids, num_segments, num_rows, dim, grad_out, grad_x,
                             grad_x_dtype, false, ptr_kind, stream);
}

extern "C" int glx_aggregate_weighted_backward_x_chunked(int device, int op, const int64_t* rows, const float* w,
                                                         int32_t heads, const int32_t* cnt, int32_t num_ids,
                                                         int32_t num_segments, int64_t num_rows, int32_t dim,
                                                         const float* grad_out, void* grad_x, int grad_x_dtype,
                                                         int ptr_kind, void* stream) {
  GLX_REQUIRE_TRAIN_DTYPE(grad_x_dtype, "glx_aggregate_weighted_backward_x_chunked: grad_x_dtype");
  return weighted_backward_x(device, op, rows, w, heads, cnt, num_ids, num_segments, num_rows, dim, grad_out, grad_x,
                             grad_x_dtype, true, ptr_kind, stream);
}

extern "C" int glx_aggregate_weighted_backward_x(int device, int op, const int64_t* rows, const float* w, int32_t heads,
                                                 const int32_t* cnt, int32_t num_ids, int32_t num_segments,
                                                 int64_t num_rows, int32_t dim, const float* grad_out, float* grad_x,
                                                 int ptr_kind, void* stream) {
  return glx_aggregate_weighted_backward_x_ex(device, op, rows, w, heads, cnt, num_ids, num_segments, num_rows, dim,
                                              grad_out, grad_x, GLX_DTYPE_F32, ptr_kind, stream);
}

extern "C" int glx_aggregate_weighted_backward_w_ex(int device, int op, const void* x, int x_dtype, int64_t num_rows,
                                                    int32_t dim, const int64_t* rows, int32_t heads,
                                                    const int32_t* cnt, int32_t num_ids, int32_t num_segments,
                                                    float default_attr, const float* grad_out, float* grad_w,
                                                    int ptr_kind, void* stream) {
  GLX_REQUIRE_TRAIN_DTYPE(x_dtype, "glx_aggregate_weighted_backward_w_ex: x_dtype");
  GLX_WEIGHTED_REQUIRE("glx_aggregate_weighted_backward_w");
  GLX_REQUIRE(num_rows == 0 || x != nullptr, "x is NULL");
  GLX_REQUIRE(num_ids == 0 || rows != nullptr, "rows is NULL");
  GLX_REQUIRE(num_segments == 0 || grad_out != nullptr, "grad_out is NULL");
  GLX_REQUIRE(num_ids == 0 || grad_w != nullptr, "grad_w is NULL");
  int rc = glx_init_device(device);
  if (rc != GLX_OK) return rc;
  if (num_ids == 0) return GLX_OK;
  GlxDeviceGuard guard(device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", device);
  GlxHostStage st(device, ptr_kind, stream, GlxHostStage::ADMIT);
  WBwdWArgs a;
  a.dtype = x_dtype;
  st.in_bytes(&a.x, x, (size_t)num_rows * dim * (size_t)glx_dtype_size(x_dtype));
  st.in(&a.rows, rows, (size_t)num_ids);
  st.in(&a.cnt, cnt, (size_t)num_segments);
  st.in(&a.grad_out, grad_out, (size_t)num_segments * dim);
  st.out(&a.grad_w, grad_w, (size_t)num_ids * heads);
  rc = st.begin();
  GlxScratch lease;
  if (rc == GLX_OK) {
    if (num_segments == 0) {  // nothing was consumed
      rc = glx_zero_f32_async(a.grad_w, (size_t)num_ids * heads, st.s);
    } else {
      if (cnt == nullptr) a.cnt = nullptr;
      rc = glx_seg_layout(a.cnt, num_ids, num_segments, st.s, &lease, &a.seg);
      if (rc == GLX_OK) {
        a.num_rows = num_rows;
        a.dim = dim;
        a.heads = heads;
        a.C = dim / heads;
        a.default_attr = default_attr;
        if (op == GLX_AGG_SUM) launch_wbwd_w<GLX_AGG_SUM>(a, st.s);
        else launch_wbwd_w<GLX_AGG_MEAN>(a, st.s);
      }
    }
  }
  return st.finish(rc);
}

extern "C" int glx_aggregate_weighted_backward_w(int device, int op, const float* x, int64_t num_rows, int32_t dim,
                                                 const int64_t* rows, int32_t heads, const int32_t* cnt,
                                                 int32_t num_ids, int32_t num_segments, float default_attr,
                                                 const float* grad_out, float* grad_w, int ptr_kind, void* stream) {
  return glx_aggregate_weighted_backward_w_ex(device, op, x, GLX_DTYPE_F32, num_rows, dim, rows, heads, cnt, num_ids,
                                              num_segments, default_attr, grad_out, grad_w, ptr_kind, stream);
}
