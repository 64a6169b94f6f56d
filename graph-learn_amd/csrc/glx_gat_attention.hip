// glx fused GAT attention and its gradients: the logit of every (neighbour, head), leaky_relu, the softmax over each
// segment of a counts= request and dropout on the coefficients, in one kernel per direction -- the attention step of
// the reference's GATConv (graphlearn/python/nn/tf/layers/gat_conv.py:96-104: leaky_relu(self + neighbour),
// unsorted_segment_softmax, nn/tf/utils/softmax.py:24-50, then tf.nn.dropout).
//
// Contract (include/glx.h).  Segments as in glx_segment_softmax.  For a consumed position p of
// segment sg and head h:
//   logit     tv = t[rows[p], h], or default_attr for a row outside [0, num_rows); pre = s[sg, h] + tv;
//             e = pre > 0 ? pre : pre * negative_slope  (two float32 roundings; default_attr = -inf masks a position)
//   softmax   soft = expf(e - max) / sum, glx_segment_softmax's definition, bound and exact rules
//   dropout   element i = p * heads + h draws word i & 3 of Philox block i >> 2 (row 0, seed, call) and is kept iff
//             word >= T = floor(drop_p * 2^32); alpha = keep ? soft * scale : +0.0f, scale = 1.0f / (1.0f - drop_p);
//             drop_p == 0 evaluates no Philox and alpha == soft
//   backward  ga = keep ? grad_alpha * scale : +0.0f (the mask is recomputed); d = soft * (ga - sum_q soft_q * ga_q);
//             grad_e = pre > 0 ? d : d * negative_slope; grad_s[sg, h] = the segment's sum of grad_e, by the same
//             lane group; grad_t[r, h] = +0.0f plus grad_e[p, h] over the consumed p with rows[p] == r in ascending p
// EVERY element of every output is written; a position that is not consumed gets +0.0f.  No float atomics: the lane
// mapping and the trees are fixed (glx_segment_lanes.h), so the same inputs give the same bits on every call.
#include <math.h>

#include "glx_segment_lanes.h"

namespace {

struct GatArgs {
  const float* s;          // [num_segments, heads]
  const float* t;          // [num_rows, heads]
  const int64_t* rows;     // [num_ids]
  GlxSegLayout seg;
  const float* soft;       // backward: the forward's softmax            [num_ids, heads]
  const float* g;          // backward: grad_alpha                       [num_ids, heads]
  float* soft_out;         // forward: softmax before dropout, or nullptr
  float* out;              // forward: alpha_out; backward: grad_e       [num_ids, heads]
  float* grad_s;           // backward: [num_segments, heads], or nullptr
  int64_t num_rows;
  int32_t heads;
  float slope, default_attr;
  SmDropout drop;
};

// s[sg, h] + t[rows[p], h]: one coalesced load of rows per item, a gather of the narrow table t
__device__ __forceinline__ float gat_pre(const GatArgs& a, float sv, int32_t p, int h) {
  const int64_t r = a.rows[p];
  const float tv = (r >= 0 && r < a.num_rows) ? a.t[r * a.heads + h] : a.default_attr;
  return sv + tv;
}

__device__ __forceinline__ float gat_leaky(float x, float pre, float slope) { return pre > 0.0f ? x : x * slope; }

// What sm_forward / sm_backward (glx_segment_lanes.h) read and write here, for the items of head h of a segment whose
// s[sg, h] is sv.  Forward: a spilled item parks its logit, then its exponential, in alpha_out.  Dropout of element
// idx = p * heads + h is the same function going forward and going back.
template <bool DROP>
struct GatIo {
  const GatArgs& a;
  const SmItems& it;
  float sv;
  int h;
  static constexpr bool kSum = true;  // grad_s
  __device__ __forceinline__ float drop(float x, int32_t at) const { return DROP ? sm_dropout(x, at, a.drop) : x; }
  __device__ __forceinline__ float logit(int32_t i) const {
    const float pre = gat_pre(a, sv, it.pos(i), h);
    return gat_leaky(pre, pre, a.slope);
  }
  __device__ __forceinline__ float spill_logit(int32_t i) const { return a.out[it.idx(i)] = logit(i); }
  __device__ __forceinline__ float parked_logit(int32_t i) const { return a.out[it.idx(i)]; }
  __device__ __forceinline__ void park_exp(int32_t i, float t) const { a.out[it.idx(i)] = t; }
  __device__ __forceinline__ float parked_exp(int32_t i) const { return a.out[it.idx(i)]; }
  __device__ __forceinline__ void emit_soft(int32_t i, float soft) const {
    const int32_t at = it.idx(i);
    if (a.soft_out) a.soft_out[at] = soft;
    a.out[at] = drop(soft, at);
  }
  __device__ __forceinline__ float soft(int32_t i) const { return a.soft[it.idx(i)]; }
  __device__ __forceinline__ float grad(int32_t i) const {
    const int32_t at = it.idx(i);
    return drop(a.g[at], at);
  }
  __device__ __forceinline__ float emit_grad(int32_t i, float, float d) const {
    return a.out[it.idx(i)] = gat_leaky(d, gat_pre(a, sv, it.pos(i), h), a.slope);
  }
};

// The mapping of glx_segment_softmax_kernel (sm_segment_walk, glx_segment_lanes.h): G lanes own one segment, a
// workgroup 256 / G consecutive segments; FLAT (heads a power of two <= G) reduces every head at once with strides
// G / 2 .. heads, otherwise head by head.  A segment of more than kSmLongItems items is left to the second phase, where
// the whole workgroup walks it.  Last, the workgroups share the positions nobody consumed: +0.0f.  No thread leaves
// before the end.
template <int G, bool FLAT, bool DROP, bool BWD>
__global__ __launch_bounds__(256) void glx_gat_attention_kernel(GatArgs a) {
  __shared__ float red[256];
  const int H = a.heads;
  sm_segment_walk<G>(
      a.seg, H, FLAT, red,
      [&](const auto& w, const SmItems& it, int64_t sg) {
        const int h = FLAT ? (w.lane() & (H - 1)) : it.o;
        const GatIo<DROP> io = {a, it, a.s[sg * H + h], h};
        if (BWD) {
          const float gs = sm_backward(w, it, io);  // the same bits in every lane of a head
          if (a.grad_s && w.lane() < it.min_off) a.grad_s[sg * H + h] = gs;
        } else {
          sm_forward(w, it, io);
        }
      },
      [&](int64_t sg, int c) {  // an empty segment: +0.0f
        if (BWD && a.grad_s) {
          for (int h = c; h < H; h += G) a.grad_s[sg * H + h] = 0.0f;
        }
      },
      [&](int64_t i) {
        a.out[i] = 0.0f;
        if (!BWD && a.soft_out) a.soft_out[i] = 0.0f;
      });
}

template <bool BWD>
void gat_launch(const GatArgs& a, bool drop, hipStream_t s) {
  sm_for_launch(a.heads, a.seg, [&](auto g, auto flat, unsigned blocks) {
    constexpr int kG = decltype(g)::value;
    constexpr bool kFlat = decltype(flat)::value;
    if (drop) glx_gat_attention_kernel<kG, kFlat, true, BWD><<<blocks, 256, 0, s>>>(a);
    else glx_gat_attention_kernel<kG, kFlat, false, BWD><<<blocks, 256, 0, s>>>(a);
  });
}

// grad_t: one lane per (row, head) walks the row's positions in ascending order (the transpose's stable sort), so
// the bits are those of glx_aggregate_backward(Sum) with one position per segment.  Rows of `heads` floats are too
// narrow for that kernel's 8 .. 64-lane row groups.
__global__ __launch_bounds__(256) void glx_gat_grad_t_kernel(const int32_t* __restrict__ row_ptr,
                                                             const int32_t* __restrict__ pos,
                                                             const float* __restrict__ grad_e,
                                                             float* __restrict__ grad_t, int64_t total, int32_t heads) {
  const int64_t i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= total) return;
  const int64_t r = i / heads;
  const int32_t h = (int32_t)(i - r * heads);
  const int32_t l0 = row_ptr[r], l1 = row_ptr[r + 1];
  float acc = 0.0f;
  for (int32_t j = l0; j < l1; ++j) acc = acc + grad_e[(int64_t)pos[j] * heads + h];
  grad_t[i] = acc;
}

}  // namespace

// what the two entry points check alike, before any device use
#define GLX_GAT_REQUIRE()                                                                                      \
  GLX_REQUIRE(num_ids >= 0 && num_segments >= 0 && num_rows >= 0, "negative sizes");                           \
  GLX_REQUIRE(heads >= 1, "heads must be positive, got %d", heads);                                            \
  GLX_REQUIRE((int64_t)num_ids * heads <= INT32_MAX, "num_ids * heads exceeds int32");                         \
  GLX_REQUIRE((int64_t)num_segments * heads <= INT32_MAX, "num_segments * heads exceeds int32");               \
  GLX_REQUIRE(num_rows <= INT32_MAX, "num_rows must be < 2^31");                                               \
  GLX_REQUIRE(isfinite(negative_slope) && negative_slope >= 0.0f, "negative_slope must be finite and >= 0");   \
  GLX_REQUIRE(drop_p >= 0.0f && drop_p < 1.0f, "drop_p must lie in [0, 1)");                                   \
  GLX_REQUIRE(ptr_kind == GLX_PTR_HOST || ptr_kind == GLX_PTR_DEVICE, "bad ptr_kind");                         \
  GLX_REQUIRE(cnt != nullptr || num_segments == 0 || num_ids % num_segments == 0,                              \
              "cnt == NULL means equal segments: num_ids must be a multiple of num_segments");                 \
  GLX_REQUIRE(num_ids == 0 || rows != nullptr, "rows is NULL");                                                \
  GLX_REQUIRE(num_ids == 0 || num_segments == 0 || s != nullptr, "s is NULL");                                 \
  GLX_REQUIRE(num_ids == 0 || num_rows == 0 || t != nullptr, "t is NULL")

extern "C" int glx_gat_attention(int device, const float* s, const float* t, int64_t num_rows, const int64_t* rows,
                                 int32_t heads, const int32_t* cnt, int32_t num_ids, int32_t num_segments,
                                 float negative_slope, float default_attr, float drop_p, uint64_t seed, uint64_t call,
                                 float* soft_out, float* alpha_out, int ptr_kind, void* stream) {
  GLX_GAT_REQUIRE();
  GLX_REQUIRE(num_ids == 0 || alpha_out != nullptr, "alpha_out is NULL");
  GLX_REQUIRE(soft_out != nullptr || drop_p == 0.0f || num_ids == 0, "soft_out may be NULL only when drop_p == 0");
  int rc = glx_init_device(device);
  if (rc != GLX_OK) return rc;
  if (num_ids == 0) return GLX_OK;
  GlxDeviceGuard guard(device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", device);
  GlxHostStage st(device, ptr_kind, stream, GlxHostStage::ADMIT);
  GatArgs a;
  const int32_t* d_cnt;
  const size_t count = (size_t)num_ids * heads;
  st.in(&a.s, s, (size_t)num_segments * heads);
  st.in(&a.t, t, (size_t)num_rows * heads);
  st.in(&a.rows, rows, (size_t)num_ids);
  st.in(&d_cnt, cnt, (size_t)num_segments);
  st.out(&a.soft_out, soft_out, count);
  st.out(&a.out, alpha_out, count);
  rc = st.begin();
  GlxScratch lease;
  if (rc == GLX_OK) {
    if (num_segments == 0) {  // nothing was consumed
      rc = glx_zero_f32_async(a.out, count, st.s);
      if (rc == GLX_OK) rc = glx_zero_f32_async(a.soft_out, count, st.s);
    } else {
      rc = glx_seg_layout(cnt ? d_cnt : nullptr, num_ids, num_segments, st.s, &lease, &a.seg);
      if (rc == GLX_OK) {
        a.soft = a.g = nullptr;
        a.grad_s = nullptr;
        a.num_rows = num_rows;
        a.heads = heads;
        a.slope = negative_slope;
        a.default_attr = default_attr;
        a.drop = SmDropout(drop_p, seed, call);
        gat_launch<false>(a, drop_p != 0.0f, st.s);
      }
    }
  }
  return st.finish(rc);
}

extern "C" int glx_gat_attention_backward(int device, const float* soft, const float* grad_alpha, const float* s,
                                          const float* t, int64_t num_rows, const int64_t* rows, int32_t heads,
                                          const int32_t* cnt, int32_t num_ids, int32_t num_segments,
                                          float negative_slope, float default_attr, float drop_p, uint64_t seed,
                                          uint64_t call, float* grad_e_out, float* grad_s_out, float* grad_t_out,
                                          int ptr_kind, void* stream) {
  GLX_GAT_REQUIRE();
  GLX_REQUIRE(num_ids == 0 || soft != nullptr, "soft is NULL");
  GLX_REQUIRE(num_ids == 0 || grad_alpha != nullptr, "grad_alpha is NULL");
  GLX_REQUIRE(num_ids == 0 || grad_e_out != nullptr, "grad_e_out is NULL");
  int rc = glx_init_device(device);
  if (rc != GLX_OK) return rc;
  const size_t count = (size_t)num_ids * heads;
  const size_t s_count = (size_t)num_segments * heads, t_count = (size_t)num_rows * heads;
  if (count == 0 && (grad_s_out == nullptr || s_count == 0) && (grad_t_out == nullptr || t_count == 0)) return GLX_OK;
  GlxDeviceGuard guard(device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", device);
  GlxHostStage st(device, ptr_kind, stream, GlxHostStage::ADMIT);
  GatArgs a;
  const int32_t* d_cnt;
  float* d_gt;
  st.in(&a.soft, soft, count);
  st.in(&a.g, grad_alpha, count);
  st.in(&a.s, s, s_count);
  st.in(&a.t, t, t_count);
  st.in(&a.rows, rows, (size_t)num_ids);
  st.in(&d_cnt, cnt, (size_t)num_segments);
  st.out(&a.out, grad_e_out, count);
  st.out(&a.grad_s, grad_s_out, s_count);
  st.out(&d_gt, grad_t_out, t_count);
  rc = st.begin();
  GlxScratch lease;
  if (rc == GLX_OK) {
    if (num_ids == 0 || num_segments == 0) {  // nothing was consumed: every output is zeros
      rc = glx_zero_f32_async(a.out, count, st.s);
      if (rc == GLX_OK) rc = glx_zero_f32_async(a.grad_s, s_count, st.s);
      if (rc == GLX_OK) rc = glx_zero_f32_async(d_gt, t_count, st.s);
    } else {
      const bool want_t = d_gt != nullptr && num_rows > 0;
      GlxAggTranspose tr;
      rc = glx_seg_layout_bwd(want_t, a.rows, cnt ? d_cnt : nullptr, num_ids, num_segments, num_rows, st.s, &lease, &tr,
                              &a.seg);
      if (rc == GLX_OK) {
        a.soft_out = nullptr;
        a.num_rows = num_rows;
        a.heads = heads;
        a.slope = negative_slope;
        a.default_attr = default_attr;
        a.drop = SmDropout(drop_p, seed, call);
        gat_launch<true>(a, drop_p != 0.0f, st.s);
        if (want_t) {
          const int64_t total = (int64_t)t_count;
          glx_gat_grad_t_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st.s>>>(tr.row_ptr, tr.pos, a.out, d_gt, total,
                                                                                 heads);
        }
      }
    }
  }
  return st.finish(rc);
}
