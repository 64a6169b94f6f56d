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
  float slope, default_attr, scale;
  uint32_t thresh;         // keep an element iff its word >= thresh
  uint64_t seed, call;
};

// s[sg, h] + t[rows[p], h]: one coalesced load of rows per item, a gather of the narrow table t
__device__ __forceinline__ float gat_pre(const GatArgs& a, float sv, int32_t p, int h) {
  const int64_t r = a.rows[p];
  const float tv = (r >= 0 && r < a.num_rows) ? a.t[r * a.heads + h] : a.default_attr;
  return sv + tv;
}

__device__ __forceinline__ float gat_leaky(float x, float pre, float slope) { return pre > 0.0f ? x : x * slope; }

// dropout of element idx = p * heads + h of the request: the same function going forward and going back
template <bool DROP>
__device__ __forceinline__ float gat_drop(const GatArgs& a, float x, int32_t idx) {
  return DROP ? sm_dropout(x, idx, a.thresh, a.scale, a.seed, a.call) : x;
}

// Item i of a segment that starts at position s0.  FLAT: the segment's [count, heads] block is one run and item i is
// element s0 * heads + i (position s0 + i / heads; the lane's head is fixed); otherwise item i is position s0 + i of
// head o.
template <bool FLAT>
struct GatItems {
  int32_t s0, H, o, hshift;
  __device__ __forceinline__ int32_t idx(int32_t i) const { return FLAT ? s0 * H + i : (s0 + i) * H + o; }
  __device__ __forceinline__ int32_t pos(int32_t i) const { return FLAT ? s0 + (i >> hshift) : s0 + i; }
};

// One (segment, head set) by a group of G lanes: lane c owns items c, c + G, ..; the first kSmR stay in registers,
// later ones park their logit, then their exponential, in alpha_out between the passes (the same lane writes and
// reads an element).
template <int G, bool FLAT, bool DROP>
__device__ __forceinline__ void gat_fwd_group(const GatArgs& a, const GatItems<FLAT>& it, float sv, int h, int32_t items,
                                              int min_off, int c) {
  float v[kSmR];
  float m = -INFINITY;
#pragma unroll
  for (int r = 0; r < kSmR; ++r) {
    const int32_t i = c + r * G;
    v[r] = -INFINITY;
    if (i < items) {
      const float pre = gat_pre(a, sv, it.pos(i), h);
      v[r] = gat_leaky(pre, pre, a.slope);
    }
    m = fmaxf(m, v[r]);
  }
  for (int32_t i = c + kSmR * G; i < items; i += G) {
    const float pre = gat_pre(a, sv, it.pos(i), h);
    const float e = gat_leaky(pre, pre, a.slope);
    a.out[it.idx(i)] = e;
    m = fmaxf(m, e);
  }
  m = sm_group_reduce<SmMax, G>(m, min_off);
  float sum = 0.0f;
#pragma unroll
  for (int r = 0; r < kSmR; ++r) {
    if (c + r * G < items) {
      v[r] = expf(v[r] - m);
      sum += v[r];
    }
  }
  for (int32_t i = c + kSmR * G; i < items; i += G) {
    const int32_t at = it.idx(i);
    const float x = expf(a.out[at] - m);
    a.out[at] = x;
    sum += x;
  }
  sum = sm_group_reduce<SmAdd, G>(sum, min_off);
#pragma unroll
  for (int r = 0; r < kSmR; ++r) {
    const int32_t i = c + r * G;
    if (i < items) {
      const int32_t at = it.idx(i);
      const float soft = v[r] / sum;
      if (a.soft_out) a.soft_out[at] = soft;
      a.out[at] = gat_drop<DROP>(a, soft, at);
    }
  }
  for (int32_t i = c + kSmR * G; i < items; i += G) {
    const int32_t at = it.idx(i);
    const float soft = a.out[at] / sum;
    if (a.soft_out) a.soft_out[at] = soft;
    a.out[at] = gat_drop<DROP>(a, soft, at);
  }
}

// Returns the group's sum of grad_e (the same bits in every lane of a head).
template <int G, bool FLAT, bool DROP>
__device__ __forceinline__ float gat_bwd_group(const GatArgs& a, const GatItems<FLAT>& it, float sv, int h, int32_t items,
                                               int min_off, int c) {
  float av[kSmR], gv[kSmR];
  float dot = 0.0f;
#pragma unroll
  for (int r = 0; r < kSmR; ++r) {
    const int32_t i = c + r * G;
    av[r] = gv[r] = 0.0f;
    if (i < items) {
      const int32_t at = it.idx(i);
      av[r] = a.soft[at];
      gv[r] = gat_drop<DROP>(a, a.g[at], at);
      dot += av[r] * gv[r];
    }
  }
  for (int32_t i = c + kSmR * G; i < items; i += G) {
    const int32_t at = it.idx(i);
    dot += a.soft[at] * gat_drop<DROP>(a, a.g[at], at);
  }
  dot = sm_group_reduce<SmAdd, G>(dot, min_off);
  float gs = 0.0f;
#pragma unroll
  for (int r = 0; r < kSmR; ++r) {
    const int32_t i = c + r * G;
    if (i < items) {
      const float ge = gat_leaky(av[r] * (gv[r] - dot), gat_pre(a, sv, it.pos(i), h), a.slope);
      a.out[it.idx(i)] = ge;
      gs += ge;
    }
  }
  for (int32_t i = c + kSmR * G; i < items; i += G) {
    const int32_t at = it.idx(i);
    const float d = a.soft[at] * (gat_drop<DROP>(a, a.g[at], at) - dot);
    const float ge = gat_leaky(d, gat_pre(a, sv, it.pos(i), h), a.slope);
    a.out[at] = ge;
    gs += ge;
  }
  return sm_group_reduce<SmAdd, G>(gs, min_off);
}

// A long segment by the whole workgroup: thread t owns items t, t + 256, ..
template <bool FLAT, bool DROP>
__device__ __forceinline__ void gat_fwd_block(const GatArgs& a, const GatItems<FLAT>& it, float sv, int h, int32_t items,
                                              int min_off, float* red) {
  const int tid = threadIdx.x;
  float m = -INFINITY;
  for (int32_t i = tid; i < items; i += 256) {
    const float pre = gat_pre(a, sv, it.pos(i), h);
    const float e = gat_leaky(pre, pre, a.slope);
    a.out[it.idx(i)] = e;
    m = fmaxf(m, e);
  }
  m = sm_block_reduce<SmMax>(m, min_off, red);
  float sum = 0.0f;
  for (int32_t i = tid; i < items; i += 256) {
    const int32_t at = it.idx(i);
    const float x = expf(a.out[at] - m);
    a.out[at] = x;
    sum += x;
  }
  sum = sm_block_reduce<SmAdd>(sum, min_off, red);
  for (int32_t i = tid; i < items; i += 256) {
    const int32_t at = it.idx(i);
    const float soft = a.out[at] / sum;
    if (a.soft_out) a.soft_out[at] = soft;
    a.out[at] = gat_drop<DROP>(a, soft, at);
  }
}

template <bool FLAT, bool DROP>
__device__ __forceinline__ float gat_bwd_block(const GatArgs& a, const GatItems<FLAT>& it, float sv, int h, int32_t items,
                                               int min_off, float* red) {
  const int tid = threadIdx.x;
  float dot = 0.0f;
  for (int32_t i = tid; i < items; i += 256) {
    const int32_t at = it.idx(i);
    dot += a.soft[at] * gat_drop<DROP>(a, a.g[at], at);
  }
  dot = sm_block_reduce<SmAdd>(dot, min_off, red);
  float gs = 0.0f;
  for (int32_t i = tid; i < items; i += 256) {
    const int32_t at = it.idx(i);
    const float d = a.soft[at] * (gat_drop<DROP>(a, a.g[at], at) - dot);
    const float ge = gat_leaky(d, gat_pre(a, sv, it.pos(i), h), a.slope);
    a.out[at] = ge;
    gs += ge;
  }
  return sm_block_reduce<SmAdd>(gs, min_off, red);
}

// The mapping of glx_segment_softmax_kernel: G lanes own one segment, a workgroup 256 / G consecutive segments; FLAT
// (heads a power of two <= G) reduces every head at once with strides G / 2 .. heads, otherwise head by head.  A
// segment of more than kSmLongItems items is left to the second phase, where the whole workgroup walks it.  Last, the
// workgroups share the positions nobody consumed: +0.0f.  No thread leaves before the end.
template <int G, bool FLAT, bool DROP, bool BWD>
__global__ __launch_bounds__(256) void glx_gat_attention_kernel(GatArgs a) {
  __shared__ float red[256];
  constexpr int kSegs = 256 / G;
  const int c = threadIdx.x & (G - 1);
  const int H = a.heads;
  const int min_off = FLAT ? H : 1;
  const int outer = FLAT ? 1 : H;
  const int64_t first = blockIdx.x * (int64_t)kSegs;
  GatItems<FLAT> it;
  it.H = H;
  it.s0 = 0;
  it.o = 0;
  it.hshift = FLAT ? __ffs(H) - 1 : 0;
  {
    const int64_t sg = first + threadIdx.x / G;
    if (sg < a.seg.num_segments) {  // the same answer in every lane of the group
      int32_t s0, s1;
      seg_bounds(a.seg, sg, &s0, &s1);
      const int64_t items = FLAT ? (int64_t)(s1 - s0) * H : (int64_t)(s1 - s0);
      it.s0 = s0;
      if (items > 0 && items <= kSmLongItems) {
        for (int o = 0; o < outer; ++o) {
          const int h = FLAT ? (c & (H - 1)) : o;
          const float sv = a.s[sg * H + h];
          it.o = o;
          if (BWD) {
            const float gs = gat_bwd_group<G, FLAT, DROP>(a, it, sv, h, (int32_t)items, min_off, c);
            if (a.grad_s && c < min_off) a.grad_s[sg * H + h] = gs;
          } else {
            gat_fwd_group<G, FLAT, DROP>(a, it, sv, h, (int32_t)items, min_off, c);
          }
        }
      } else if (BWD && items == 0 && a.grad_s) {  // an empty segment: +0.0f
        for (int h = c; h < H; h += G) a.grad_s[sg * H + h] = 0.0f;
      }
    }
  }
  for (int j = 0; j < kSegs; ++j) {  // every condition below is the same in all 256 threads
    const int64_t sg = first + j;
    if (sg >= a.seg.num_segments) break;
    int32_t s0, s1;
    seg_bounds(a.seg, sg, &s0, &s1);
    const int64_t items = FLAT ? (int64_t)(s1 - s0) * H : (int64_t)(s1 - s0);
    if (items <= kSmLongItems) continue;
    it.s0 = s0;
    for (int o = 0; o < outer; ++o) {
      const int h = FLAT ? ((int)threadIdx.x & (H - 1)) : o;
      const float sv = a.s[sg * H + h];
      it.o = o;
      if (BWD) {
        const float gs = gat_bwd_block<FLAT, DROP>(a, it, sv, h, (int32_t)items, min_off, red);
        if (a.grad_s && (int)threadIdx.x < min_off) a.grad_s[sg * H + h] = gs;
      } else {
        gat_fwd_block<FLAT, DROP>(a, it, sv, h, (int32_t)items, min_off, red);
      }
    }
  }
  const int64_t tail = seg_tail(a.seg);
  const int64_t end = (int64_t)a.seg.num_ids * H;
  for (int64_t i = tail * H + blockIdx.x * 256LL + threadIdx.x; i < end; i += gridDim.x * 256LL) {
    a.out[i] = 0.0f;
    if (!BWD && a.soft_out) a.soft_out[i] = 0.0f;
  }
}

template <bool FLAT, bool DROP, bool BWD>
void gat_launch_g(const GatArgs& a, int G, hipStream_t s) {
  const unsigned blocks = sm_blocks(G, a.heads, a.seg.num_ids, a.seg.num_segments);
  glx_for_group(G, [&](auto g) {
    glx_gat_attention_kernel<decltype(g)::value, FLAT, DROP, BWD><<<blocks, 256, 0, s>>>(a);
  });
}

template <bool BWD>
void gat_launch(const GatArgs& a, bool drop, hipStream_t s) {
  bool flat;
  const int G = sm_width(a.heads, a.seg.num_ids, a.seg.num_segments, &flat);
  if (flat) {
    if (drop) gat_launch_g<true, true, BWD>(a, G, s);
    else gat_launch_g<true, false, BWD>(a, G, s);
  } else {
    if (drop) gat_launch_g<false, true, BWD>(a, G, s);
    else gat_launch_g<false, false, BWD>(a, G, s);
  }
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

void gat_fill(GatArgs* a, int64_t num_rows, int32_t heads, float negative_slope, float default_attr, float drop_p,
              uint64_t seed, uint64_t call) {
  a->num_rows = num_rows;
  a->heads = heads;
  a->slope = negative_slope;
  a->default_attr = default_attr;
  a->scale = 1.0f / (1.0f - drop_p);
  a->thresh = (uint32_t)floor((double)drop_p * 4294967296.0);
  a->seed = seed;
  a->call = call;
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
        gat_fill(&a, num_rows, heads, negative_slope, default_attr, drop_p, seed, call);
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
      if (want_t) {  // the transpose computes the segment ends on its way: the layout takes them, it scans nothing
        rc = glx_agg_transpose(a.rows, d_cnt, num_ids, num_segments, num_rows, st.s, &lease, &tr);
        if (rc == GLX_OK) rc = glx_seg_layout(nullptr, num_ids, num_segments, st.s, &lease, &a.seg);
        if (rc == GLX_OK) a.seg.seg_end = tr.seg_end;
      } else {
        rc = glx_seg_layout(cnt ? d_cnt : nullptr, num_ids, num_segments, st.s, &lease, &a.seg);
      }
      if (rc == GLX_OK) {
        a.soft_out = nullptr;
        gat_fill(&a, num_rows, heads, negative_slope, default_attr, drop_p, seed, call);
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
