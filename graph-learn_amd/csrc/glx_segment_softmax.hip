// glx ragged segment softmax and its gradient: the normalisation of per-neighbour, per-head attention logits over the
// segments of a counts= request -- what the reference's GAT layer computes with unsorted_segment_softmax before its
// unsorted_segment_sum(nbr * alpha) (graphlearn/python/nn/tf/layers/gat_conv.py:101-112, nn/tf/utils/softmax.py:24-50).
//
// Contract (include/glx.h).  e[num_ids, heads] float32; segments as in glx_aggregate_weighted: the
// prefix sums of the clamped cnt cut at num_ids, or the implied layout of num_ids / num_segments positions each.
//   forward      for each (segment s, head h) over its k consumed positions: m = max e, t_p = expf(e_p - m),
//                alpha_p = t_p / sum_q t_q (no epsilon).  NaN or +inf among the logits, or all of them -inf: the whole
//                column is NaN (the NaN travels in the sum: e - m is NaN for that position, whatever fmaxf did to m)
//   backward     grad_e_p = alpha_p * (grad_alpha_p - sum_q alpha_q * grad_alpha_q)
// EVERY element of the output is written; a position that is not consumed gets +0.0f.  No atomics: each (s, h) is
// reduced by one lane group, or by one workgroup, with a fixed lane-to-element mapping and a fixed tree, so the same
// inputs give the same bits on every call.  The ORDER of the sums is the mapping's and not part of the contract.
#include "glx_segment_lanes.h"

namespace {

struct SmArgs {
  const float* a;          // forward: e; backward: alpha                 [num_ids, heads]
  const float* g;          // backward: grad_alpha; forward: unused       [num_ids, heads]
  GlxSegLayout seg;
  float* out;              // forward: alpha_out; backward: grad_e        [num_ids, heads]
  int32_t heads;
};

// One (segment, head set) by a group of G lanes.  The lane's items are base[i * stride], i = c, c + G, ..; the first
// kSmR of them stay in registers between the passes, later ones are read again (and the exponentials parked in out).
template <int G>
__device__ __forceinline__ void sm_fwd_group(const float* __restrict__ e, float* __restrict__ out, int32_t items,
                                             int32_t stride, int min_off, int c) {
  float v[kSmR];
  float m = -INFINITY;
#pragma unroll
  for (int r = 0; r < kSmR; ++r) {
    const int32_t i = c + r * G;
    v[r] = i < items ? e[i * stride] : -INFINITY;
    m = fmaxf(m, v[r]);
  }
  for (int32_t i = c + kSmR * G; i < items; i += G) m = fmaxf(m, e[i * stride]);
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
    const float t = expf(e[i * stride] - m);
    out[i * stride] = t;
    sum += t;
  }
  sum = sm_group_reduce<SmAdd, G>(sum, min_off);
#pragma unroll
  for (int r = 0; r < kSmR; ++r) {
    const int32_t i = c + r * G;
    if (i < items) out[i * stride] = v[r] / sum;
  }
  for (int32_t i = c + kSmR * G; i < items; i += G) out[i * stride] = out[i * stride] / sum;
}

template <int G>
__device__ __forceinline__ void sm_bwd_group(const float* __restrict__ alpha, const float* __restrict__ grad,
                                             float* __restrict__ out, int32_t items, int32_t stride, int min_off,
                                             int c) {
  float av[kSmR], gv[kSmR];
  float dot = 0.0f;
#pragma unroll
  for (int r = 0; r < kSmR; ++r) {
    const int32_t i = c + r * G;
    if (i < items) {
      av[r] = alpha[i * stride];
      gv[r] = grad[i * stride];
      dot += av[r] * gv[r];
    }
  }
  for (int32_t i = c + kSmR * G; i < items; i += G) dot += alpha[i * stride] * grad[i * stride];
  dot = sm_group_reduce<SmAdd, G>(dot, min_off);
#pragma unroll
  for (int r = 0; r < kSmR; ++r) {
    const int32_t i = c + r * G;
    if (i < items) out[i * stride] = av[r] * (gv[r] - dot);
  }
  for (int32_t i = c + kSmR * G; i < items; i += G) out[i * stride] = alpha[i * stride] * (grad[i * stride] - dot);
}

// A long segment by the whole workgroup: thread t owns items t, t + 256, ..; three passes over memory.
__device__ __forceinline__ void sm_fwd_block(const float* __restrict__ e, float* __restrict__ out, int64_t items,
                                             int32_t stride, int min_off, float* red) {
  const int tid = threadIdx.x;
  float m = -INFINITY;
  for (int64_t i = tid; i < items; i += 256) m = fmaxf(m, e[i * stride]);
  m = sm_block_reduce<SmMax>(m, min_off, red);
  float sum = 0.0f;
  for (int64_t i = tid; i < items; i += 256) {
    const float t = expf(e[i * stride] - m);
    out[i * stride] = t;
    sum += t;
  }
  sum = sm_block_reduce<SmAdd>(sum, min_off, red);
  for (int64_t i = tid; i < items; i += 256) out[i * stride] = out[i * stride] / sum;
}

__device__ __forceinline__ void sm_bwd_block(const float* __restrict__ alpha, const float* __restrict__ grad,
                                             float* __restrict__ out, int64_t items, int32_t stride, int min_off,
                                             float* red) {
  const int tid = threadIdx.x;
  float dot = 0.0f;
  for (int64_t i = tid; i < items; i += 256) dot += alpha[i * stride] * grad[i * stride];
  dot = sm_block_reduce<SmAdd>(dot, min_off, red);
  for (int64_t i = tid; i < items; i += 256) out[i * stride] = alpha[i * stride] * (grad[i * stride] - dot);
}

// G lanes own one segment; a workgroup owns 256 / G consecutive segments.
//   FLAT  (heads a power of two <= G)  the segment's [count, heads] block is one run of count * heads items; lane c
//         owns items c, c + G, .. -- all of head c % heads, because heads divides G -- and a butterfly with strides
//         G / 2 .. heads reduces every head at once.  Consecutive lanes read consecutive floats.
//   !FLAT (3, 6, .. heads, or more than 64)  head by head: for each head, lane c owns positions c, c + G, .. and the
//         whole group reduces.
// A segment of more than kSmLongItems items is left to the second phase, where the whole workgroup walks it (the same
// mapping with 256 lanes, reduced through LDS).  Last, the workgroups share the positions nobody consumed: +0.0f.
// No thread leaves before the end: the second phase synchronises the workgroup.
template <int G, bool FLAT, bool BWD>
__global__ __launch_bounds__(256) void glx_segment_softmax_kernel(SmArgs a) {
  __shared__ float red[256];
  constexpr int kSegs = 256 / G;
  const int c = threadIdx.x & (G - 1);
  const int H = a.heads;
  const int32_t stride = FLAT ? 1 : H;
  const int min_off = FLAT ? H : 1;
  const int outer = FLAT ? 1 : H;
  const int64_t first = blockIdx.x * (int64_t)kSegs;
  {
    const int64_t sg = first + threadIdx.x / G;
    if (sg < a.seg.num_segments) {  // the same answer in every lane of the group
      int32_t s0, s1;
      seg_bounds(a.seg, sg, &s0, &s1);
      const int64_t items = FLAT ? (int64_t)(s1 - s0) * H : (int64_t)(s1 - s0);
      if (items > 0 && items <= kSmLongItems) {
        for (int o = 0; o < outer; ++o) {
          const int64_t at = (int64_t)s0 * H + o;
          if (BWD) sm_bwd_group<G>(a.a + at, a.g + at, a.out + at, (int32_t)items, stride, min_off, c);
          else sm_fwd_group<G>(a.a + at, a.out + at, (int32_t)items, stride, min_off, c);
        }
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
    for (int o = 0; o < outer; ++o) {
      const int64_t at = (int64_t)s0 * H + o;
      if (BWD) sm_bwd_block(a.a + at, a.g + at, a.out + at, items, stride, min_off, red);
      else sm_fwd_block(a.a + at, a.out + at, items, stride, min_off, red);
    }
  }
  const int64_t tail = seg_tail(a.seg);
  const int64_t end = (int64_t)a.seg.num_ids * H;
  for (int64_t i = tail * H + blockIdx.x * 256LL + threadIdx.x; i < end; i += gridDim.x * 256LL) a.out[i] = 0.0f;
}

template <bool FLAT, bool BWD>
void sm_launch_g(const SmArgs& a, int G, hipStream_t s) {
  const unsigned blocks = sm_blocks(G, a.heads, a.seg.num_ids, a.seg.num_segments);
  glx_for_group(G, [&](auto g) {
    glx_segment_softmax_kernel<decltype(g)::value, FLAT, BWD><<<blocks, 256, 0, s>>>(a);
  });
}

// the group width and the item mapping: sm_width (glx_segment_lanes.h)
template <bool BWD>
void sm_launch(const SmArgs& a, hipStream_t s) {
  bool flat;
  const int G = sm_width(a.heads, a.seg.num_ids, a.seg.num_segments, &flat);
  if (flat) sm_launch_g<true, BWD>(a, G, s);
  else sm_launch_g<false, BWD>(a, G, s);
}

// the body both entry points share, behind their argument checks
int sm_run(int device, bool bwd, const float* in0, const float* in1, int32_t heads, const int32_t* cnt, int32_t num_ids,
           int32_t num_segments, float* out, int ptr_kind, void* stream) {
  int rc = glx_init_device(device);
  if (rc != GLX_OK) return rc;
  if (num_ids == 0) return GLX_OK;
  GlxDeviceGuard guard(device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", device);
  GlxHostStage st(device, ptr_kind, stream, GlxHostStage::ADMIT);
  SmArgs a;
  const int32_t* d_cnt;
  const size_t count = (size_t)num_ids * heads;
  st.in(&a.a, in0, count);
  a.g = nullptr;
  if (bwd) st.in(&a.g, in1, count);
  st.in(&d_cnt, cnt, (size_t)num_segments);
  st.out(&a.out, out, count);
  rc = st.begin();
  GlxScratch lease;
  if (rc == GLX_OK) {
    if (num_segments == 0) {  // nothing was consumed
      rc = glx_zero_f32_async(a.out, count, st.s);
    } else {
      rc = glx_seg_layout(cnt ? d_cnt : nullptr, num_ids, num_segments, st.s, &lease, &a.seg);
      if (rc == GLX_OK) {
        a.heads = heads;
        if (bwd) sm_launch<true>(a, st.s);
        else sm_launch<false>(a, st.s);
      }
    }
  }
  return st.finish(rc);
}

}  // namespace

// what the two entry points check alike, before any device use
#define GLX_SOFTMAX_REQUIRE()                                                                \
  GLX_REQUIRE(num_ids >= 0 && num_segments >= 0, "negative sizes");                          \
  GLX_REQUIRE(heads > 0, "heads must be positive, got %d", heads);                           \
  GLX_REQUIRE((int64_t)num_ids * heads <= INT32_MAX, "num_ids * heads exceeds int32");       \
  GLX_REQUIRE(ptr_kind == GLX_PTR_HOST || ptr_kind == GLX_PTR_DEVICE, "bad ptr_kind")

extern "C" int glx_segment_softmax(int device, const float* e, int32_t heads, const int32_t* cnt, int32_t num_ids,
                                   int32_t num_segments, float* alpha_out, int ptr_kind, void* stream) {
  GLX_SOFTMAX_REQUIRE();
  GLX_REQUIRE(num_ids == 0 || e != nullptr, "e is NULL");
  GLX_REQUIRE(num_ids == 0 || alpha_out != nullptr, "alpha_out is NULL");
  return sm_run(device, false, e, nullptr, heads, cnt, num_ids, num_segments, alpha_out, ptr_kind, stream);
}

extern "C" int glx_segment_softmax_backward(int device, const float* alpha, const float* grad_alpha, int32_t heads,
                                            const int32_t* cnt, int32_t num_ids, int32_t num_segments, float* grad_e,
                                            int ptr_kind, void* stream) {
  GLX_SOFTMAX_REQUIRE();
  GLX_REQUIRE(num_ids == 0 || alpha != nullptr, "alpha is NULL");
  GLX_REQUIRE(num_ids == 0 || grad_alpha != nullptr, "grad_alpha is NULL");
  GLX_REQUIRE(num_ids == 0 || grad_e != nullptr, "grad_e is NULL");
  return sm_run(device, true, alpha, grad_alpha, heads, cnt, num_ids, num_segments, grad_e, ptr_kind, stream);
}
