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

// What sm_forward / sm_backward (glx_segment_lanes.h) read and write here: item i of the (segment, head set) is element
// i * stride from its first one.  a: the logits e going forward, alpha going back.  Forward: pass 2 reads e again, it
// parks no logit; a spilled item's exponential is parked in out.
struct SmIo {
  const float* a;
  const float* g;
  float* out;
  int32_t stride;
  static constexpr bool kSum = false;
  template <typename I> __device__ __forceinline__ float logit(I i) const { return a[i * stride]; }
  template <typename I> __device__ __forceinline__ float spill_logit(I i) const { return logit(i); }
  template <typename I> __device__ __forceinline__ float parked_logit(I i) const { return logit(i); }
  template <typename I> __device__ __forceinline__ void park_exp(I i, float t) const { out[i * stride] = t; }
  template <typename I> __device__ __forceinline__ float parked_exp(I i) const { return out[i * stride]; }
  template <typename I> __device__ __forceinline__ void emit_soft(I i, float soft) const { out[i * stride] = soft; }
  template <typename I> __device__ __forceinline__ float soft(I i) const { return a[i * stride]; }
  template <typename I> __device__ __forceinline__ float grad(I i) const { return g[i * stride]; }
  template <typename I> __device__ __forceinline__ float emit_grad(I i, float, float d) const { return out[i * stride] = d; }
};

// One (segment, head set) from its first element on.  The inputs never alias the output: the loads of a later item
// may pass the stores of an earlier one.
template <bool BWD, typename W>
__device__ __forceinline__ void sm_one(const W& w, const SmItems& it, const float* __restrict__ a,
                                       const float* __restrict__ g, float* __restrict__ out) {
  const SmIo io = {a, g, out, it.flat ? 1 : it.H};
  if (BWD) sm_backward(w, it, io);
  else sm_forward(w, it, io);
}

// sm_segment_walk's mapping (glx_segment_lanes.h): G lanes own one segment; a workgroup owns 256 / G consecutive ones.
//   FLAT  (heads a power of two <= G)  the segment's [count, heads] block is one run of count * heads items; lane c
//         owns items c, c + G, .. -- all of head c % heads, because heads divides G -- and a butterfly with strides
//         G / 2 .. heads reduces every head at once.  Consecutive lanes read consecutive floats.
//   !FLAT (3, 6, .. heads, or more than 64)  head by head: for each head, lane c owns positions c, c + G, .. and the
//         whole group reduces.
// A segment of more than kSmLongItems items is left to the second phase, where the whole workgroup walks it (the same
// mapping with 256 lanes, reduced through LDS).  Last, the workgroups share the positions nobody consumed: +0.0f.
template <int G, bool FLAT, bool BWD>
__global__ __launch_bounds__(256) void glx_segment_softmax_kernel(SmArgs a) {
  __shared__ float red[256];
  sm_segment_walk<G>(
      a.seg, a.heads, FLAT, red,
      [&](const auto& w, const SmItems& it, int64_t) {
        const int32_t at = it.idx(0);
        sm_one<BWD>(w, it, a.a + at, BWD ? a.g + at : nullptr, a.out + at);
      },
      [](int64_t, int) {}, [&](int64_t i) { a.out[i] = 0.0f; });
}

// the group width and the item mapping: sm_width (glx_segment_lanes.h)
template <bool BWD>
void sm_launch(const SmArgs& a, hipStream_t s) {
  sm_for_launch(a.heads, a.seg, [&](auto g, auto flat, unsigned blocks) {
    glx_segment_softmax_kernel<decltype(g)::value, decltype(flat)::value, BWD><<<blocks, 256, 0, s>>>(a);
  });
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
