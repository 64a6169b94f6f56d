// The lane mapping that the per-segment normalisations share (glx_segment_softmax.hip, glx_gat_attention.hip): a
// group of G lanes owns one segment, a segment of more than kSmLongItems items is walked by the whole workgroup, and
// every reduction runs in a fixed tree -- the same inputs give the same bits on every call.
#ifndef GLX_SEGMENT_LANES_H_
#define GLX_SEGMENT_LANES_H_
#include "glx_common.h"

constexpr int kSmR = 4;                // items of a segment a lane keeps in registers between the passes
constexpr int kSmLongItems = 1024;     // a segment with more items than this is walked by the whole workgroup
constexpr int kSmTailBlocks = 1024;    // at most this many workgroups are launched for the unconsumed tail alone

struct SmMax {
  static __device__ __forceinline__ float op(float x, float y) { return fmaxf(x, y); }
};
struct SmAdd {
  static __device__ __forceinline__ float op(float x, float y) { return x + y; }
};

// over the lanes of a G-lane group whose distance is a multiple of min_off: every one of them ends with the same bits
// (both partners of an exchange compute the same commutative operation)
template <typename OP, int G>
__device__ __forceinline__ float sm_group_reduce(float x, int min_off) {
  for (int off = G >> 1; off >= min_off; off >>= 1) x = OP::op(x, __shfl_xor(x, off, G));
  return x;
}

// the same over the 256 threads of the workgroup, through LDS in a fixed tree; called by all 256 threads
template <typename OP>
__device__ __forceinline__ float sm_block_reduce(float x, int min_off, float* red) {
  const int tid = threadIdx.x;
  red[tid] = x;
  __syncthreads();
  for (int s = 128; s >= min_off; s >>= 1) {
    if (tid < s) red[tid] = OP::op(red[tid], red[tid + s]);
    __syncthreads();
  }
  const float r = red[tid & (min_off - 1)];
  __syncthreads();  // red is free again
  return r;
}

// the consumed positions [s0, s1) of segment sg; A carries seg_end (inclusive prefix sums of the clamped counts, or
// nullptr: the implied layout), fanout and num_ids
template <typename A>
__device__ __forceinline__ void sm_bounds(const A& a, int64_t sg, int32_t* s0, int32_t* s1) {
  int64_t b0, b1;
  if (a.seg_end) {
    b0 = sg ? a.seg_end[sg - 1] : 0;
    b1 = a.seg_end[sg];
  } else {
    b0 = sg * (int64_t)a.fanout;
    b1 = b0 + a.fanout;
  }
  if (b0 > a.num_ids) b0 = a.num_ids;  // counts that promise more positions than the request has are cut
  if (b1 > a.num_ids) b1 = a.num_ids;
  *s0 = (int32_t)b0;
  *s1 = (int32_t)b1;
}

// the first position that no segment consumed
template <typename A>
__device__ __forceinline__ int64_t sm_tail(const A& a) {
  if (a.seg_end) {
    const int64_t tail = a.seg_end[a.num_segments - 1];
    return tail > a.num_ids ? a.num_ids : tail;
  }
  return (int64_t)a.num_segments * a.fanout;
}

// the smallest group of 8 .. 64 lanes that covers `lanes`
inline int sm_group_for(int64_t lanes) { return lanes <= 8 ? 8 : lanes <= 16 ? 16 : lanes <= 32 ? 32 : 64; }

// The group width comes from the mean item count of a segment (the sizes alone: the counts live on the device).
// FLAT (heads a power of two <= 64): an item is one (position, head) and the group is at least `heads` wide;
// otherwise an item is one position and the heads are walked one after the other.
inline int sm_width(int32_t heads, int32_t num_ids, int32_t num_segments, bool* flat) {
  const int H = heads;
  *flat = H <= 64 && (H & (H - 1)) == 0;
  const int64_t items = *flat ? (int64_t)num_ids * H : (int64_t)num_ids;
  int G = sm_group_for((items + num_segments - 1) / num_segments);
  if (*flat && G < H) G = H;
  return G;
}

// workgroups of a launch: 256 / G segments each, and enough of them for a tail nobody consumed, should the segments
// be few and the request long
inline unsigned sm_blocks(int G, int32_t heads, int32_t num_ids, int32_t num_segments) {
  const int64_t seg_blocks = ((int64_t)num_segments + (256 / G) - 1) / (256 / G);
  int64_t tail_blocks = ((int64_t)num_ids * heads + 256 * 16 - 1) / (256 * 16);
  if (tail_blocks > kSmTailBlocks) tail_blocks = kSmTailBlocks;
  return (unsigned)(seg_blocks > tail_blocks ? seg_blocks : tail_blocks);
}

#endif  // GLX_SEGMENT_LANES_H_
