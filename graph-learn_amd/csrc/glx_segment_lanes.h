// The segment layout of a counts= request, and the lane mapping that the per-segment normalisations share
// (glx_segment_softmax.hip, glx_gat_attention.hip, glx_dot_attention.hip): a group of G lanes owns one segment, a segment of more than
// kSmLongItems items is walked by the whole workgroup, and every reduction runs in a fixed tree -- the same inputs give
// the same bits on every call.
#ifndef GLX_SEGMENT_LANES_H_
#define GLX_SEGMENT_LANES_H_
#include "glx_lane_groups.h"

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

// Dropout of element idx of a request under (seed, call): word idx & 3 of Philox block idx >> 2 (row 0); kept, and
// scaled, iff the word reaches thresh = floor(drop_p * 2^32).  The same function going forward and going back.
__device__ __forceinline__ float sm_dropout(float x, int32_t idx, uint32_t thresh, float scale, uint64_t seed,
                                            uint64_t call) {
  const GlxPhilox b = glx_philox_block((uint32_t)idx >> 2, 0u, seed, call);
  const int k = idx & 3;
  const uint32_t w = k == 0 ? b.w[0] : k == 1 ? b.w[1] : k == 2 ? b.w[2] : b.w[3];
  return w >= thresh ? x * scale : 0.0f;
}

// The ragged-or-implied layout of a counts= request: segment sg is positions [seg_end[sg - 1], seg_end[sg]) (seg_end:
// the inclusive prefix sums of the counts clamped at 0), or, with seg_end == nullptr, `fanout` positions each.  Counts
// that promise more positions than the request has are cut at num_ids; a position no segment reaches is not consumed.
struct GlxSegLayout {
  const int64_t* seg_end;  // [num_segments], or nullptr: the implied layout
  int32_t fanout, num_ids, num_segments;
};

// the consumed positions [s0, s1) of segment sg
__device__ __forceinline__ void seg_bounds(const GlxSegLayout& L, int64_t sg, int32_t* s0, int32_t* s1) {
  int64_t b0, b1;
  if (L.seg_end) {
    b0 = sg ? L.seg_end[sg - 1] : 0;
    b1 = L.seg_end[sg];
  } else {
    b0 = sg * (int64_t)L.fanout;
    b1 = b0 + L.fanout;
  }
  if (b0 > L.num_ids) b0 = L.num_ids;  // a cnt that promises more positions than the request has reads none of them
  if (b1 > L.num_ids) b1 = L.num_ids;
  *s0 = (int32_t)b0;
  *s1 = (int32_t)b1;
}

// s1 - s0 of seg_bounds, the positions of segment sg that the request really has: Mean's divisor
__device__ __forceinline__ int32_t seg_count(const GlxSegLayout& L, int32_t sg) {
  if (L.seg_end == nullptr) return L.fanout;
  int64_t b0 = sg ? L.seg_end[sg - 1] : 0, b1 = L.seg_end[sg];
  if (b0 > L.num_ids) b0 = L.num_ids;
  if (b1 > L.num_ids) b1 = L.num_ids;
  return (int32_t)(b1 - b0);
}

// the first position that no segment consumed
__device__ __forceinline__ int64_t seg_tail(const GlxSegLayout& L) {
  if (L.seg_end) {
    const int64_t tail = L.seg_end[L.num_segments - 1];
    return tail > L.num_ids ? L.num_ids : tail;
  }
  return (int64_t)L.num_segments * L.fanout;
}

// Is position p consumed?  *sg: its segment (0 when it is not) -- the first segment whose end lies beyond p, or
// p / fanout.  The answer depends on p alone, so the lanes of a group that share p agree on it.
__device__ __forceinline__ bool seg_of_position(const GlxSegLayout& L, int64_t p, int32_t* sg) {
  bool consumed;
  *sg = 0;
  if (L.seg_end) {
    consumed = p < L.seg_end[L.num_segments - 1];
    if (consumed) {
      int32_t lo = 0, hi = L.num_segments - 1;
      while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (L.seg_end[mid] > p) hi = mid; else lo = mid + 1;
      }
      *sg = lo;
    }
  } else {
    consumed = L.fanout > 0 && p / L.fanout < L.num_segments;
    if (consumed) *sg = (int32_t)(p / L.fanout);
  }
  return consumed;
}

// The layout of a request of num_segments >= 1 segments; d_cnt: the counts on the device, or nullptr.  A ragged request
// scans its counts into `lease` (workspace slot 1).
inline int glx_seg_layout(const int32_t* d_cnt, int32_t num_ids, int32_t num_segments, hipStream_t s, GlxScratch* lease,
                          GlxSegLayout* L) {
  L->seg_end = nullptr;
  L->fanout = num_ids / num_segments;
  L->num_ids = num_ids;
  L->num_segments = num_segments;
  return d_cnt ? glx_agg_segment_ends(d_cnt, num_segments, s, lease, &L->seg_end) : GLX_OK;
}

// The group width comes from the mean item count of a segment (the sizes alone: the counts live on the device).
// FLAT (heads a power of two <= 64): an item is one (position, head) and the group is at least `heads` wide;
// otherwise an item is one position and the heads are walked one after the other.
inline int sm_width(int32_t heads, int32_t num_ids, int32_t num_segments, bool* flat) {
  const int H = heads;
  *flat = H <= 64 && (H & (H - 1)) == 0;
  const int64_t items = *flat ? (int64_t)num_ids * H : (int64_t)num_ids;
  int G = glx_group_for((items + num_segments - 1) / num_segments);
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
