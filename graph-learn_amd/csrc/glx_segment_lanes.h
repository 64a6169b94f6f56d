// The segment layout of a counts= request, and the per-segment softmax that glx_segment_softmax.hip,
// glx_gat_attention.hip and glx_dot_attention.hip share -- the lane mapping, the order of operations (sm_forward,
// sm_backward) and the walk over the segments (sm_segment_walk): a group of G lanes owns one segment, a segment of more
// than kSmLongItems items is walked by the whole workgroup, and every reduction runs in a fixed tree -- the same inputs
// give the same bits on every call.  A kernel supplies only where a logit comes from and where a value goes (its io).
#ifndef GLX_SEGMENT_LANES_H_
#define GLX_SEGMENT_LANES_H_
#include "glx_lane_groups.h"

constexpr int kSmR = 4;                // items of a segment a lane keeps in registers between the passes
constexpr int kSmLongItems = 1024;     // a segment with more items than this is walked by the whole workgroup
constexpr int kSmTailBlocks = 1024;    // at most this many workgroups are launched for the unconsumed tail alone

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
// scans its counts into `lease` (kSlotRequest of GlxTrainSlot, glx_chunks.h).
inline int glx_seg_layout(const int32_t* d_cnt, int32_t num_ids, int32_t num_segments, hipStream_t s, GlxScratch* lease,
                          GlxSegLayout* L) {
  L->seg_end = nullptr;
  L->fanout = num_ids / num_segments;
  L->num_ids = num_ids;
  L->num_segments = num_segments;
  return d_cnt ? glx_agg_segment_ends(d_cnt, num_segments, s, lease, &L->seg_end) : GLX_OK;
}

// The layout of a request whose transpose the caller holds: the transpose computed the segment ends on its way.
inline GlxSegLayout glx_seg_layout_of(const GlxAggTranspose& t, int32_t num_ids, int32_t num_segments) {
  return GlxSegLayout{t.seg_end, t.fanout, num_ids, num_segments};
}

// The layout of a backward request that may want the gradient of its rows as well: with want_rows the transpose goes
// into `lease` and the layout takes its segment ends, it scans nothing; otherwise glx_seg_layout.
inline int glx_seg_layout_bwd(bool want_rows, const int64_t* d_rows, const int32_t* d_cnt, int32_t num_ids,
                              int32_t num_segments, int64_t num_rows, hipStream_t s, GlxScratch* lease,
                              GlxAggTranspose* t, GlxSegLayout* L) {
  if (!want_rows) return glx_seg_layout(d_cnt, num_ids, num_segments, s, lease, L);
  const int rc = glx_agg_transpose(d_rows, d_cnt, num_ids, num_segments, num_rows, s, lease, t);
  if (rc == GLX_OK) *L = glx_seg_layout_of(*t, num_ids, num_segments);
  return rc;
}

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

// Who owns the items of a segment.  A group of G lanes: lane c owns items c, c + G, .. and keeps the first kSmR of them
// in registers between the passes.
template <int G>
struct SmGroupWalker {
  static constexpr int kRegs = kSmR, kStep = G;
  typedef int32_t Index;
  int c;
  __device__ __forceinline__ int lane() const { return c; }
  template <typename OP>
  __device__ __forceinline__ float reduce(float x, int min_off) const { return sm_group_reduce<OP, G>(x, min_off); }
};

// The whole workgroup (a long segment): thread t owns items t, t + 256, .. and keeps none of them; every reduce is
// called by all 256 threads.
struct SmBlockWalker {
  static constexpr int kRegs = 0, kStep = 256;
  typedef int64_t Index;  // as long as the walk is long: no step past the last item overflows
  float* red;  // 256 floats of LDS
  __device__ __forceinline__ int lane() const { return threadIdx.x; }
  template <typename OP>
  __device__ __forceinline__ float reduce(float x, int min_off) const { return sm_block_reduce<OP>(x, min_off, red); }
};

// The items of one segment [s0, s1) of a request of H heads.  flat (H a power of two no wider than the group): the
// segment's [count, H] block is one run, item i is element s0 * H + i (position s0 + i / H), a lane's items share its
// head `lane % H`, and a reduce with min_off = H folds every head at once.  Otherwise head by head (o = 0 .. outer):
// item i is position s0 + i of head o.
struct SmItems {
  int32_t s0, H, o, hshift, items, min_off, outer;
  bool flat;
  __device__ __forceinline__ int32_t idx(int32_t i) const { return flat ? s0 * H + i : (s0 + i) * H + o; }
  __device__ __forceinline__ int32_t pos(int32_t i) const { return flat ? s0 + (i >> hshift) : s0 + i; }
};

__device__ __forceinline__ SmItems sm_items(bool flat, int32_t s0, int32_t s1, int32_t H) {
  SmItems it;
  it.flat = flat;
  it.s0 = s0;
  it.H = H;
  it.o = 0;
  it.hshift = flat ? __ffs(H) - 1 : 0;
  it.items = flat ? (s1 - s0) * H : s1 - s0;  // at most num_ids * heads: int32
  it.min_off = flat ? H : 1;
  it.outer = flat ? 1 : H;
  return it;
}

// THE softmax of one (segment, head set), K5-sm's definition: m = max v, t = expf(v - m), soft = t / sum t, in this
// order of operations -- the walker's register items r = 0 .. kRegs - 1, then its spilled items in ascending i.  io:
//   logit(i)         the logit of a register item
//   spill_logit(i)   the logit of a spilled item, which io may park for pass 2
//   parked_logit(i)  that logit again in pass 2
//   park_exp(i, t) / parked_exp(i)   a spilled item's exponential between passes 2 and 3
//   emit_soft(i, soft)   the finished value
// A lane parks and reads back its own items only.
template <typename W, typename IO>
__device__ __forceinline__ void sm_forward(const W& w, const SmItems& it, const IO& io) {
  constexpr int R = W::kRegs, S = W::kStep;
  const int c = w.lane();
  const int32_t items = it.items;
  float v[R ? R : 1];
  float m = -INFINITY;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int32_t i = c + r * S;
    v[r] = i < items ? io.logit(i) : -INFINITY;
    m = fmaxf(m, v[r]);
  }
  for (typename W::Index i = c + R * S; i < items; i += S) m = fmaxf(m, io.spill_logit(i));
  m = w.template reduce<SmMax>(m, it.min_off);
  float sum = 0.0f;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (c + r * S < items) {
      v[r] = expf(v[r] - m);
      sum += v[r];
    }
  }
  for (typename W::Index i = c + R * S; i < items; i += S) {
    const float t = expf(io.parked_logit(i) - m);
    io.park_exp(i, t);
    sum += t;
  }
  sum = w.template reduce<SmAdd>(sum, it.min_off);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int32_t i = c + r * S;
    if (i < items) io.emit_soft(i, v[r] / sum);
  }
  for (typename W::Index i = c + R * S; i < items; i += S) io.emit_soft(i, io.parked_exp(i) / sum);
}

// Its gradient: dot = sum soft * g, d = soft * (g - dot), in the same item order.  io: soft(i); grad(i), the incoming
// gradient (which may re-apply dropout); emit_grad(i, soft_i, d_i), which returns what it wrote.  IO::kSum: return the sum
// of what emit_grad returned, reduced like the rest (the same bits in every lane of a head); otherwise 0.0f.
template <typename W, typename IO>
__device__ __forceinline__ float sm_backward(const W& w, const SmItems& it, const IO& io) {
  constexpr int R = W::kRegs, S = W::kStep;
  const int c = w.lane();
  const int32_t items = it.items;
  float av[R ? R : 1], gv[R ? R : 1];
  float dot = 0.0f;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int32_t i = c + r * S;
    av[r] = gv[r] = 0.0f;
    if (i < items) {
      av[r] = io.soft(i);
      gv[r] = io.grad(i);
      dot += av[r] * gv[r];
    }
  }
  for (typename W::Index i = c + R * S; i < items; i += S) dot += io.soft(i) * io.grad(i);
  dot = w.template reduce<SmAdd>(dot, it.min_off);
  float gs = 0.0f;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int32_t i = c + r * S;
    if (i < items) gs += io.emit_grad(i, av[r], av[r] * (gv[r] - dot));
  }
  for (typename W::Index i = c + R * S; i < items; i += S) {
    const float a = io.soft(i);
    gs += io.emit_grad(i, a, a * (io.grad(i) - dot));
  }
  return IO::kSum ? w.template reduce<SmAdd>(gs, it.min_off) : 0.0f;
}

// The walk of glx_segment_softmax_kernel and glx_gat_attention_kernel over a request of H heads: G lanes own one
// segment, a workgroup 256 / G consecutive segments.
//   1  body(SmGroupWalker<G>, items, sg) for each head set (items.o) of the group's segment, unless it is empty --
//      empty(sg, c) -- or has more than kSmLongItems items
//   2  body(SmBlockWalker, items, sg) for each of those long segments, by the whole workgroup: every condition is the
//      same in all 256 threads
//   3  fill(i) for every element i of the [num_ids, H] positions nobody consumed, shared by the workgroups
// No thread leaves before the end: the second phase synchronises the workgroup.  red: 256 floats of LDS.
template <int G, typename BODY, typename EMPTY, typename FILL>
__device__ __forceinline__ void sm_segment_walk(const GlxSegLayout& seg, int32_t H, bool flat, float* red, BODY&& body,
                                                EMPTY&& empty, FILL&& fill) {
  constexpr int kSegs = 256 / G;
  const int64_t first = blockIdx.x * (int64_t)kSegs;
  {
    const SmGroupWalker<G> w = {(int)threadIdx.x & (G - 1)};
    const int64_t sg = first + threadIdx.x / G;
    if (sg < seg.num_segments) {  // the same answer in every lane of the group
      int32_t s0, s1;
      seg_bounds(seg, sg, &s0, &s1);
      SmItems it = sm_items(flat, s0, s1, H);
      if (it.items > 0 && it.items <= kSmLongItems) {
        for (it.o = 0; it.o < it.outer; ++it.o) body(w, it, sg);
      } else if (it.items == 0) {
        empty(sg, w.c);
      }
    }
  }
  const SmBlockWalker w = {red};
  // The four segments of 64-lane groups are unrolled, so that their bounds load together: left to itself the compiler
  // does so for one instance in 48 only, and a request without long segments pays four dependent loads otherwise.
  constexpr int kUnroll = kSegs <= 4 ? kSegs : 1;
#pragma unroll kUnroll
  for (int j = 0; j < kSegs; ++j) {  // every condition below is the same in all 256 threads
    const int64_t sg = first + j;
    if (sg >= seg.num_segments) break;
    int32_t s0, s1;
    seg_bounds(seg, sg, &s0, &s1);
    SmItems it = sm_items(flat, s0, s1, H);
    if (it.items <= kSmLongItems) continue;
    for (it.o = 0; it.o < it.outer; ++it.o) body(w, it, sg);
  }
  const int64_t end = (int64_t)seg.num_ids * H;
  for (int64_t i = seg_tail(seg) * H + blockIdx.x * 256LL + threadIdx.x; i < end; i += gridDim.x * 256LL) fill(i);
}

// Dropout under (seed, call): element idx of a request draws word idx & 3 of Philox block idx >> 2 (row 0) and is kept,
// and scaled, iff the word reaches thresh = floor(drop_p * 2^32), scale = 1.0f / (1.0f - drop_p).
struct SmDropout {
  uint32_t thresh;
  float scale;
  uint64_t seed, call;
  SmDropout() = default;
  SmDropout(float drop_p, uint64_t seed_, uint64_t call_)
      : thresh((uint32_t)floor((double)drop_p * 4294967296.0)), scale(1.0f / (1.0f - drop_p)), seed(seed_), call(call_) {}
};

// The same function going forward and going back.
__device__ __forceinline__ float sm_dropout(float x, int32_t idx, const SmDropout& d) {
  const GlxPhilox b = glx_philox_block((uint32_t)idx >> 2, 0u, d.seed, d.call);
  const int k = idx & 3;
  const uint32_t w = k == 0 ? b.w[0] : k == 1 ? b.w[1] : k == 2 ? b.w[2] : b.w[3];
  return w >= d.thresh ? x * d.scale : 0.0f;
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

// launch(g, flat, blocks) with sm_width's group width and mapping as integral constants (a kernel template takes
// decltype(g)::value and decltype(flat)::value) and sm_blocks' workgroups
template <typename F>
inline void sm_for_launch(int32_t heads, const GlxSegLayout& seg, F&& launch) {
  bool flat;
  const int G = sm_width(heads, seg.num_ids, seg.num_segments, &flat);
  const unsigned blocks = sm_blocks(G, heads, seg.num_ids, seg.num_segments);
  glx_for_group(G, [&](auto g) {
    if (flat) launch(g, std::true_type(), blocks);
    else launch(g, std::false_type(), blocks);
  });
}

#endif  // GLX_SEGMENT_LANES_H_
