// glx node features + segmented aggregation (Sum/Mean/Max/Min/Prod) + lookup.
// Replaces graphlearn/src/core/operator/aggregator/{aggregator.cc:25-86,
// sum_aggregator.cc:25-33, mean_aggregator.cc:26-61, max_aggregator.cc:26-40,
// min_aggregator.cc, prod_aggregator.cc} and the GetAttribute()->GetFloats()
// reads behind them (memory_node_storage.cc:127-138).
//
// SpMM-shaped but HBM-bound (0.25 flop/byte): the design goal is to keep many
// independent 16-byte row loads in flight per lane and to touch every feature
// byte once.  A group of G lanes owns one segment and walks its rows in the
// reference's order; lane c of the group owns columns [4c, 4c+4) so each output
// element is accumulated left-to-right exactly like the reference's serial loop
// (bit-identical results, no cross-lane reduction at all).
#include <float.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <new>
#include <type_traits>

#include "glx_common.h"

namespace {

// ---- segment bookkeeping ---------------------------------------------------
// AggregatingRequest's cursor (aggregating_request.cc:86-105) consumes ids in
// order and hands id c to segment segment_ids[c] only while the sequence stays
// non-decreasing and inside [0, num_segments); the first violation stalls the
// cursor for good.  valid_len = index of that first violation.
//
// One streaming pass over segment_ids does all of it (round 5; rounds 1-4 ran a validity pass and then one binary
// search per segment -- 24 dependent loads each -- which cost 0.1 ms on the headline's 16.4 M ids, 5 % of the step):
//   valid_len
//   level = 0  when the request is what a dense sampler response implies -- segment s = ids [s f, (s + 1) f),
//              f = n / num_segments -- and the reduce may use arithmetic segment bounds (no seg_start read);
//           1  when the reduce must read seg_start;
//           2  when the scan left seg_start incomplete and glx_seg_fixup_kernel fills it (the reduce reads it too)
//   seg_start[s] = lower_bound(seg[0..valid_len), s), s in [0, num_segments]: position i writes it for every s in
//                  (seg[i - 1], seg[i]] (the last position for the segments after seg[n - 1]).
// A violation, or a run of more than kSegRunMax empty segments (one thread would write them all), leaves the rest
// to the fix-up kernel: the old binary search, which exits at once otherwise.
// valid_len and level live in two 64-bit words of a small per-stream buffer, each tagged with the call's epoch in its
// high half and raised with atomicMax: a word whose tag is not this call's reads as "nothing raised", so no launch is
// spent on resetting them (a launch costs as much as the whole scan of a small request).
constexpr int32_t kSegRunMax = 64;

// (SegState, seg_level and seg_valid_len live in glx_common.h: glx_aggregate_grad.hip reads the same words)

__global__ void glx_seg_reset_kernel(unsigned long long* words) {  // captured launches only (see prepare_segments)
  words[0] = 0;
  words[1] = 0;
}

// The scan's partition of a request (round 25; tests/test_seg_scan_partition_cpu.py restates it).  A workgroup walks the
// request grid-stride in TILES of kSegScanTile ids.  Within a tile a thread issues kSegScanLoads independent 16-byte
// loads before it uses any: load instruction L of the tile covers the ids [L kSegScanSpan, (L + 1) kSegScanSpan) of the
// tile, thread t its quad [4 t, 4 t + 4) of those, so consecutive lanes read consecutive 16 bytes and a wave reads 1 KiB
// per instruction, 4 KiB per tile.  The id before a quad comes from the lane below (a cross-lane read of its last id);
// only lane 0 of a wave loads it from memory, once per load instruction.  The tile at the end of the request, and every
// tile of a `seg` that is not 16-byte aligned, loads its ids one by one (the same partition, the same cross-lane read).
constexpr int kSegScanThreads = 256;
constexpr int kSegScanLoads = 4;
constexpr int32_t kSegScanSpan = kSegScanThreads * 4;
constexpr int32_t kSegScanTile = kSegScanSpan * kSegScanLoads;
constexpr int kSegScanWgPerCu = 8;  // grid = this many workgroups per CU of the device at most: every wave slot, once

// (quo, rem) = (i / f, i % f) of a position, moved on by a distance whose own (d / f, d % f) the caller holds:
// no division per id, one per thread for the start and two (uniform) for the distances
__device__ __forceinline__ void seg_counters_advance(uint32_t& quo, uint32_t& rem, uint32_t dq, uint32_t dr, uint32_t f) {
  quo += dq;
  rem += dr;  // < 2 f <= 2^32 - 2
  if (rem >= f) {
    rem -= f;
    ++quo;
  }
}

// what a thread carries from tile to tile: the counters of its next quad with the distances that move them on, and what it
// found so far (raised once per wave behind the walk)
struct SegScanCarry {
  uint32_t quo, rem, span_q, span_r, wrap_q, wrap_r;  // unused when f == 0
  int32_t level, bad_at;
};

// One tile.  WHOLE: every quad of the tile is inside the request and `seg` is 16-byte aligned -- one 16-byte load per
// quad; else id by id.  (Two instantiations, not a branch per load: behind a branch the compiler waited for each load
// where the two sides met, and the loads of a tile went out one after the other.)
template <bool WHOLE>
__device__ __forceinline__ void seg_scan_tile(const int32_t* __restrict__ seg, int32_t n, int32_t num_segments, int32_t f,
                                              int64_t t0, int lane, SegScanCarry& c, int32_t* __restrict__ seg_start) {
  const uint32_t uf = (uint32_t)f;
  int32_t v[kSegScanLoads][4], below[kSegScanLoads];
#pragma unroll
  for (int L = 0; L < kSegScanLoads; ++L) {
    const int64_t i0 = t0 + L * kSegScanSpan + threadIdx.x * 4;
    if (WHOLE) {
      const int4 q = *reinterpret_cast<const int4*>(seg + i0);
      v[L][0] = q.x; v[L][1] = q.y; v[L][2] = q.z; v[L][3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[L][j] = i0 + j < n ? seg[i0 + j] : 0;
    }
    below[L] = (lane == 0 && i0 > 0 && i0 < n) ? seg[i0 - 1] : -1;  // -1 before the first id of the request
  }
#pragma unroll
  for (int L = 0; L < kSegScanLoads; ++L) {
    const int64_t i0 = t0 + L * kSegScanSpan + threadIdx.x * 4;
    const int32_t m = i0 >= n ? 0 : ((n - i0) < 4 ? (int32_t)(n - i0) : 4);
    // every lane takes part in the cross-lane read; a quad that has ids has a full quad in the lane below
    const int32_t from_lane = __shfl_up(v[L][3], 1);
    int32_t prev = lane == 0 ? below[L] : from_lane;
    // the id before this quad is itself out of range: a violation at or before it (its own quad reports it), so
    // nothing from here on belongs to the request -- and `prev` is no segment to count on from.  The quad writes and
    // reports nothing; the thread stays for its later tiles and for the wave's ballots.
    const bool live = m > 0 && !(i0 > 0 && (prev < 0 || prev >= num_segments));
    // The quad nearly every quad is: behind an id in range, every id its predecessor or the segment after it, and not
    // the request's last.  Then no id is out of range (prev <= v0 <= .. <= v3 < num_segments), no run is long, and a
    // position writes at most its own segment's entry -- straight-line code, four predicated stores.  (The general
    // code below ran a loop per id and a loop per entry: round 25's trace showed the scan bound by the instructions
    // it issues, some 400 per quad, not by its bytes or its wave count.)
    const uint32_t d0 = (uint32_t)v[L][0] - (uint32_t)prev, d1 = (uint32_t)v[L][1] - (uint32_t)v[L][0],
                   d2 = (uint32_t)v[L][2] - (uint32_t)v[L][1], d3 = (uint32_t)v[L][3] - (uint32_t)v[L][2];
    const bool plain = (uint32_t)prev < (uint32_t)num_segments && (uint32_t)v[L][3] < (uint32_t)num_segments &&
                       (d0 | d1 | d2 | d3) <= 1u && i0 + 4 < n;
    if (plain) {
      const int32_t i = (int32_t)i0;
      if (d0) seg_start[v[L][0]] = i;
      if (d1) seg_start[v[L][1]] = i + 1;
      if (d2) seg_start[v[L][2]] = i + 2;
      if (d3) seg_start[v[L][3]] = i + 3;
      if (f > 0) {
        uint32_t q = c.quo, r = c.rem;
        bool nonuniform = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          nonuniform |= (uint32_t)v[L][j] != q;
          const bool wraps = ++r == uf;
          q += wraps ? 1u : 0u;
          r = wraps ? 0u : r;
        }
        if (nonuniform && c.level < 1) c.level = 1;
      }
    } else if (live) {
      uint32_t q = c.quo, r = c.rem;  // i / f and i % f, carried along
      bool nonuniform = false, incomplete = false;
      int32_t bad = n;
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // unrolled: v[L][j] stays a register, not an indexed copy of the tile
        if (j >= m) break;
        const int32_t i = (int32_t)i0 + j, cur = v[L][j];
        if (cur < 0 || cur >= num_segments || cur < prev) {  // prev == -1 before the first id
          bad = i;
          break;
        }
        if (cur != prev) {
          if (cur - prev > kSegRunMax) incomplete = true;
          else for (int32_t s = prev + 1; s <= cur; ++s) seg_start[s] = i;
        }
        if (f > 0) {
          nonuniform |= (uint32_t)cur != q;
          if (++r == uf) { r = 0; ++q; }
        }
        prev = cur;
      }
      if (bad == n && i0 + m == n) {  // the last ids: the segments after the last one used start (and end) at n
        if (num_segments - prev > kSegRunMax) incomplete = true;
        else for (int32_t s = prev + 1; s <= num_segments; ++s) seg_start[s] = n;
      }
      if (bad < c.bad_at) c.bad_at = bad;
      const int32_t here = (incomplete || bad < n) ? 2 : (nonuniform ? 1 : 0);
      if (here > c.level) c.level = here;
    }
    if (f > 0) {
      if (L + 1 < kSegScanLoads) seg_counters_advance(c.quo, c.rem, c.span_q, c.span_r, uf);
      else seg_counters_advance(c.quo, c.rem, c.wrap_q, c.wrap_r, uf);
    }
  }
}

__global__ __launch_bounds__(kSegScanThreads) void glx_seg_scan_kernel(const int32_t* __restrict__ seg, int32_t n,
                                                                       int32_t num_segments, int32_t f,
                                                                       unsigned long long* __restrict__ words, uint32_t epoch,
                                                                       int32_t* __restrict__ seg_start) {
  const int lane = threadIdx.x & 63;
  const bool aligned = (reinterpret_cast<uintptr_t>(seg) & 15) == 0;
  // the grid is at most ceil(n / kSegScanTile) workgroups, so every position below -- those past the end included --
  // is < n + stride <= 2^31 + 2^31: 64-bit for the comparisons with n, 32-bit unsigned for the counters
  const int64_t stride = (int64_t)gridDim.x * kSegScanTile;
  SegScanCarry c = {0, 0, 0, 0, 0, 0, 0, n};
  if (f > 0) {
    const uint32_t uf = (uint32_t)f;
    const uint32_t first = (uint32_t)blockIdx.x * (uint32_t)kSegScanTile + threadIdx.x * 4u;
    const uint32_t wrap = (uint32_t)stride - (uint32_t)((kSegScanLoads - 1) * kSegScanSpan);  // last quad of a tile -> first of the next
    c.quo = first / uf, c.rem = first % uf;
    c.span_q = (uint32_t)kSegScanSpan / uf, c.span_r = (uint32_t)kSegScanSpan % uf;
    c.wrap_q = wrap / uf, c.wrap_r = wrap % uf;
  }
  for (int64_t t0 = (int64_t)blockIdx.x * kSegScanTile; t0 < n; t0 += stride) {
    if (aligned && t0 + kSegScanTile <= n) seg_scan_tile<true>(seg, n, num_segments, f, t0, lane, c, seg_start);  // uniform over the workgroup
    else seg_scan_tile<false>(seg, n, num_segments, f, t0, lane, c, seg_start);
  }
  // One atomic per WAVE and word, and none once the word already says as much (round 6): a ragged request whose length
  // divides evenly raises level 1 from nearly every thread -- 4 M atomics on one address for the headline's 16.4 M ids,
  // which queue at the memory side: +0.78 ms on a 3.6 ms aggregate (profiles/r06/seg_ragged_probe.txt).  The words only
  // grow, so a (coherent) read that already shows this wave's value or more makes the atomic redundant.
  // (no thread has left: every lane of the wave is in the ballots, and lane 0 speaks for it)
  const unsigned long long tag = (unsigned long long)epoch << 32;
  int32_t bad_at = c.bad_at;
  const uint64_t at2 = __ballot(c.level == 2), at1 = __ballot(c.level >= 1);
  if (at2) {  // the first violation of the wave = the smallest bad_at (n: none, a long run of empty segments only)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int32_t other = __shfl_xor(bad_at, o);
      if (other < bad_at) bad_at = other;
    }
  }
  const int32_t wave_level = at2 ? 2 : (at1 ? 1 : 0);
  if (wave_level && lane == 0) {
    if (bad_at < n) {  // the largest n - i = the first violation
      const unsigned long long mine = tag | (uint32_t)(n - bad_at);
      if (__hip_atomic_load(&words[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < mine) atomicMax(&words[0], mine);
    }
    const unsigned long long mine = tag | (uint32_t)wave_level;
    if (__hip_atomic_load(&words[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < mine) atomicMax(&words[1], mine);
  }
}

// The scan as it was launched through round 24 (glx_tune("seg_scan_parent", 1): same-process A/B and the equality
// tests): one thread per quad, its own load of the id before the quad, 1 KiB per wave.
__global__ __launch_bounds__(256) void glx_seg_scan_parent_kernel(const int32_t* __restrict__ seg, int32_t n, int32_t num_segments,
                                                                  int32_t f, unsigned long long* __restrict__ words, uint32_t epoch,
                                                                  int32_t* __restrict__ seg_start) {
  const int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i0 >= n) return;
  int32_t v[4];
  const int32_t m = (n - i0) < 4 ? (int32_t)(n - i0) : 4;
  if (m == 4 && (reinterpret_cast<uintptr_t>(seg) & 15) == 0) {
    const int4 q = *reinterpret_cast<const int4*>(seg + i0);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    for (int j = 0; j < 4; ++j) v[j] = j < m ? seg[i0 + j] : 0;
  }
  int32_t prev = i0 > 0 ? seg[i0 - 1] : -1;
  // the id before this thread's is itself out of range: a violation at or before it (its own thread reports it), so
  // nothing from here on belongs to the request -- and `prev` is no segment to count on from
  if (i0 > 0 && (prev < 0 || prev >= num_segments)) return;
  int32_t quo = f > 0 ? (int32_t)(i0 / f) : 0, rem = f > 0 ? (int32_t)(i0 % f) : 0;  // i / f and i % f, carried along
  bool nonuniform = false, incomplete = false;
  int32_t bad_at = n;
  for (int j = 0; j < m; ++j) {
    const int32_t i = (int32_t)i0 + j, cur = v[j];
    if (cur < 0 || cur >= num_segments || cur < prev) {  // prev == -1 before the first id
      bad_at = i;
      break;
    }
    if (cur != prev) {
      if (cur - prev > kSegRunMax) incomplete = true;
      else for (int32_t s = prev + 1; s <= cur; ++s) seg_start[s] = i;
    }
    if (f > 0) {
      nonuniform |= cur != quo;
      if (++rem == f) { rem = 0; ++quo; }
    }
    prev = cur;
  }
  if (bad_at == n && i0 + m == n) {  // the last ids: the segments after the last one used start (and end) at n
    if (num_segments - prev > kSegRunMax) incomplete = true;
    else for (int32_t s = prev + 1; s <= num_segments; ++s) seg_start[s] = n;
  }
  const unsigned long long tag = (unsigned long long)epoch << 32;
  if (bad_at < n) atomicMax(&words[0], tag | (uint32_t)(n - bad_at));  // the largest n - i = the first violation
  const int32_t level = (incomplete || bad_at < n) ? 2 : (nonuniform ? 1 : 0);
  // One atomic per WAVE, and none once the word already says as much (round 6): a ragged request whose length divides
  // evenly raises level 1 from nearly every thread -- 4 M atomics on one address for the headline's 16.4 M ids, which
  // queue at the memory side: +0.78 ms on a 3.6 ms aggregate (profiles/r06/seg_ragged_probe.txt).  The word only grows,
  // so a (coherent) read that already shows this wave's level or more makes the atomic redundant.
  // (ballots see the lanes still here: threads past the end of the request, or behind an out-of-range id, have left)
  const uint64_t here = __ballot(true), at2 = __ballot(level == 2), at1 = __ballot(level >= 1);
  const int32_t wave_level = at2 ? 2 : (at1 ? 1 : 0);
  if (wave_level && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)here) - 1)) {
    const unsigned long long mine = tag | (uint32_t)wave_level;
    if (__hip_atomic_load(&words[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < mine) atomicMax(&words[1], mine);
  }
}

// seg_start[s] = lower_bound(seg[0..valid_len), s) for every s -- only when the scan left the table incomplete.
// The grid walks the segments grid-stride: the common case (nothing to fix) then costs a capped launch that reads the
// level and returns, not a workgroup per 256 segments.
constexpr int kSegFixupWgPerCu = 2;   // 256 threads each
constexpr int kSegFixupSearches = 4;  // x 4 searches in flight per thread = a CU's 2,048 thread slots, as a full grid filled them
__global__ void glx_seg_fixup_kernel(const int32_t* __restrict__ seg, SegState st, int32_t n, int32_t num_segments,
                                     int32_t* __restrict__ seg_start) {
  if (seg_level(st) != 2) return;
  const int32_t valid_len = seg_valid_len(st, n);
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  // kSegFixupSearches segments a thread per pass, their searches side by side: each is a chain of dependent loads, and
  // the capped grid has that many times fewer threads than a thread per segment had
  for (int64_t s0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s0 <= num_segments; s0 += step * kSegFixupSearches) {
    int32_t lo[kSegFixupSearches], hi[kSegFixupSearches];
#pragma unroll
    for (int k = 0; k < kSegFixupSearches; ++k) {
      lo[k] = 0;
      hi[k] = s0 + k * step <= num_segments ? valid_len : 0;
    }
    bool more = valid_len > 0;
    while (more) {  // seg[0] exists in here: valid_len > 0
      int32_t mid[kSegFixupSearches], at[kSegFixupSearches];
#pragma unroll
      for (int k = 0; k < kSegFixupSearches; ++k) {
        mid[k] = lo[k] + ((hi[k] - lo[k]) >> 1);
        at[k] = seg[lo[k] < hi[k] ? mid[k] : 0];
      }
      more = false;
#pragma unroll
      for (int k = 0; k < kSegFixupSearches; ++k) {
        if (lo[k] < hi[k]) {
          if (at[k] < s0 + k * step) lo[k] = mid[k] + 1; else hi[k] = mid[k];
        }
        more |= lo[k] < hi[k];
      }
    }
#pragma unroll
    for (int k = 0; k < kSegFixupSearches; ++k) {
      if (s0 + k * step <= num_segments) seg_start[s0 + k * step] = lo[k];
    }
  }
}

// raw id -> feature row (int32, -1 = unknown id) for the hashed id map.
__global__ void glx_rows_kernel(GlxIdMap map, const int64_t* __restrict__ ids, int64_t n,
                                int32_t* __restrict__ rows) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  rows[i] = (int32_t)glx_row_of(map, ids[i]);
}

// (agg_init, agg_combine, AggElem and the raw-vector loads live in glx_common.h, shared with glx_aggregate_grad.hip)

// float32 -> float16 for the upload, round to nearest even, bit-identical -- all 2^32 inputs -- to
// torch.Tensor.to(torch.float16) of a contiguous CPU tensor, i.e. torch's vectorised conversion (the bfloat16 sibling,
// glx_f32_to_bf16_bits, lives in glx_common.h: the training path's row gradients round with it too).  A NaN keeps the
// sign and the top ten payload bits and sets the quiet bit (sign | 0x7E00 | payload >> 13).  Integer arithmetic only,
// so no floating-point mode (denormal flushing) can change a result.
__host__ __device__ __forceinline__ uint16_t glx_f32_to_f16_bits(uint32_t u) {
  const uint32_t sign = (u >> 16) & 0x8000u;
  const uint32_t a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return (uint16_t)(sign | 0x7E00u | ((a >> 13) & 0x3FFu));  // NaN: quiet, top payload bits
  if (a >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);  // >= 65520 (half-way past 65504, ties to even = 2^16): inf
  if (a >= 0x38800000u) {  // a normal half (>= 2^-14): rebias the exponent by 127 - 15, round off 13 mantissa bits
    const uint32_t m = a - 0x38000000u;
    return (uint16_t)(sign | ((m + 0xFFFu + ((m >> 13) & 1u)) >> 13));
  }
  // a half subnormal: round(|x| / 2^-24); |x| = mant 2^(e - 150), so shift the 24-bit significand by 126 - e
  const uint32_t e = a >> 23;
  const uint32_t sh = 126u - e;  // >= 14
  if (sh >= 25u) return (uint16_t)sign;  // < 2^-25 (float32 subnormals and zeros included): +-0
  const uint32_t mant = (a & 0x7fffffu) | 0x800000u;
  const uint32_t q = mant >> sh, rem = mant & ((1u << sh) - 1u), half = 1u << (sh - 1u);
  return (uint16_t)(sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u)));  // q + 1 may be 0x400 = 2^-14
}
// float32 -> OCP float8, round to nearest even, bit-identical to torch.Tensor.to(torch.float8_e4m3fn /
// torch.float8_e5m2) of a contiguous CPU tensor; integer arithmetic only.  MBITS mantissa bits under a BIAS-biased
// exponent; `a` is |x|'s bits, below the type's overflow threshold.
template <int MBITS, int BIAS>
__host__ __device__ __forceinline__ uint32_t glx_f32_to_f8_finite(uint32_t a) {
  constexpr uint32_t kDrop = 23u - MBITS;                   // float32 mantissa bits rounded off
  constexpr uint32_t kMinNormal = (uint32_t)(127 - BIAS + 1) << 23;  // 2^(1 - BIAS)
  if (a >= kMinNormal) {  // rebias the exponent, round; a carry out of the mantissa rounds up to the next binade
    const uint32_t m = a - ((uint32_t)(127 - BIAS) << 23);
    return (m + ((1u << (kDrop - 1u)) - 1u) + ((m >> kDrop) & 1u)) >> kDrop;
  }
  // a subnormal: round(|x| / 2^(1 - BIAS - MBITS)); |x| = mant 2^(e - 150), so shift the 24-bit significand
  const uint32_t e = a >> 23;
  const uint32_t sh = (uint32_t)(150 + 1 - BIAS - MBITS) - e;  // > kDrop
  if (sh >= 25u) return 0u;  // under half the smallest subnormal (float32 subnormals and zeros included)
  const uint32_t mant = (a & 0x7fffffu) | 0x800000u;
  const uint32_t q = mant >> sh, rem = mant & ((1u << sh) - 1u), half = 1u << (sh - 1u);
  return q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u);  // q + 1 may be the smallest normal
}
// e4m3fn has no infinity: 464 (the tie between 448 and the absent 480) still rounds to even = 448 = 0x7E, everything
// above it reaches the code 0x7F = NaN by the rounding's own carry -- overflow is NaN, not saturation -- and so do
// +-inf and every NaN (sign kept).
__host__ __device__ __forceinline__ uint8_t glx_f32_to_f8e4m3_bits(uint32_t u) {
  const uint32_t sign = (u >> 24) & 0x80u;
  const uint32_t a = u & 0x7fffffffu;
  if (a >= 0x43F00000u) return (uint8_t)(sign | 0x7Fu);  // >= 480, inf, NaN
  return (uint8_t)(sign | glx_f32_to_f8_finite<3, 7>(a));
}
// e5m2: 57344 is the largest number (0x7B); 61440 (the tie) and above is inf (0x7C); a NaN is sign | 0x7F.
__host__ __device__ __forceinline__ uint8_t glx_f32_to_f8e5m2_bits(uint32_t u) {
  const uint32_t sign = (u >> 24) & 0x80u;
  const uint32_t a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return (uint8_t)(sign | 0x7Fu);
  if (a >= 0x47800000u) return (uint8_t)(sign | 0x7Cu);  // >= 65536 (61440 .. 65536 round up to it below)
  return (uint8_t)(sign | glx_f32_to_f8_finite<2, 15>(a));
}

struct AggArgs {
  const void* X;             // elements of `dtype` (X1 / X2 below: float32 only)
  const int64_t* node_ids;   // raw ids (dense map) ...
  const int32_t* rows;       // ... or pre-translated rows (hashed map / multi-source); one is null
  const int32_t* seg_start;  // [num_segments + 1], or null: uniform segments of `fanout` ids
  SegState seg_state;        // with seg_start: level 0 -> the segments ARE uniform (`fanout` ids each), seg_start is not read
  float* emb_out;
  int32_t* cnt_out;
  int64_t num_rows;
  int64_t stride;
  int64_t swizzle_rows;
  int32_t dim;
  int32_t num_segments;
  int32_t fanout;
  float default_attr;
  int32_t col0, ncols;       // the columns [col0, col0 + ncols) this launch reduces (a column slice, or all)
  int32_t store_mode;        // glx_aggregate_grp_kernel: 0 non-temporal output stores (default), 1 plain stores (ablation)
  int32_t load_repeats;      // glx_aggregate_grp_kernel, Max / Min over a whole wave: 0 a row the segment already folded is not
                             // loaded again, 1 every position is loaded (launch_agg_grp chooses)
  int32_t segs_per_group;    // glx_aggregate_grp_kernel: consecutive segments one lane group reduces
  int32_t xcd_slices;        // glx_aggregate_grp_kernel: > 1 = workgroup b reduces column slice b % xcd_slices (ncols each)
  int32_t stripe_chunk;      // glx_aggregate_grp_kernel: > 0 = XCD stripes of this many segment blocks (agg_stripe_block)
  uint32_t stripe_full;      // ... the slice-local block indices [0, stripe_full) that the stripes permute
  // further row sources of the distributed store (glx_dist.hip): virtual row r lives in
  // source 0 when r < base1, in source 1 (the hot-row replica) when r < base2, else in
  // source 2 (the halo rows of this request, plain row-major, no swizzle).
  const float* X1;
  const float* X2;
  int64_t stride1, swizzle1, stride2;
  int32_t base1, base2;
  int32_t dtype;  // X's storage type (host side: picks the instantiation; last, so no field above moves)
};

// Feature rows are < 2^31 (checked at creation), so a row index fits an int32 --
// half the registers of the raw int64 id.
__device__ __forceinline__ int32_t agg_row_at(const AggArgs& a, int32_t pos) {
  if (a.rows) return a.rows[pos];
  const int64_t id = a.node_ids[pos];
  return (id >= 0 && id < a.num_rows) ? (int32_t)id : -1;
}

template <int NSRC, int DT = GLX_DTYPE_F32>
__device__ __forceinline__ const typename AggElem<DT>::raw* agg_row_ptr(const AggArgs& a, int32_t row) {
  const typename AggElem<DT>::raw* X = static_cast<const typename AggElem<DT>::raw*>(a.X);
  if constexpr (NSRC == 1) {
    return X + glx_swizzle_row(row, a.swizzle_rows) * a.stride;
  } else {
    static_assert(DT == GLX_DTYPE_F32, "the distributed store's row sources are float32");
    if (row < a.base1) return X + glx_swizzle_row(row, a.swizzle_rows) * a.stride;
    if (row < a.base2) return a.X1 + glx_swizzle_row(row - a.base1, a.swizzle1) * a.stride1;
    return a.X2 + (int64_t)(row - a.base2) * a.stride2;
  }
}

// G lanes per segment, VEC elements per lane per pass (VEC = 4: one 16-byte load of
// floats, 8 bytes of halves, per row per lane; VEC = 1 for dims that are not a multiple of 4).
// U rows are issued back-to-back before the first is consumed.  NSRC = 3: rows come from the
// three sources of a distributed store.  DT: the table's storage type.
template <int OP, int G, int VEC, int U, int NSRC, int DT>
__global__ __launch_bounds__(256) void glx_aggregate_kernel(AggArgs a) {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  const int64_t gid = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / G;
  const int c = threadIdx.x & (G - 1);
  if (gid >= a.num_segments) return;
  int32_t s0, s1;
  if (a.seg_start && seg_level(a.seg_state) != 0) {
    s0 = a.seg_start[gid];
    s1 = a.seg_start[gid + 1];
  } else {  // a dense sampler response: segment gid = ids [gid * fanout, (gid + 1) * fanout)
    s0 = (int32_t)gid * a.fanout;
    s1 = s0 + a.fanout;
  }
  const int32_t n = s1 - s0;
  if (c == 0 && a.col0 == 0) a.cnt_out[gid] = n;
  float* out = a.emb_out + gid * (int64_t)a.dim;
  const int32_t col_end = a.col0 + a.ncols;
  for (int32_t col = a.col0 + c * VEC; col < col_end; col += G * VEC) {
    vec_t acc;
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = agg_init<OP>();
    for (int32_t base = s0; base < s1; base += U) {
      int32_t row[U];
#pragma unroll
      for (int u = 0; u < U; ++u) row[u] = (base + u < s1) ? agg_row_at(a, base + u) : -2;
      vec_t val[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (row[u] >= 0) {
          val[u] = agg_load<DT, VEC>(agg_row_ptr<NSRC, DT>(a, row[u]) + col);
        } else {
#pragma unroll
          for (int v = 0; v < VEC; ++v) val[u][v] = a.default_attr;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (row[u] != -2) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[v] = agg_combine<OP>(acc[v], val[u][v]);
        }
      }
    }
    // FinalFunc: aggregator.cc:74-86 (empty -> default), mean_aggregator.cc:45-61.
    if (n == 0) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] = a.default_attr;
    } else if (OP == GLX_AGG_MEAN) {
      const float fn = (float)n;
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] = acc[v] / fn;
    }
    *reinterpret_cast<vec_t*>(out + col) = acc;
  }
}

// ---- the wide shapes (16-byte loads, 8..64 lanes per segment): ids fetched ONCE, coalesced ------------------
// glx_aggregate_kernel above asks for every id with a load of its own in which all lanes of a group read the same
// address, each followed by a wait: a fanout-10 segment is ten dependent round trips before the first row load
// issues.  Here a group of G lanes keeps a CHUNK of G * IDR consecutive positions of its id
// range in registers -- lane c holds positions chunk_base + k G + c, one coalesced load per register -- already
// translated to feature rows, and hands row `pos` to all its lanes with a cross-lane read: v_readlane for a whole
// wave (the row index, the swizzle, the multiply by the pitch and the bounds test then run on the scalar unit and
// the row load takes its base address from SGPRs), ds_bpermute for the narrower groups.  A group reduces S
// consecutive segments one after the other so a chunk serves several of them (S f <= chunk for the dense sampler
// responses); up to U row loads are issued back to back before the first is consumed.  Accumulation order is
// unchanged: lane c owns columns [4c, 4c + 4) of its group's segment and folds the rows left to right
// (aggregator.cc:45-56), so results stay bit-identical to the reference's serial loop.
template <int G, int IDR>
__device__ __forceinline__ void agg_chunk_load(const AggArgs& a, int32_t chunk_base, int32_t pos_end, int c,
                                               int32_t (&myrow)[IDR]) {
#pragma unroll
  for (int k = 0; k < IDR; ++k) {
    const int32_t pos = chunk_base + k * G + c;
    myrow[k] = pos < pos_end ? agg_row_at(a, pos) : -1;
  }
}

// row held for chunk slot idx in [0, G * IDR) (group-uniform idx)
template <int G, int IDR>
__device__ __forceinline__ int32_t agg_chunk_get(const int32_t (&myrow)[IDR], int32_t idx) {
  if (G == 64) {
    int32_t r = __builtin_amdgcn_readlane(myrow[0], idx & 63);
#pragma unroll
    for (int k = 1; k < IDR; ++k) {
      const int32_t t = __builtin_amdgcn_readlane(myrow[k], idx & 63);
      r = (idx >> 6) == k ? t : r;
    }
    return r;
  }
  int32_t r = __shfl(myrow[0], idx & (G - 1), G);
#pragma unroll
  for (int k = 1; k < IDR; ++k) {
    const int32_t t = __shfl(myrow[k], idx & (G - 1), G);
    r = (idx / G) == k ? t : r;
  }
  return r;
}

// Row pointer with 32-bit row arithmetic (rows < 2^31, pitch < 2^31 floats): for a wave-uniform row this is a
// handful of SALU instructions.
__device__ __forceinline__ uint32_t agg_swizzle32(uint32_t r, uint32_t swizzle_rows) {
  const uint32_t m = ((r >> GLX_SWIZZLE_BITS) * 0x9E3779B1u) >> (32 - GLX_SWIZZLE_BITS);
  return r < swizzle_rows ? r ^ m : r;
}

// The pitch is in elements (< 2^31 of them), so the product scales by the element size in the pointer arithmetic.
template <int NSRC, int DT>
__device__ __forceinline__ const typename AggElem<DT>::raw* agg_row_ptr32(const AggArgs& a, int32_t row) {
  const typename AggElem<DT>::raw* X = static_cast<const typename AggElem<DT>::raw*>(a.X);
  if constexpr (NSRC == 1) {
    return X + (uint64_t)agg_swizzle32((uint32_t)row, (uint32_t)a.swizzle_rows) * (uint32_t)a.stride;
  } else {
    static_assert(DT == GLX_DTYPE_F32, "the distributed store's row sources are float32");
    if (row < a.base1) {
      return X + (uint64_t)agg_swizzle32((uint32_t)row, (uint32_t)a.swizzle_rows) * (uint32_t)a.stride;
    }
    if (row < a.base2) {
      return a.X1 + (uint64_t)agg_swizzle32((uint32_t)(row - a.base1), (uint32_t)a.swizzle1) * (uint32_t)a.stride1;
    }
    return a.X2 + (uint64_t)(uint32_t)(row - a.base2) * (uint32_t)a.stride2;
  }
}

// One batch: rows of chunk slots [slot0, slot0 + count), count <= U (kFull: count == U, no tests at all), all
// loads issued before the first is folded into acc, in slot order.
template <int OP, int G, int VEC, int U, int NSRC, int IDR, bool kFull, int DT>
__device__ __forceinline__ void agg_grp_batch(const AggArgs& a, const int32_t (&myrow)[IDR], int32_t slot0, int32_t count,
                                              uint32_t col_ld, float __attribute__((ext_vector_type(VEC)))& acc) {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  int32_t row[U];
#pragma unroll
  for (int u = 0; u < U; ++u) row[u] = agg_chunk_get<G, IDR>(myrow, slot0 + u);
  agg_raw_vec<DT, VEC> val[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (kFull || u < count) {
      // an unknown id (row -1) reads row 0 and is replaced below: no divergent branch around the load
      const int32_t r = row[u] >= 0 ? row[u] : 0;
      val[u] = agg_load_raw<DT, VEC>(agg_row_ptr32<NSRC, DT>(a, r) + col_ld);
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (kFull || u < count) {
      vec_t x = agg_up<DT, VEC>(val[u]);
#pragma unroll
      for (int v = 0; v < VEC; ++v) x[v] = row[u] < 0 ? a.default_attr : x[v];
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] = agg_combine<OP>(acc[v], x[v]);
    }
  }
}

// ---- Max / Min over a whole wave: a row the segment has already folded is not loaded again -------------------
// The fold is a select -- Max (l < r) ? r : l from -37, Min (r < l) ? r : l from FLT_MAX -- so the accumulator is never
// NaN (a NaN operand is never selected, the start is none), once x has been folded it is >= x (Max; <= x for Min) in
// the order of the non-NaN floats, and every later fold only moves it further: folding the same row AGAIN selects
// nothing, whatever came in between (+-0, +-inf, NaN elements, values at or below -37, and the unknown ids, which all
// fold default_attr).  Dropping the later occurrences and folding the rest in the same order is therefore exact, bit
// for bit.  It pays where draws with replacement repeat the few neighbours of a low-degree seed: C3's hop 1 (fanout
// 25) holds 5.7 distinct rows per segment, and every repeat was a 1 KiB wave load through the vector-memory pipeline
// that launch is bound by.  Sum, Mean and Prod have no such property and never come here.
//
// Lane c holds the row of chunk slot c.  keep = the first slot of every distinct row among the slots [lo, hi): one
// iteration per DISTINCT row -- the lowest pending slot survives and takes every slot that holds its row out of the
// pending set.  The masks live in SGPRs and the branch is scalar.
// (Not the 16-byte loads of a half table, GLX_AGG_HALF_LD16: an ablation already, and the masks cost it a wave of occupancy.)
template <int OP, int G, int VEC>
constexpr bool kAggSkipRepeats = G == 64 && VEC == 4 && (OP == GLX_AGG_MAX || OP == GLX_AGG_MIN);

__device__ __forceinline__ uint64_t agg_first_occurrences(int32_t myrow, int32_t lo, int32_t hi) {
  uint64_t pending = (hi >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << hi) - 1)) & ~(((uint64_t)1 << lo) - 1);
  uint64_t keep = 0;
  while (pending != 0) {
    const int u = __builtin_ctzll(pending);
    const int32_t r = __builtin_amdgcn_readlane(myrow, u);
    const uint64_t bit = (uint64_t)1 << u;
    keep |= bit;
    pending &= ~(__ballot(myrow == r) | bit);
  }
  return keep;
}

// agg_grp_batch over the next `count` set bits of keep (kFull: count == U), lowest first, instead of consecutive
// slots: the same loads back to back, the same fold.  The bits taken are cleared.
template <int OP, int VEC, int U, int NSRC, bool kFull, int DT>
__device__ __forceinline__ void agg_keep_batch(const AggArgs& a, int32_t myrow, uint64_t& keep, int32_t count, uint32_t col_ld,
                                               float __attribute__((ext_vector_type(VEC)))& acc) {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  int32_t row[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    row[u] = -1;
    if (kFull || u < count) {
      row[u] = __builtin_amdgcn_readlane(myrow, __builtin_ctzll(keep));
      keep &= keep - 1;
    }
  }
  agg_raw_vec<DT, VEC> val[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (kFull || u < count) {
      const int32_t r = row[u] >= 0 ? row[u] : 0;  // as in agg_grp_batch
      val[u] = agg_load_raw<DT, VEC>(agg_row_ptr32<NSRC, DT>(a, r) + col_ld);
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (kFull || u < count) {
      vec_t x = agg_up<DT, VEC>(val[u]);
#pragma unroll
      for (int v = 0; v < VEC; ++v) x[v] = row[u] < 0 ? a.default_attr : x[v];
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] = agg_combine<OP>(acc[v], x[v]);
    }
  }
}

// XCD stripes: the slice-local workgroup index j (j = b / n for workgroup b and n column slices) -> the segment block
// it reduces.  Workgroup b runs on XCD b % 8 (observed placement, used for speed only), so the P = 8 / n XCDs that
// share a slice see j = P k + m (m = the XCD's label, k = its k-th workgroup of the launch).  The permutation hands
// label m the m-th chunk of `chunk` consecutive blocks out of every run of P * chunk, so each XCD walks contiguous
// stripes of segments -- a seed's hop-1 samples, and the rows their twins share, stay in one L2 -- instead of every
// P-th block.  It is a bijection of [0, full) (full = whole runs only) and the identity beyond: every (segment block,
// slice) pair is reduced exactly once whatever the placement.
__device__ __forceinline__ uint32_t agg_stripe_block(uint32_t j, uint32_t P, uint32_t chunk, uint32_t full) {
  if (j >= full) return j;
  const uint32_t span = P * chunk;
  const uint32_t run = j / span;
  const uint32_t r = j - run * span;
  const uint32_t k = r / P;
  return run * span + (r - k * P) * chunk + k;
}

__device__ __forceinline__ void agg_store4(int32_t store_mode, float* dst, float __attribute__((ext_vector_type(4))) v) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  if (store_mode == 1) *reinterpret_cast<f4*>(dst) = v;
  else __builtin_nontemporal_store(v, reinterpret_cast<f4*>(dst));
}

template <int OP, int G, int VEC, int U, int NSRC, int IDR, int DT>
__global__ __launch_bounds__(256) void glx_aggregate_grp_kernel(AggArgs a) {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  constexpr int kChunk = G * IDR;
  static_assert(U <= kChunk, "a batch must fit the chunk");
  constexpr int kGroupsPerBlock = 256 / G;
  // XCD-affine column slices (a.xcd_slices > 1): workgroup b runs on XCD b % 8 (observed placement, used for speed
  // only), so slice = b % xcd_slices keeps one column slice of EVERY row in one XCD's L2
  const uint32_t nsl = a.xcd_slices > 1 ? (uint32_t)a.xcd_slices : 1u;
  const int32_t slice = (int32_t)(blockIdx.x % nsl);
  uint32_t j = blockIdx.x / nsl;
  if (a.stripe_chunk > 0) j = agg_stripe_block(j, 8u / nsl, (uint32_t)a.stripe_chunk, a.stripe_full);
  const int64_t blk = j;
  int64_t grp = blk * kGroupsPerBlock + threadIdx.x / G;
  const int c = threadIdx.x & (G - 1);
  const int32_t S = a.segs_per_group;
  int64_t seg64 = grp * S;
  if (seg64 >= a.num_segments) return;
  int32_t seg_first = (int32_t)seg64;
  if (G == 64) seg_first = __builtin_amdgcn_readfirstlane(seg_first);
  const int32_t seg_last = (a.num_segments - seg_first) < S ? a.num_segments : seg_first + S;
  // segment boundaries: arithmetic for a dense sampler response, else lane j of the group holds start[seg_first + j]
  // (an explicit segment_ids tensor that spells out the dense response -- flags[1] == 0 -- takes the arithmetic too)
  const bool use_starts = a.seg_start != nullptr && seg_level(a.seg_state) != 0;
  int32_t mystart = 0;
  if (use_starts) mystart = a.seg_start[seg_first + (c <= seg_last - seg_first ? c : 0)];
  const int32_t starts[1] = {mystart};
  const int32_t pos_first = use_starts ? agg_chunk_get<G, 1>(starts, 0) : seg_first * a.fanout;
  const int32_t pos_end = use_starts ? agg_chunk_get<G, 1>(starts, seg_last - seg_first) : seg_last * a.fanout;
  const int32_t col_lo = a.col0 + slice * a.ncols;
  const int32_t col_end = col_lo + a.ncols;
  for (int32_t col_pass = col_lo; col_pass < col_end; col_pass += G * VEC) {
    const int32_t col = col_pass + c * VEC;
    const bool col_ok = col < col_end;
    const uint32_t col_ld = col_ok ? (uint32_t)col : (uint32_t)col_lo;  // lanes past the end re-read lane 0's columns, unused
    int32_t chunk_base = pos_first;
    int32_t myrow[IDR];
    agg_chunk_load<G, IDR>(a, chunk_base, pos_end, c, myrow);
    for (int32_t sg = seg_first; sg < seg_last; ++sg) {
      int32_t s0, s1;
      if (use_starts) {
        s0 = agg_chunk_get<G, 1>(starts, sg - seg_first);
        s1 = agg_chunk_get<G, 1>(starts, sg - seg_first + 1);
      } else {
        s0 = sg * a.fanout;
        s1 = s0 + a.fanout;
      }
      vec_t acc;
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] = agg_init<OP>();
      bool folded = false;
      if constexpr (kAggSkipRepeats<OP, G, VEC>) {
        static_assert(IDR == 1, "a whole wave keeps one id register");
        if (a.load_repeats == 0) {
          // piece by piece of up to kChunk positions, each resident in the chunk as a whole: the first occurrences of
          // the piece, folded in order.  (A repeat across two pieces is loaded again: skipping any subset is exact.)
          for (int32_t pos = s0; pos < s1;) {
            const int32_t piece_end = (s1 - pos) < kChunk ? s1 : pos + kChunk;
            if (piece_end - chunk_base > kChunk) {
              chunk_base = pos;
              agg_chunk_load<G, IDR>(a, chunk_base, pos_end, c, myrow);
            }
            uint64_t keep = agg_first_occurrences(myrow[0], pos - chunk_base, piece_end - chunk_base);
            int32_t m = __builtin_popcountll(keep);
            for (; m >= U; m -= U) agg_keep_batch<OP, VEC, U, NSRC, true, DT>(a, myrow[0], keep, U, col_ld, acc);
            if (m > 0) agg_keep_batch<OP, VEC, U, NSRC, false, DT>(a, myrow[0], keep, m, col_ld, acc);
            pos = piece_end;
          }
          folded = true;
        }
      }
      for (int32_t base = s0; !folded && base < s1; base += U) {
        const int32_t stop = (s1 - base) < U ? s1 : base + U;
        if (stop > chunk_base + kChunk) {  // the batch runs past the chunk: next chunk starts at this batch
          chunk_base = base;
          agg_chunk_load<G, IDR>(a, chunk_base, pos_end, c, myrow);
        }
        if (stop - base == U) agg_grp_batch<OP, G, VEC, U, NSRC, IDR, true, DT>(a, myrow, base - chunk_base, U, col_ld, acc);
        else agg_grp_batch<OP, G, VEC, U, NSRC, IDR, false, DT>(a, myrow, base - chunk_base, stop - base, col_ld, acc);
      }
      // FinalFunc: aggregator.cc:74-86 (empty -> default), mean_aggregator.cc:45-61.
      const int32_t n = s1 - s0;
      if (n == 0) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = a.default_attr;
      } else if (OP == GLX_AGG_MEAN) {
        const float fn = (float)n;
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = acc[v] / fn;
      }
      if (col_ok) {
        float* const dst = a.emb_out + sg * (int64_t)a.dim + col;
        // the outputs are written once and never read by this launch: the non-temporal hint (round 4, A/B in
        // profiles/r04/agg_probe_run8_nt_stores.txt: uniform rows -2.4 .. -5 %, the power-law requests -1 %, L2-resident -12 .. -20 %;
        // `sc1` write-through stores: no gain).  GLX_AGG_STORE=1 restores plain stores.  A half table's lane owns 8
        // columns: two 16-byte stores (emb_out is only known to be 16-byte aligned).
        if constexpr (VEC == 8) {
          agg_store4(a.store_mode, dst, acc.lo);
          agg_store4(a.store_mode, dst + 4, acc.hi);
        } else {
          if (a.store_mode == 1) *reinterpret_cast<vec_t*>(dst) = acc;
          else __builtin_nontemporal_store(acc, reinterpret_cast<vec_t*>(dst));
        }
      }
      if (c == 0 && col_pass == 0) a.cnt_out[sg] = n;
    }
  }
}

// ---- north_star's "dense feature tile staged in LDS, MFMA on the tile" formulation of Sum / Mean, kept as a
// measured ABLATION (GLX_AGG_MFMA=1; profiles/r03/mfma_ablation.txt) ----------------------------
// A segmented sum is the SpMM  Out[Sg, D] = S[Sg, N] * Xg[N, D]  with S the 0/1 segment-indicator matrix.  For a
// dense sampler response (uniform fanout f) a workgroup owns 16 consecutive segments = 16 f consecutive ids:
//   * the 4 waves gather KC rows at a time into LDS with 16-byte loads (row pitch D + 16 floats: the four rows
//     of one MFMA step then sit in four disjoint groups of 16 banks);
//   * wave w owns the columns [w D/4, (w+1) D/4) as NB = D/64 blocks of 16 and issues, per 4 rows,
//     v_mfma_f32_16x16x4_f32 with A[m][k] = (row k belongs to segment m) and B[k][n] = the staged row;
//   * f32 MFMA is an exact fmaf chain over k in order and the indicator is 0 or 1, so every output element
//     is still accumulated in the reference's left-to-right order (sum_aggregator.cc:25-33) -- as long as every
//     staged element is finite: the other 15 segments' rows enter each column as 0 x row, and 0 x inf and 0 x NaN
//     are NaN, so one non-finite element would turn its column into NaN for all 16 segments of the workgroup (the
//     reference leaves them finite).  Staging therefore flags any element whose exponent field is all ones (an
//     integer test on the bits), and a workgroup that staged one recomputes its <= 16 segments with the serial VALU
//     fold straight from global memory (agg_mfma_serial) before the stores: bit-identical on any input.
// 15/16 of the multiply-adds multiply by zero, f32 MFMA runs at the vector rate (157 TF), and the reduce is
// 0.25 flop/byte: the matrix core cannot make it faster than the HBM stream -- the ablation measures what the
// LDS round trip and the workgroup barriers cost instead.
__device__ __forceinline__ bool agg_nonfinite4(float __attribute__((ext_vector_type(4))) v) {
  // exponent field all ones (inf / NaN): (bits & 0x7f800000) == 0x7f800000 for any of the four
  const uint32_t e = 0x7f800000u;
  return ((__float_as_uint(v[0]) & e) == e) || ((__float_as_uint(v[1]) & e) == e) || ((__float_as_uint(v[2]) & e) == e) ||
         ((__float_as_uint(v[3]) & e) == e);
}

// The reference's serial fold of one output element of a dense sampler response (segment sg, column col): what the
// grouped VALU kernel computes, for the workgroups of the MFMA ablation that staged a non-finite element.  The fields
// of AggArgs it reads come by value (a reference to the kernel argument would have it copied to scratch).
__device__ __noinline__ float agg_mfma_serial(const float* X, const int64_t* node_ids, const int32_t* rows,
                                              int64_t num_rows, int64_t stride, int64_t swizzle_rows,
                                              float default_attr, int64_t sg, int32_t col, int32_t f) {
  float acc = 0.0f;  // InitFunc (aggregator.cc:61-65)
  for (int32_t r = 0; r < f; ++r) {
    const int64_t pos = sg * f + r;
    int64_t row;
    if (rows) {
      row = rows[pos];
    } else {
      const int64_t id = node_ids[pos];
      row = (id >= 0 && id < num_rows) ? id : -1;
    }
    const float x = row >= 0 ? X[glx_swizzle_row(row, swizzle_rows) * stride + col] : default_attr;
    acc = acc + x;
  }
  return acc;
}

template <int OP, int NB>
__global__ __launch_bounds__(256) void glx_aggregate_mfma_kernel(AggArgs a) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  constexpr int KC = 32;  // rows staged per round
  extern __shared__ float tile[];  // [KC][pitch]
  constexpr int32_t D = 64 * NB;
  constexpr int32_t pitch = D + 16;
  const int32_t f = a.fanout;
  const int64_t seg0 = (int64_t)blockIdx.x * 16;
  const int32_t nseg = (int32_t)((a.num_segments - seg0) < 16 ? (a.num_segments - seg0) : 16);
  const int64_t id0 = seg0 * f;
  const int32_t nrows = nseg * f;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int m = lane & 15;   // A: segment row of this lane / B, C: column inside the block
  const int kq = lane >> 4;  // A, B: which of the step's 4 rows / C: row group
  f4 acc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = f4{0.f, 0.f, 0.f, 0.f};
  constexpr int32_t row_f4 = D / 4;
  constexpr int32_t PT = KC * row_f4 / 256;  // 16-byte pieces per thread per round (2 NB)
  bool nonfinite = false;  // this thread staged an inf / NaN (the default row's included)
  for (int32_t base = 0; base < nrows; base += KC) {
    // stage rows [base, base + KC): thread t moves pieces t, t + 256, ...; all loads issued before the first store
    f4 v[PT];
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      const int32_t p = threadIdx.x + i * 256;
      const int32_t r = p / row_f4;
      const int32_t c4 = p - r * row_f4;
      v[i] = f4{0.f, 0.f, 0.f, 0.f};
      if (base + r < nrows) {
        const int32_t row = agg_row_at(a, (int32_t)(id0 + base + r));
        if (row >= 0) v[i] = *reinterpret_cast<const f4*>(agg_row_ptr<1>(a, row) + c4 * 4);
        else v[i] = f4{a.default_attr, a.default_attr, a.default_attr, a.default_attr};
      }
    }
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      const int32_t p = threadIdx.x + i * 256;
      const int32_t r = p / row_f4;
      const int32_t c4 = p - r * row_f4;
      *reinterpret_cast<f4*>(tile + r * pitch + c4 * 4) = v[i];
      nonfinite |= agg_nonfinite4(v[i]);
    }
    __syncthreads();
#pragma unroll 2
    for (int32_t k4 = 0; k4 < KC; k4 += 4) {
      const int32_t krow = base + k4 + kq;
      const float ind = (krow < nrows && krow / f == m) ? 1.0f : 0.0f;
      const float* brow = tile + (k4 + kq) * pitch + wave * (D / 4) + m;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(ind, brow[b * 16], acc[b], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // one flag per workgroup: every thread of it then either keeps the MFMA sums or refolds its own outputs serially
  const bool refold = __syncthreads_or(nonfinite) != 0;
  // C/D: col = lane & 15, row = (lane >> 4) * 4 + reg
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int32_t srow = kq * 4 + reg;
    if (srow < nseg) {
      float* out = a.emb_out + (seg0 + srow) * (int64_t)D + wave * (D / 4) + m;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        float v = acc[b][reg];
        if (refold) {
          v = agg_mfma_serial(static_cast<const float*>(a.X), a.node_ids, a.rows, a.num_rows, a.stride, a.swizzle_rows,
                              a.default_attr, seg0 + srow, wave * (D / 4) + m + b * 16, f);
        }
        if (f == 0) v = a.default_attr;
        else if (OP == GLX_AGG_MEAN) v = v / (float)f;
        out[b * 16] = v;
      }
    }
  }
  if (threadIdx.x < nseg) a.cnt_out[seg0 + threadIdx.x] = f;
}

// ---- experiment knobs ------------------------------------------------------------------------------------
// Read from the environment ONCE (first launch in the process; Process() runs on up to 32 pool threads and
// getenv is not something to call per launch), and settable at run time through glx_tune() so a probe can A/B
// kernels inside one process.  Every knob is an ablation / measurement aid: 0 = the product's default.
struct AggKnobs {
  std::atomic<int> mfma{0};     // GLX_AGG_MFMA=1: the LDS-staged MFMA formulation of Sum / Mean (ablation)
  std::atomic<int> unroll{0};   // GLX_AGG_UNROLL: rows in flight per lane (0 = chosen from the fanout)
  std::atomic<int> slices{0};   // GLX_AGG_SLICES=2|4|8: column slices as consecutive launches (ablation)
  std::atomic<int> legacy{0};   // GLX_AGG_LEGACY=1: the round-1..3 kernel (one id load per row per lane)
  std::atomic<int> segs{0};     // GLX_AGG_SEGS: segments per lane group (0 = chosen from fanout and grid size)
  std::atomic<int> xcd{0};      // GLX_AGG_XCD_SLICES=1|2|4|8: column slice = workgroup % n (XCD-affine); 0 = 2 for big requests
  std::atomic<int> occ{0};      // GLX_AGG_OCCUPANCY=3..7: workgroups per CU, capped with an unused LDS allocation
  std::atomic<int> store{0};    // GLX_AGG_STORE=1: plain output stores instead of non-temporal ones (ablation)
  std::atomic<int> stripes{-1}; // GLX_AGG_XCD_STRIPES=0: workgroup j of a slice reduces segment block j (no XCD stripes); 1 = on; -1 = default
  std::atomic<int> chunk{0};    // GLX_AGG_XCD_CHUNK: segment blocks per XCD stripe chunk (0 = kXcdStripeChunk)
  std::atomic<int> half_ld16{0};// GLX_AGG_HALF_LD16=1: half and float8 tables in the grouped kernel with 8 columns per lane
                                // (16-byte loads of halves, 8-byte loads of float8); 2: 4 columns per lane, the float32
                                // lane-to-column map, for every type; 0 = default (launch_agg_cols: 4, float8 rows of >= 256: 8)
  std::atomic<int> repeats{0};  // GLX_AGG_REPEATS=1: Max / Min load every position of a segment, repeated rows included (ablation);
                                // 2: first occurrences only whatever the segment length; 0 = by length (launch_agg_grp)
  std::atomic<int> seg_parent{0};  // GLX_SEG_SCAN_PARENT=1: explicit segment_ids with the scan and fix-up launches of rounds 5..24 (A/B)
  std::atomic<int> seg_wgs{0};     // GLX_SEG_SCAN_WGS: at most this many workgroups in the scan's grid (0 = kSegScanWgPerCu per CU)
};

AggKnobs& agg_knobs() {
  static AggKnobs k;
  static std::once_flag once;
  std::call_once(once, [] {
    auto env = [](const char* name) {
      const char* e = getenv(name);
      return e ? atoi(e) : 0;
    };
    k.mfma = env("GLX_AGG_MFMA");
    k.unroll = env("GLX_AGG_UNROLL");
    k.slices = env("GLX_AGG_SLICES");
    k.legacy = env("GLX_AGG_LEGACY");
    k.segs = env("GLX_AGG_SEGS");
    k.xcd = env("GLX_AGG_XCD_SLICES");
    k.occ = env("GLX_AGG_OCCUPANCY");
    k.store = env("GLX_AGG_STORE");
    if (getenv("GLX_AGG_XCD_STRIPES")) k.stripes = env("GLX_AGG_XCD_STRIPES");
    k.chunk = env("GLX_AGG_XCD_CHUNK");
    k.half_ld16 = env("GLX_AGG_HALF_LD16");
    k.seg_parent = env("GLX_SEG_SCAN_PARENT");
    k.seg_wgs = env("GLX_SEG_SCAN_WGS");
    k.repeats = env("GLX_AGG_REPEATS");
  });
  return k;
}

bool agg_use_mfma(const AggArgs& a, int op) {
  if (agg_knobs().mfma.load(std::memory_order_relaxed) == 0) return false;
  // float32 tables only: a half table takes the VALU kernel with the knob set
  return a.dtype == GLX_DTYPE_F32 && (op == GLX_AGG_SUM || op == GLX_AGG_MEAN) && a.seg_start == nullptr && a.fanout > 0 && a.X1 == nullptr &&
         a.X2 == nullptr && (a.dim == 64 || a.dim == 128 || a.dim == 256) && (a.stride % 4) == 0 &&
         (reinterpret_cast<uintptr_t>(a.X) & 15) == 0;
}

template <int OP>
void launch_agg_mfma(const AggArgs& a, hipStream_t s) {
  const unsigned grid = (unsigned)((a.num_segments + 15) / 16);
  const size_t lds = (size_t)32 * (a.dim + 16) * sizeof(float);
  if (a.dim == 64) glx_aggregate_mfma_kernel<OP, 1><<<grid, 256, lds, s>>>(a);
  else if (a.dim == 128) glx_aggregate_mfma_kernel<OP, 2><<<grid, 256, lds, s>>>(a);
  else glx_aggregate_mfma_kernel<OP, 4><<<grid, 256, lds, s>>>(a);
}

// ---- legacy kernel launch (narrow / unaligned shapes, and GLX_AGG_LEGACY=1) --------------------------------
// Rows in flight per lane of glx_aggregate_kernel: A/B on the C3 hop-2 request (profiles/r02/agg_unroll_probe.txt)
// 3 / 4 / 5 / 6 / 8 / 10 / 12 rows -> 2.26 / 2.19 / 2.11 / 2.10 / 2.21 / 2.49 / 2.48 ms; wide float4 shapes 6, narrow 8.
template <int OP, int G, int VEC, int NSRC, int DT>
void launch_agg_g(const AggArgs& a, hipStream_t s) {
  const int64_t threads = (int64_t)a.num_segments * G;
  const unsigned grid = (unsigned)((threads + 255) / 256);
  constexpr bool kWide = VEC == 4 && G >= 32;
  glx_aggregate_kernel<OP, G, VEC, kWide ? 6 : 8, NSRC, DT><<<grid, 256, 0, s>>>(a);
}

// ---- grouped kernel launch ---------------------------------------------------------------------------------
// Rows in flight per lane (U): the fewest batches per segment wins, then the smaller batch (registers):
// fanout 10 -> 10, 15 -> 15, 25 -> 15 (15 + 10), 20 -> 10, 5 -> 5 of 6.  GLX_AGG_UNROLL overrides.
int agg_grp_unroll(int32_t fanout, int32_t avg_len) {
  static const int kU[] = {6, 8, 10, 12, 15};
  const int want = agg_knobs().unroll.load(std::memory_order_relaxed);
  for (int u : kU) {
    if (u == want) return u;
  }
  const int32_t f = fanout > 0 ? fanout : (avg_len > 0 ? avg_len : 10);
  int best = 10, best_batches = INT32_MAX;
  for (int u : kU) {
    const int batches = (f + u - 1) / u;
    if (batches < best_batches) {
      best = u;
      best_batches = batches;
    }
  }
  return best;
}

constexpr int32_t kAggSkipMinLen = 16;

template <int OP, int G, int VEC, int NSRC, int IDR, int DT>
void launch_agg_grp(AggArgs a, int32_t num_ids, hipStream_t s) {
  const int32_t avg = a.num_segments > 0 ? (int32_t)(num_ids / a.num_segments) : 0;
  // segments per group: one.  More (a chunk of ids then serves several segments: one id load per G * IDR / fanout
  // segments) lowers the L2-resident floor but loses on every real request (profiles/r04/agg_probe_*): more, shorter
  // waves keep more independent row loads in flight.  GLX_AGG_SEGS overrides.
  int32_t S = 1;
  const int want = agg_knobs().segs.load(std::memory_order_relaxed);
  // ... except over a table small enough that most of a big request is served on-die (<= 1 GiB = four Infinity Caches;
  // round 6): such a launch is not waiting for HBM but for its own vector-memory pipeline -- C5's item -> shop reduce
  // (6.55 M ids over the 1 GB shop table: three quarters of its row reads hit L1, the per-CU TA/TCP/TD path busy ~95 % of the
  // launch, profiles/r06/c5_is_reduce.md) -- and there three segments per group (one id chunk serves all three, a
  // third of the waves to launch and drain) took 0.49 -> 0.43 ms, while the same setting LOSES on the tables HBM
  // serves: C2 (1.2 GB) 0.55 -> 0.63, C4 0.98 -> 1.08, C3 (10 GB) 1.84 -> 1.84 (profiles/r06/agg_probe_*_segs.txt).
  // Small requests stay at one (a group per segment fills the chip sooner).
  // (the test is on the table's bytes: a half table of twice the rows is as small)
  constexpr int64_t kElemBytes = sizeof(typename AggElem<DT>::raw);
  if (NSRC == 1 && (int64_t)a.num_rows * a.stride * kElemBytes <= ((int64_t)1 << 30) && a.num_segments >= 3 * 32768) S = 3;
  if (want > 0) S = want;
  if (S > G - 1) S = G - 1;  // lane j of the group holds the start of its j-th segment (and lane S the end)
  if (S < 1) S = 1;
  a.segs_per_group = S;
  a.store_mode = agg_knobs().store.load(std::memory_order_relaxed);
  // Max / Min, a whole wave per segment: rows a segment has already folded are not loaded again (agg_first_occurrences)
  // when the segments average kAggSkipMinLen positions or more.  Same process, six alternations, C3 store, ms with every
  // position loaded -> first occurrences only (profiles/r16/agg_repeat_ab.txt): hop 1 (fanout 25, 5.25 distinct rows per
  // segment) 0.0928 -> 0.0713; hop 2 (fanout 10, 8.78 distinct) 1.6026 -> 1.6384, a LOSS beyond the spread: its saved
  // loads are cache hits of a fabric-bound launch and the mask loop delays every wave's first load; rows uniform over
  // the table (nothing to skip) 3.5054 -> 3.5097.  Those two launches give 5 ns per mask iteration against 18 ns per
  // load saved, i.e. the masks pay once more than a fifth of the positions repeat -- which the launcher cannot see, so
  // the rule is on what it can: the longer a segment of draws with replacement, the larger that share, and 16 lies
  // between the fanout that lost and the one that won.  GLX_AGG_REPEATS = 1 loads every position whatever the length
  // (the behaviour before round 16), 2 skips whatever the length.
  const int repeats = agg_knobs().repeats.load(std::memory_order_relaxed);
  a.load_repeats = repeats == 1 ? 1 : (repeats == 2 ? 0 : (avg >= kAggSkipMinLen ? 0 : 1));
  const int64_t groups = ((int64_t)a.num_segments + S - 1) / S;
  const int64_t seg_blocks = (groups + (256 / G) - 1) / (256 / G);
  const int32_t nsl = a.xcd_slices > 1 ? a.xcd_slices : 1;
  const int64_t blocks = seg_blocks * nsl;
  const unsigned grid = (unsigned)blocks;
  // XCD stripes (agg_stripe_block): whole runs of (8 / n) * chunk segment blocks are permuted, the tail stays in order
  if (a.stripe_chunk > 0 && nsl < 8) {
    const int64_t span = (int64_t)(8 / nsl) * a.stripe_chunk;
    a.stripe_full = (uint32_t)(seg_blocks / span * span);
  } else {
    a.stripe_chunk = 0;
    a.stripe_full = 0;
  }
  // occupancy cap (experiment): k workgroups per CU by declaring 160 KiB / k of LDS nobody touches
  const int occ = agg_knobs().occ.load(std::memory_order_relaxed);
  const size_t lds = (occ >= 3 && occ <= 7) ? (size_t)(160 * 1024 / occ) & ~(size_t)255 : 0;
  switch (agg_grp_unroll(a.seg_start ? 0 : a.fanout, avg)) {
    case 6: glx_aggregate_grp_kernel<OP, G, VEC, 6, NSRC, IDR, DT><<<grid, 256, lds, s>>>(a); break;
    case 8: glx_aggregate_grp_kernel<OP, G, VEC, 8, NSRC, IDR, DT><<<grid, 256, lds, s>>>(a); break;
    case 12: glx_aggregate_grp_kernel<OP, G, VEC, 12, NSRC, IDR, DT><<<grid, 256, lds, s>>>(a); break;
    case 15: glx_aggregate_grp_kernel<OP, G, VEC, 15, NSRC, IDR, DT><<<grid, 256, lds, s>>>(a); break;
    default: glx_aggregate_grp_kernel<OP, G, VEC, 10, NSRC, IDR, DT><<<grid, 256, lds, s>>>(a); break;
  }
}

// The grouped kernel at G = 64 / 32 / 16 / 8 lanes per segment for `lanes` = columns / VEC.
template <int OP, int VEC, int NSRC, int DT>
void launch_agg_grp_g(const AggArgs& a, int lanes, int32_t num_ids, hipStream_t s) {
  if (lanes >= 64) launch_agg_grp<OP, 64, VEC, NSRC, 1, DT>(a, num_ids, s);
  else if (lanes >= 32) launch_agg_grp<OP, 32, VEC, NSRC, 1, DT>(a, num_ids, s);
  else if (lanes >= 16) launch_agg_grp<OP, 16, VEC, NSRC, 1, DT>(a, num_ids, s);
  else launch_agg_grp<OP, 8, VEC, NSRC, 2, DT>(a, num_ids, s);
}

template <int OP, int NSRC, int DT>
void launch_agg_cols(const AggArgs& a0, int32_t num_ids, int want_xcd, hipStream_t s) {
  AggArgs a = a0;
  // the per-segment kernel's VEC = 4 path: 4 elements per lane (16 bytes of floats, 8 of halves, 4 of float8).  The
  // tests below are in elements: a 16-byte-aligned base and a pitch that is a multiple of 4 elements keep every
  // 4-column load aligned for every element size, one byte included -- so an odd dim, an odd view pitch or a view
  // whose base is off by 1-3 bytes takes the scalar path.
  bool vec4 = a.dim % 4 == 0 && a.ncols % 4 == 0 && a.col0 % 4 == 0 && (reinterpret_cast<uintptr_t>(a.emb_out) & 15) == 0 &&
              (reinterpret_cast<uintptr_t>(a.X) & 15) == 0 && (a.stride % 4) == 0;
  if (NSRC > 1) {
    vec4 = vec4 && (reinterpret_cast<uintptr_t>(a.X1) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.X2) & 15) == 0 &&
           (a.stride1 % 4) == 0 && (a.stride2 % 4) == 0;
  }
  // the grouped kernel: EV = 4 elements per lane, one load per row -- 16 bytes of floats, 8 of halves, 4 of float8
  // -- so a half table keeps the float32 lane-to-column map, group size and slicing.  Measured on the C3 hop-2 request
  // (profiles/r08/half_features.txt, bfloat16, same process, ms): 8-byte loads 1.24 (whole rows) / 1.33 (two slices)
  // against 16-byte loads of 8 columns per lane -- half the lanes per segment, so G = 32 at D = 256 and no scalar
  // row path -- 1.62 / 1.65, no faster than the float32 table's 1.63.  GLX_AGG_HALF_LD16=1 selects the 16-byte
  // loads (every dimension, pitch and offset a multiple of 8 elements).
  // float8 turns out the other way round where rows are long (profiles/r29/fp8_features.txt, same process, ms, 4 / 8
  // columns per lane): C3 hop-2 (D = 256) 1.04 / 0.80 on the sampled ids and 1.12 / 1.02 on uniformly random ones --
  // 8-byte loads, two segments per wave -- but C2's shape (D = 128, G = 16) 0.50 / 0.53 and 0.83 / 0.82.  So float8
  // rows of >= 256 columns take 8 columns per lane when every dimension, pitch and offset allows it, narrower ones
  // keep 4.  GLX_AGG_HALF_LD16=2 selects 4 columns per lane for every type (the ablation of this rule).
  int ev = 4;
  if constexpr (DT != GLX_DTYPE_F32) {
    const int ld16 = agg_knobs().half_ld16.load(std::memory_order_relaxed);
    const bool fits8 = vec4 && a.dim % 8 == 0 && a.ncols % 8 == 0 && a.col0 % 8 == 0 && (a.stride % 8) == 0;
    if (ld16 == 1 || (ld16 == 0 && glx_dtype_is_f8(DT) && a.ncols >= 256 && fits8)) ev = 8;
  }
  const bool wide = vec4 && a.dim % ev == 0 && a.ncols % ev == 0 && a.col0 % ev == 0 && (a.stride % ev) == 0;
  // the grouped kernel reads row 0 in place of an unknown id's row: some row must exist
  const bool has_rows = NSRC > 1 ? (a.X2 != nullptr || a.base2 > 0) : a.num_rows > 0;
  if (wide && has_rows && a.ncols >= 8 * ev && agg_knobs().legacy.load(std::memory_order_relaxed) == 0) {
    if (want_xcd > 1 && a.col0 == 0 && a.ncols == a.dim && a.dim % (ev * want_xcd) == 0 && a.dim / want_xcd >= 8 * ev) {
      a.xcd_slices = want_xcd;  // only the grouped kernel knows about slices
      a.ncols = a.dim / want_xcd;
    }
    // lanes per segment, 16-byte loads each.  (8-byte loads over twice the lanes -- a whole wave per 128-column slice
    // keeps the scalar row path -- were measured and dropped: equal on uniform rows, 13 % slower on the power-law
    // request; profiles/r04/agg_probe_*_run4.txt.  The kernel keeps its VEC parameter.)
    if constexpr (DT != GLX_DTYPE_F32) {
      if (ev == 8) {
        launch_agg_grp_g<OP, 8, NSRC, DT>(a, a.ncols / 8, num_ids, s);
        return;
      }
    }
    launch_agg_grp_g<OP, 4, NSRC, DT>(a, a.ncols / 4, num_ids, s);
    return;
  }
  if (vec4) {
    const int lanes = a.ncols / 4;
    if (lanes >= 64) launch_agg_g<OP, 64, 4, NSRC, DT>(a, s);
    else if (lanes >= 32) launch_agg_g<OP, 32, 4, NSRC, DT>(a, s);
    else if (lanes >= 16) launch_agg_g<OP, 16, 4, NSRC, DT>(a, s);
    else if (lanes >= 8) launch_agg_g<OP, 8, 4, NSRC, DT>(a, s);
    else if (lanes >= 4) launch_agg_g<OP, 4, 4, NSRC, DT>(a, s);
    else if (lanes >= 2) launch_agg_g<OP, 2, 4, NSRC, DT>(a, s);
    else launch_agg_g<OP, 1, 4, NSRC, DT>(a, s);
  } else {
    const int lanes = a.ncols;
    if (lanes >= 64) launch_agg_g<OP, 64, 1, NSRC, DT>(a, s);
    else if (lanes >= 16) launch_agg_g<OP, 16, 1, NSRC, DT>(a, s);
    else if (lanes >= 4) launch_agg_g<OP, 4, 1, NSRC, DT>(a, s);
    else launch_agg_g<OP, 1, 1, NSRC, DT>(a, s);
  }
}

// Column slices.
//  * XCD-affine slices (the default for big requests): ONE launch, workgroup b reduces column slice b % n.  With the
//    observed b % 8 workgroup -> XCD placement each XCD's 4 MB L2 then holds 1 / n of every hub row instead of whole
//    rows of 1 / 8 of the segments: n times as many hub rows stay L2-resident per XCD, at the price of reading the ids
//    n times and of 1 / n-row pieces.  Measured (profiles/r04/agg_probe_*_run4.txt, same process, ms): C3 hop-2
//    (D = 256, 16.4 M ids) n = 1 / 2 / 4: 1.96 / 1.85 / 1.82 on the power-law request, 3.48 / 3.52 / 3.72 on uniformly
//    random rows; C2 (D = 128) 0.633 / 0.561 / 0.596 and 0.853 / 0.881 / 0.929; C4's shape 1.03 / 0.96 / 1.07 and
//    1.86 / 1.90 / 1.98.  n = 2 is the default: -6 .. -11 % where rows are re-used, +1 .. 3 % where none is; small
//    requests (C3 hop 1: 0.098 -> 0.120 ms) stay whole.  GLX_AGG_XCD_SLICES = 1 (off) | 2 | 4 | 8 overrides.
//  * XCD stripes (agg_stripe_block; the default for the same requests of >= 4 M ids): the XCDs that share a slice
//    walk contiguous chunks of kXcdStripeChunk segment blocks instead of every (8 / n)-th block, so a seed's hop-1
//    samples and their twins' shared rows are fetched into ONE L2.  This moves the slice trade-off: measured
//    (profiles/r07/stripe_ab.txt, same process, 6 alternations, ms; old default = n 2 without stripes): C3 hop-2
//    1.829 -> 1.609 with n = 1 (n = 2 with stripes: 1.690), degree-biased seeds 1.991 -> 1.977 (n = 2: 1.957), C2 0.552
//    -> 0.535 with n = 2 (n = 1: 0.579), C4's shape 0.962 -> 0.926 with n = 2 (n = 1: 0.947), uniformly random rows
//    3.295 -> 3.217.  So with stripes, rows of >= 256 floats take n = 1 and narrower rows keep n = 2.  Chunks of
//    16 / 32 / 64 / 256 blocks are within 1 % of each other; requests under 4 M ids stay in order (C3 hop 1:
//    0.098 -> 0.100 with stripes).  The other users of the grouped kernel take the stripes under the same rule: three
//    segments per group (C5's item -> shop reduce, 6.55 M ids: bench.py --workload c5, three interleaved runs each,
//    0.677 -> 0.686 ms/step by median -- inside its 2 % run-to-run spread, profiles/r07/bench_ab_interleaved.txt), the
//    3-source distributed reduce and explicit segment_ids (the permutation moves whole segment blocks, so neither the
//    row source nor the segment bounds see it).  GLX_AGG_XCD_STRIPES = 0 (off) | 1 and GLX_AGG_XCD_CHUNK override.
//  * GLX_AGG_SLICES = n: the columns in n slices, one LAUNCH after the other (ablation; profiles/r02: no gain).
constexpr int32_t kXcdSliceMinIds = 4 << 20;
constexpr int32_t kXcdStripeChunk = 64;

template <int OP, int NSRC, int DT>
void launch_agg_n(const AggArgs& a0, int32_t num_ids, hipStream_t s) {
  AggArgs a = a0;
  a.col0 = 0;
  a.ncols = a.dim;
  a.xcd_slices = 0;
  int stripes = agg_knobs().stripes.load(std::memory_order_relaxed);
  if (stripes < 0) stripes = num_ids >= kXcdSliceMinIds ? 1 : 0;
  int xcd = agg_knobs().xcd.load(std::memory_order_relaxed);
  if (xcd == 0) {  // by columns for every storage type: a half table at D = 256 is fastest whole, too (r08)
    xcd = (num_ids >= kXcdSliceMinIds && a.dim % 8 == 0 && a.dim >= 128) ? 2 : 1;
    if (xcd == 2 && stripes > 0 && a.dim >= 256) xcd = 1;
  }
  int slices = agg_knobs().slices.load(std::memory_order_relaxed);
  if ((slices != 2 && slices != 4 && slices != 8) || a.dim % (4 * slices) != 0) slices = 1;
  if (xcd != 2 && xcd != 4 && xcd != 8) xcd = 1;
  int chunk = agg_knobs().chunk.load(std::memory_order_relaxed);
  if (chunk <= 0) chunk = kXcdStripeChunk;
  a.stripe_chunk = stripes > 0 ? chunk : 0;
  for (int c = 0; c < slices; ++c) {
    a.ncols = a.dim / slices;
    a.col0 = c * a.ncols;
    launch_agg_cols<OP, NSRC, DT>(a, num_ids, slices == 1 ? xcd : 1, s);
  }
}

template <int OP>
void launch_agg(const AggArgs& a, int32_t num_ids, hipStream_t s) {
  if (a.X1 || a.X2) launch_agg_n<OP, 3, GLX_DTYPE_F32>(a, num_ids, s);  // the distributed store: float32 only
  else if (a.dtype == GLX_DTYPE_BF16) launch_agg_n<OP, 1, GLX_DTYPE_BF16>(a, num_ids, s);
  else if (a.dtype == GLX_DTYPE_F16) launch_agg_n<OP, 1, GLX_DTYPE_F16>(a, num_ids, s);
  else if (a.dtype == GLX_DTYPE_F8E4M3) launch_agg_n<OP, 1, GLX_DTYPE_F8E4M3>(a, num_ids, s);
  else if (a.dtype == GLX_DTYPE_F8E5M2) launch_agg_n<OP, 1, GLX_DTYPE_F8E5M2>(a, num_ids, s);
  else launch_agg_n<OP, 1, GLX_DTYPE_F32>(a, num_ids, s);
}

// Upload: row r of the caller's dense [V, D] matrix -> its (swizzled, pitched) slot.  SRC / DST: element types of
// the caller's matrix and of the table; float32 -> half / float8 rounds (glx_f32_to_bf16_bits and its siblings),
// equal types copy the bits.
template <int SRC, int DST>
__global__ void glx_place_rows_kernel(const void* __restrict__ src_v, int64_t num_rows, int32_t dim,
                                      int64_t stride, int64_t swizzle_rows, void* __restrict__ dst_v) {
  typedef typename std::conditional<SRC == GLX_DTYPE_F32, uint32_t, typename std::conditional<glx_dtype_is_f8(SRC), uint8_t, uint16_t>::type>::type src_t;
  typedef typename std::conditional<DST == GLX_DTYPE_F32, uint32_t, typename std::conditional<glx_dtype_is_f8(DST), uint8_t, uint16_t>::type>::type dst_t;
  const src_t* __restrict__ src = static_cast<const src_t*>(src_v);
  dst_t* __restrict__ dst = static_cast<dst_t*>(dst_v);
  const int64_t total = num_rows * (int64_t)dim;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += step) {
    const int64_t r = t / dim;
    const int32_t c = (int32_t)(t - r * dim);
    dst_t v;
    if constexpr (SRC == DST) v = src[t];
    else if constexpr (DST == GLX_DTYPE_BF16) v = glx_f32_to_bf16_bits(src[t]);
    else if constexpr (DST == GLX_DTYPE_F8E4M3) v = glx_f32_to_f8e4m3_bits(src[t]);
    else if constexpr (DST == GLX_DTYPE_F8E5M2) v = glx_f32_to_f8e5m2_bits(src[t]);
    else v = glx_f32_to_f16_bits(src[t]);
    dst[glx_swizzle_row(r, swizzle_rows) * stride + c] = v;
  }
}

// Feature gather (LookupNodes float attributes): G lanes per output row; a half table's rows are upcast to float32.
template <int DT>
__global__ __launch_bounds__(256) void glx_lookup_kernel(GlxIdMap map, const void* __restrict__ Xv,
                                                         int64_t stride, int64_t swizzle_rows, int32_t dim, const int64_t* __restrict__ ids,
                                                         int64_t n, float default_attr,
                                                         float* __restrict__ out, int G) {
  const typename AggElem<DT>::raw* __restrict__ X = static_cast<const typename AggElem<DT>::raw*>(Xv);
  const int64_t gid = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / G;
  const int c = threadIdx.x % G;
  if (gid >= n) return;
  int64_t row = glx_row_of(map, ids[gid]);
  if (row >= 0) row = glx_swizzle_row(row, swizzle_rows);
  float* o = out + gid * (int64_t)dim;
  // 4 elements per lane: a float32 table's rows as they always were; a half or float8 table's only when its rows are
  // 8-byte aligned (a view's pitch is its dim, its base the caller's; a float8 load of 4 columns needs 4 bytes)
  bool vec4 = (dim & 3) == 0;
  if constexpr (DT != GLX_DTYPE_F32) vec4 = vec4 && (stride & 3) == 0 && (reinterpret_cast<uintptr_t>(Xv) & 7) == 0;
  if (vec4) {
    for (int32_t col = c * 4; col < dim; col += G * 4) {
      float4 v = make_float4(default_attr, default_attr, default_attr, default_attr);
      if (row >= 0) {
        const float __attribute__((ext_vector_type(4))) q = agg_load<DT, 4>(X + row * stride + col);
        v = make_float4(q[0], q[1], q[2], q[3]);
      }
      *reinterpret_cast<float4*>(o + col) = v;
    }
  } else {
    for (int32_t col = c; col < dim; col += G) o[col] = row >= 0 ? AggElem<DT>::up(X[row * stride + col]) : default_attr;
  }
}

int run_aggregate(AggArgs& a, int op, const int32_t* d_seg, int32_t num_ids, hipStream_t s) {
  GlxKernelTimer timer(GLX_KERNEL_AGGREGATE, s);
  if (agg_use_mfma(a, op)) {  // ablation knob (GLX_AGG_MFMA=1): the LDS-staged MFMA formulation of Sum / Mean
    if (op == GLX_AGG_SUM) launch_agg_mfma<GLX_AGG_SUM>(a, s);
    else launch_agg_mfma<GLX_AGG_MEAN>(a, s);
    timer.stop();
    return GLX_OK;
  }
  switch (op) {
    case GLX_AGG_SUM: launch_agg<GLX_AGG_SUM>(a, num_ids, s); break;
    case GLX_AGG_MEAN: launch_agg<GLX_AGG_MEAN>(a, num_ids, s); break;
    case GLX_AGG_MAX: launch_agg<GLX_AGG_MAX>(a, num_ids, s); break;
    case GLX_AGG_MIN: launch_agg<GLX_AGG_MIN>(a, num_ids, s); break;
    case GLX_AGG_PROD: launch_agg<GLX_AGG_PROD>(a, num_ids, s); break;
    default: break;
  }
  timer.stop();
  return GLX_OK;
}

// Segment bookkeeping shared by the single-table and the multi-source entry: fills
// a.seg_start (or a.fanout for uniform segments) from scratch laid out by the caller.
// scratch = seg_start (Sg + 1) + kSegScratchExtra int32 (a captured call's two words).
namespace {
// Two 64-bit words per (calling thread, device, stream) -- the same scope as the scratch workspace, so that host
// threads that share a stream (the default one, say) do not raise each other's words -- zeroed when made, freed with the
// thread.  The epoch that tags them is the BUFFER's own counter (round 6; a process-wide counter wrapped after 2^32
// explicit-segment_ids calls of all threads together, after which stale words carried larger tags than new calls and
// atomicMax never landed: ADVICE r05): every call on a buffer is ordered on its stream, so when the counter wraps the
// words are cleared by a memset on that stream and counting restarts at 1 -- no tag of an earlier lap can be seen again.
// A recycled stream handle finds words of an older epoch of the same buffer, which read as "nothing raised".
struct SegBuf {
  int dev;
  hipStream_t stream;
  unsigned long long* words;
  uint32_t epoch;  // the last epoch handed out (0 = none yet: 0 tags the zeroed words)
};
constexpr size_t kSegBufsMax = 64;  // streams a thread keeps words for; the oldest goes when a 65th shows up
struct SegWords {
  std::vector<SegBuf> bufs;
  ~SegWords() {
    for (auto& e : bufs) {  // best effort: at process exit the runtime may already be gone
      if (hipSetDevice(e.dev) == hipSuccess) (void)hipFree(e.words);
    }
    (void)hipGetLastError();
  }
};
thread_local SegWords g_seg_words;

// *out = the words of (this thread, the current device, s) and the next epoch on them.  Never called while s is being
// captured (prepare_segments keeps a captured call's words in the call's own scratch): it may allocate.
int seg_words_for(hipStream_t s, unsigned long long** out, uint32_t* epoch) {
  int dev = 0;
  GLX_HIP(hipGetDevice(&dev));
  SegBuf* buf = nullptr;
  for (auto& e : g_seg_words.bufs) {
    if (e.dev == dev && e.stream == s) {
      buf = &e;
      break;
    }
  }
  if (buf == nullptr) {
    if (g_seg_words.bufs.size() >= kSegBufsMax) {  // streams come and go: drop the oldest (hipFree waits for its readers)
      const SegBuf old = g_seg_words.bufs.front();
      g_seg_words.bufs.erase(g_seg_words.bufs.begin());
      GlxDeviceGuard guard(old.dev);
      (void)hipFree(old.words);
    }
    unsigned long long* p = nullptr;
    GLX_HIP(hipMalloc(&p, 256));
    GLX_HIP(hipMemsetAsync(p, 0, 256, s));  // ordered before the first scan on this stream
    g_seg_words.bufs.push_back(SegBuf{dev, s, p, 0u});
    buf = &g_seg_words.bufs.back();
  }
  if (++buf->epoch == 0) {  // wrapped: clear the words behind every earlier call of this stream, restart at 1
    GLX_HIP(hipMemsetAsync(buf->words, 0, 16, s));
    buf->epoch = 1;
  }
  *out = buf->words;
  *epoch = buf->epoch;
  return GLX_OK;
}

// *out = the compute units of the current device: what the bookkeeping grids are sized to.  Asked of the runtime once
// per device (an attribute query, no stream work: allowed while a stream is being captured).
int seg_device_cus(int* out) {
  static std::atomic<int> known[64];
  int dev = 0;
  GLX_HIP(hipGetDevice(&dev));
  int cus = (dev >= 0 && dev < 64) ? known[dev].load(std::memory_order_relaxed) : 0;
  if (cus <= 0) {
    GLX_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    GLX_REQUIRE(cus > 0, "device %d reports %d compute units", dev, cus);
    if (dev >= 0 && dev < 64) known[dev].store(cus, std::memory_order_relaxed);
  }
  *out = cus;
  return GLX_OK;
}
}  // namespace

// (kSegScratchExtra -- the int32 words behind seg_start[num_segments + 1] -- is declared in glx_common.h)

int prepare_segments(AggArgs& a, const int32_t* d_seg, int32_t num_ids, int32_t num_segments, int32_t* scratch,
                     hipStream_t s) {
  a.fanout = num_segments > 0 ? num_ids / num_segments : 0;
  memset(&a.seg_state, 0, sizeof(a.seg_state));
  if (d_seg == nullptr) {  // uniform segments: nothing to derive, nothing to read
    a.seg_start = nullptr;
    return GLX_OK;
  }
  int32_t* seg_start = scratch;
  unsigned long long* words = nullptr;
  SegState st;
  // A captured launch is replayed with the SAME epoch: the words a replay raised would still carry it in the next
  // replay -- and the per-stream buffer may not even exist yet (no allocation inside a capture), nor is the capture
  // stream the one a replay runs on.  A captured call therefore keeps its two words in its OWN scratch (the plan's
  // replayable arena), cleared by one more node of the graph.
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &capturing) == hipSuccess && capturing != hipStreamCaptureStatusNone) {
    const uintptr_t at = (reinterpret_cast<uintptr_t>(scratch + (size_t)num_segments + 1) + 7) & ~(uintptr_t)7;
    words = reinterpret_cast<unsigned long long*>(at);
    st.epoch = 1;
    glx_seg_reset_kernel<<<1, 1, 0, s>>>(words);
  } else {
    int rc = seg_words_for(s, &words, &st.epoch);
    if (rc != GLX_OK) return rc;
  }
  // uniform segments are possible when the ids divide evenly; the scan then checks seg[i] == i / fanout
  const int32_t f = (num_segments > 0 && num_ids > 0 && num_ids % num_segments == 0) ? num_ids / num_segments : 0;
  st.words = words;
  st.floor_level = num_ids == 0 ? 2 : (f > 0 ? 0 : 1);
  const bool parent = agg_knobs().seg_parent.load(std::memory_order_relaxed) != 0;
  int64_t fixup_grid = ((int64_t)num_segments + 1 + 255) / 256;
  if (parent) {
    if (num_ids > 0) {
      glx_seg_scan_parent_kernel<<<(unsigned)(((int64_t)num_ids + 1023) / 1024), 256, 0, s>>>(d_seg, num_ids, num_segments, f,
                                                                                            words, st.epoch, seg_start);
    }
  } else {
    int cus = 0;
    int rc = seg_device_cus(&cus);
    if (rc != GLX_OK) return rc;
    if (num_ids > 0) {
      // a few workgroups per CU that walk the request in tiles: a wave moves 4 KiB per tile, not 1 KiB in its life
      int64_t grid = ((int64_t)num_ids + kSegScanTile - 1) / kSegScanTile;  // never more: the kernel's 32-bit counters
      if (grid > (int64_t)cus * kSegScanWgPerCu) grid = (int64_t)cus * kSegScanWgPerCu;
      const int cap = agg_knobs().seg_wgs.load(std::memory_order_relaxed);
      if (cap > 0 && grid > cap) grid = cap;
      glx_seg_scan_kernel<<<(unsigned)grid, kSegScanThreads, 0, s>>>(d_seg, num_ids, num_segments, f, words, st.epoch, seg_start);
    }
    if (fixup_grid > (int64_t)cus * kSegFixupWgPerCu) fixup_grid = (int64_t)cus * kSegFixupWgPerCu;
  }
  glx_seg_fixup_kernel<<<(unsigned)fixup_grid, 256, 0, s>>>(d_seg, st, num_ids, num_segments, seg_start);
  a.seg_start = seg_start;
  a.seg_state = st;
  return GLX_OK;
}

int aggregate_device(const glx_features* f, int op, const int64_t* d_ids, const int32_t* d_seg,
                     int32_t num_ids, int32_t num_segments, float default_attr, float* d_emb,
                     int32_t* d_cnt, hipStream_t s) {
  // scratch: seg_start (Sg+1) [+ rows (N) for hashed ids]
  const bool hashed = f->idmap.any();  // raw ids are not rows: translate first (a table lookup, or arithmetic)
  const size_t n_i32 = (size_t)num_segments + 1 + kSegScratchExtra + (hashed ? (size_t)num_ids : 0);
  GlxScratch lease;
  int rc = lease.alloc(n_i32 * sizeof(int32_t), s, 1);
  if (rc != GLX_OK) return rc;
  int32_t* scratch = lease.as<int32_t>();
  int32_t* rows = hashed ? scratch + num_segments + 1 + kSegScratchExtra : nullptr;
  AggArgs a;
  memset(&a, 0, sizeof(a));
  rc = prepare_segments(a, d_seg, num_ids, num_segments, scratch, s);
  if (rc != GLX_OK) return rc;
  if (hashed && num_ids > 0) {
    glx_rows_kernel<<<(unsigned)((num_ids + 255) / 256), 256, 0, s>>>(f->map(), d_ids, num_ids, rows);
  }
  a.X = f->X;
  a.dtype = f->dtype;
  a.node_ids = hashed ? nullptr : d_ids;
  a.rows = rows;
  a.emb_out = d_emb;
  a.cnt_out = d_cnt;
  a.num_rows = f->num_rows;
  a.stride = f->stride;
  a.swizzle_rows = f->swizzle_rows;
  a.dim = f->dim;
  a.num_segments = num_segments;
  a.default_attr = default_attr;
  run_aggregate(a, op, d_seg, num_ids, s);
  GLX_HIP(hipGetLastError());
  return GLX_OK;
}

// ---- AggregatingResponse::Stitch (aggregating_request.cc:172-213) on the device:
// fold P partial results [P][Sg][dim] in shard order, starting from InitFunc's
// value.  Pure streaming (reads P*Sg*dim*4 B once, coalesced; writes Sg*dim*4 B):
// one thread per VEC output columns of one segment.
template <int OP, int VEC>
__global__ __launch_bounds__(256) void glx_agg_stitch_kernel(const float* __restrict__ parts,
                                                             const int32_t* __restrict__ cnts, int32_t P,
                                                             int64_t num_segments, int32_t dim,
                                                             float default_attr, float* __restrict__ out,
                                                             int32_t* __restrict__ cnt_out) {
  const int32_t cols = dim / VEC;
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= num_segments * cols) return;
  const int64_t sg = t / cols;
  const int32_t c0 = (int32_t)(t - sg * cols) * VEC;
  float acc[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc[v] = agg_init<OP>();
  int32_t total = 0;
  for (int32_t p = 0; p < P; ++p) {
    const int32_t c = cnts[(int64_t)p * num_segments + sg];
    if (c == 0) continue;  // this shard saw none of the segment's ids
    const float* src = parts + ((int64_t)p * num_segments + sg) * dim + c0;
    float r[VEC];
    if (VEC == 4) {
      const float4 q = *reinterpret_cast<const float4*>(src);
      r[0] = q.x; r[1 % VEC] = q.y; r[2 % VEC] = q.z; r[3 % VEC] = q.w;
    } else {
      r[0] = src[0];
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      // Mean: left += right * segments[i] (mean_aggregator.cc:31-37)
      const float x = OP == GLX_AGG_MEAN ? r[v] * (float)c : r[v];
      acc[v] = agg_combine<OP>(acc[v], x);
    }
    total += c;
  }
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    if (total == 0) acc[v] = default_attr;                       // aggregator.cc:74-86
    else if (OP == GLX_AGG_MEAN) acc[v] = acc[v] / (float)total;  // mean_aggregator.cc:45-61
  }
  float* dst = out + sg * dim + c0;
  if (VEC == 4) *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1 % VEC], acc[2 % VEC], acc[3 % VEC]);
  else dst[0] = acc[0];
  if (c0 == 0) cnt_out[sg] = total;
}

template <int OP>
void launch_agg_stitch(bool vec4, const float* parts, const int32_t* cnts, int32_t P, int64_t sg, int32_t dim,
                       float default_attr, float* out, int32_t* cnt_out, hipStream_t s) {
  const int64_t threads = sg * (vec4 ? dim / 4 : dim);
  const unsigned grid = (unsigned)((threads + 255) / 256);
  if (vec4) glx_agg_stitch_kernel<OP, 4><<<grid, 256, 0, s>>>(parts, cnts, P, sg, dim, default_attr, out, cnt_out);
  else glx_agg_stitch_kernel<OP, 1><<<grid, 256, 0, s>>>(parts, cnts, P, sg, dim, default_attr, out, cnt_out);
}

}  // namespace

// glx_dist.hip: segmented reduce over pre-resolved virtual rows of up to three sources
// (own shard, hot-row replica, halo rows); vrows[i] = -1 is the default row.
int glx_aggregate_vrows_device(const GlxRowSource* src, int nsrc, int32_t dim, int op, const int32_t* vrows,
                               const int32_t* d_seg, int32_t num_ids, int32_t num_segments, float default_attr,
                               float* d_emb, int32_t* d_cnt, hipStream_t s) {
  GlxScratch lease;
  int rc = lease.alloc(((size_t)num_segments + 1 + kSegScratchExtra) * sizeof(int32_t), s, 1);
  if (rc != GLX_OK) return rc;
  int32_t* scratch = lease.as<int32_t>();
  AggArgs a;
  memset(&a, 0, sizeof(a));
  rc = prepare_segments(a, d_seg, num_ids, num_segments, scratch, s);
  if (rc != GLX_OK) return rc;
  const GlxRowSource none{nullptr, dim, 0, 0};
  const GlxRowSource& s0 = nsrc > 0 ? src[0] : none;
  const GlxRowSource& s1 = nsrc > 1 ? src[1] : none;
  const GlxRowSource& s2 = nsrc > 2 ? src[2] : none;
  a.X = s0.X;
  a.stride = s0.stride;
  a.swizzle_rows = s0.swizzle_rows;
  a.num_rows = s0.rows;
  a.X1 = s1.X;
  a.stride1 = s1.stride;
  a.swizzle1 = s1.swizzle_rows;
  a.X2 = s2.X;
  a.stride2 = s2.stride;
  a.base1 = (int32_t)s0.rows;
  a.base2 = (int32_t)(s0.rows + s1.rows);
  // the multi-source kernel is selected by a non-null X1 / X2; with neither (no replica, no
  // halo) the single-table kernel reads the same rows
  a.node_ids = nullptr;
  a.rows = vrows;
  a.emb_out = d_emb;
  a.cnt_out = d_cnt;
  a.dim = dim;
  a.num_segments = num_segments;
  a.default_attr = default_attr;
  run_aggregate(a, op, d_seg, num_ids, s);
  GLX_HIP(hipGetLastError());
  return GLX_OK;
}

// glx_common.h: the segment bookkeeping for the kernels of glx_aggregate_grad.hip (prepare_segments above).
int glx_segments_prepare(const int32_t* d_seg, int32_t num_ids, int32_t num_segments, int32_t* scratch, hipStream_t s,
                         GlxSegments* out) {
  AggArgs a;
  memset(&a, 0, sizeof(a));
  const int rc = prepare_segments(a, d_seg, num_ids, num_segments, scratch, s);
  if (rc != GLX_OK) return rc;
  out->seg_start = a.seg_start;
  out->state = a.seg_state;
  out->fanout = a.fanout;
  return GLX_OK;
}

extern "C" int glx_tune(const char* name, int32_t value) {
  GLX_REQUIRE(name != nullptr, "name is NULL");
  AggKnobs& k = agg_knobs();
  std::atomic<int>* slot = nullptr;
  if (strcmp(name, "agg_mfma") == 0) slot = &k.mfma;
  else if (strcmp(name, "agg_unroll") == 0) slot = &k.unroll;
  else if (strcmp(name, "agg_slices") == 0) slot = &k.slices;
  else if (strcmp(name, "agg_legacy") == 0) slot = &k.legacy;
  else if (strcmp(name, "agg_segs") == 0) slot = &k.segs;
  else if (strcmp(name, "agg_xcd_slices") == 0) slot = &k.xcd;
  else if (strcmp(name, "agg_occupancy") == 0) slot = &k.occ;
  else if (strcmp(name, "agg_store") == 0) slot = &k.store;
  else if (strcmp(name, "agg_xcd_stripes") == 0) slot = &k.stripes;
  else if (strcmp(name, "agg_xcd_chunk") == 0) slot = &k.chunk;
  else if (strcmp(name, "agg_half_ld16") == 0) slot = &k.half_ld16;
  else if (strcmp(name, "agg_repeats") == 0) slot = &k.repeats;
  else if (strcmp(name, "seg_scan_parent") == 0) slot = &k.seg_parent;
  else if (strcmp(name, "seg_scan_wgs") == 0) slot = &k.seg_wgs;
  else if (strcmp(name, "seg_epochs_before_wrap") == 0) {
    // test aid: the calling thread's segment-word buffers hand out `value` more epochs before their counter wraps
    GLX_REQUIRE(value >= 0, "seg_epochs_before_wrap must be >= 0");
    for (auto& e : g_seg_words.bufs) e.epoch = 0xffffffffu - (uint32_t)value;
    return GLX_OK;
  }
  if (slot == nullptr) {  // the side paths' knobs (glx_common.h GlxSideKnobs): -1 restores the default
    GlxSideKnobs& sk = glx_side_knobs();
    std::atomic<int64_t>* side = nullptr;
    if (strcmp(name, "cond_sequential") == 0) side = &sk.cond_sequential;
    else if (strcmp(name, "dist_no_bitmap") == 0) side = &sk.dist_no_bitmap;
    else if (strcmp(name, "filter_span_cap") == 0) side = &sk.filter_span_cap;
    else if (strcmp(name, "filter_dedup_min_rows") == 0) side = &sk.filter_dedup_min_rows;
    else if (strcmp(name, "idmap_hash_only") == 0) side = &sk.idmap_hash_only;
    else if (strcmp(name, "knn_chunk_rows") == 0) side = &sk.knn_chunk_rows;
    else if (strcmp(name, "knn_query_block") == 0) side = &sk.knn_query_block;
    else if (strcmp(name, "resolve_ids") == 0) side = &sk.resolve_ids;
    else if (strcmp(name, "resolve_blocks") == 0) side = &sk.resolve_blocks;
    else if (strcmp(name, "resolve_set_share") == 0) side = &sk.resolve_set_share;
    else if (strcmp(name, "resolve_peek") == 0) side = &sk.resolve_peek;
    else if (strcmp(name, "resolve_own_first") == 0) side = &sk.resolve_own_first;
    GLX_REQUIRE(side != nullptr, "unknown knob '%s'", name);
    side->store(value, std::memory_order_relaxed);
    return GLX_OK;
  }
  slot->store(value, std::memory_order_relaxed);
  return GLX_OK;
}

extern "C" int glx_features_create(int device, int64_t num_rows, int32_t dim, const float* X,
                                   const int64_t* ids, int ptr_kind, void* stream,
                                   glx_features** out) {
  return glx_features_create_impl(device, num_rows, dim, X, GLX_DTYPE_F32, GLX_DTYPE_F32, ids, ptr_kind, stream, true, out);
}

extern "C" int glx_features_create_ex(int device, int64_t num_rows, int32_t dim, const void* X, int x_dtype,
                                      int store_dtype, const int64_t* ids, int ptr_kind, void* stream,
                                      glx_features** out) {
  return glx_features_create_impl(device, num_rows, dim, X, x_dtype, store_dtype, ids, ptr_kind, stream, true, out);
}

namespace {
bool glx_dtype_known(int dtype) { return glx_dtype_size(dtype) != 0; }
}  // namespace

int glx_features_create_impl(int device, int64_t num_rows, int32_t dim, const void* X, int x_dtype, int store_dtype,
                             const int64_t* ids, int ptr_kind, void* stream, bool allow_arithmetic_ids, glx_features** out) {
  GLX_REQUIRE(out != nullptr, "out is NULL");
  *out = nullptr;
  GLX_REQUIRE(num_rows >= 0 && dim > 0, "bad shape [%lld, %d]", (long long)num_rows, dim);
  GLX_REQUIRE(num_rows < INT32_MAX, "num_rows must be < 2^31");
  GLX_REQUIRE(num_rows == 0 || X != nullptr, "X is NULL");
  GLX_REQUIRE(ptr_kind == GLX_PTR_HOST || ptr_kind == GLX_PTR_DEVICE, "bad ptr_kind");
  GLX_REQUIRE(glx_dtype_known(x_dtype), "unknown x_dtype %d", x_dtype);
  GLX_REQUIRE(glx_dtype_known(store_dtype), "unknown store_dtype %d", store_dtype);
  GLX_REQUIRE(x_dtype == store_dtype || x_dtype == GLX_DTYPE_F32,
              "a %s matrix cannot be stored as %s (only float32 input converts)", glx_dtype_name(x_dtype),
              glx_dtype_name(store_dtype));
  int rc = glx_init_device(device);
  if (rc != GLX_OK) return rc;
  GlxDeviceGuard guard(device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", device);
  hipStream_t s = glx_stream(stream);
  glx_features* f = new (std::nothrow) glx_features();
  GLX_REQUIRE(f != nullptr, "out of host memory");
  memset(static_cast<void*>(f), 0, sizeof(*f));
  f->device = device;
  f->num_rows = num_rows;
  f->dim = dim;
  f->dtype = store_dtype;
  f->elem_size = glx_dtype_size(store_dtype);
  f->owns_x = true;
  // Row pitch.  When a row is a multiple of 256 bytes, rows whose ids share low
  // zero bits (RMAT-style / power-of-two-structured ids are exactly the hub ids)
  // alias onto the same cache sets and HBM channels; one extra 64-byte sector per
  // row breaks the power-of-two stride.  GLX_FEATURE_ROW_PAD overrides (floats).
  // The pad counts FLOATS for every storage type -- the same bytes, 2 pad elements per float of a half table --
  // so a multiple of 4 keeps every row 16-byte aligned whatever the table stores.
  int64_t pad = 0;
  if (const char* env = getenv("GLX_FEATURE_ROW_PAD")) pad = atoll(env);  // experiment knob (floats)
  if (pad < 0 || (pad % 4) != 0) pad = 0;
  f->stride = dim + pad * 4 / f->elem_size;
  f->swizzle_rows = (num_rows >> GLX_SWIZZLE_BITS) << GLX_SWIZZLE_BITS;
  if (const char* env = getenv("GLX_FEATURE_SWIZZLE")) {
    if (atoi(env) == 0) f->swizzle_rows = 0;
  }
  const size_t bytes = (size_t)(num_rows > 0 ? num_rows : 1) * f->stride * f->elem_size;
  hipError_t e = hipMalloc(&f->X, bytes);
  GlxTemp staged;
  if (e == hipSuccess && num_rows > 0) {
    const void* d_src = X;
    const size_t src_bytes = (size_t)num_rows * dim * glx_dtype_size(x_dtype);
    if (ptr_kind == GLX_PTR_HOST) {
      e = hipMalloc(&staged.p, src_bytes);
      if (e == hipSuccess) e = hipMemcpyAsync(staged.p, X, src_bytes, hipMemcpyHostToDevice, s);
      d_src = staged.p;
    }
    if (e == hipSuccess) {
      const int64_t total = num_rows * (int64_t)dim;
      int64_t blocks = (total + 255) / 256;
      if (blocks > 65536) blocks = 65536;
      auto place = glx_place_rows_kernel<GLX_DTYPE_F32, GLX_DTYPE_F32>;
      if (store_dtype == GLX_DTYPE_BF16) {
        place = x_dtype == GLX_DTYPE_F32 ? glx_place_rows_kernel<GLX_DTYPE_F32, GLX_DTYPE_BF16>
                                         : glx_place_rows_kernel<GLX_DTYPE_BF16, GLX_DTYPE_BF16>;
      } else if (store_dtype == GLX_DTYPE_F16) {
        place = x_dtype == GLX_DTYPE_F32 ? glx_place_rows_kernel<GLX_DTYPE_F32, GLX_DTYPE_F16>
                                         : glx_place_rows_kernel<GLX_DTYPE_F16, GLX_DTYPE_F16>;
      } else if (store_dtype == GLX_DTYPE_F8E4M3) {
        place = x_dtype == GLX_DTYPE_F32 ? glx_place_rows_kernel<GLX_DTYPE_F32, GLX_DTYPE_F8E4M3>
                                         : glx_place_rows_kernel<GLX_DTYPE_F8E4M3, GLX_DTYPE_F8E4M3>;
      } else if (store_dtype == GLX_DTYPE_F8E5M2) {
        place = x_dtype == GLX_DTYPE_F32 ? glx_place_rows_kernel<GLX_DTYPE_F32, GLX_DTYPE_F8E5M2>
                                         : glx_place_rows_kernel<GLX_DTYPE_F8E5M2, GLX_DTYPE_F8E5M2>;
      }
      place<<<(unsigned)blocks, 256, 0, s>>>(d_src, num_rows, dim, f->stride, f->swizzle_rows, f->X);
    }
  }
  int64_t* tmp_ids = nullptr;
  if (e == hipSuccess && ids) {
    const int64_t* d_ids = ids;
    if (ptr_kind == GLX_PTR_HOST) {
      e = hipMalloc(&tmp_ids, (size_t)(num_rows > 0 ? num_rows : 1) * sizeof(int64_t));
      if (e == hipSuccess) e = hipMemcpyAsync(tmp_ids, ids, (size_t)num_rows * sizeof(int64_t), hipMemcpyHostToDevice, s);
      d_ids = tmp_ids;
    }
    if (e == hipSuccess) {
      rc = allow_arithmetic_ids ? glx_idmap_build_auto(d_ids, num_rows, &f->idmap, s) : glx_idmap_build(d_ids, num_rows, &f->idmap, s);
    }
  }
  if (e == hipSuccess && rc == GLX_OK && f->idmap.keys != nullptr) {
    // a hash table answers id -> row only: KNN search reports ids, so the rows' ids stay on the device (glx_knn.hip)
    if (tmp_ids) {
      f->knn_row_ids = tmp_ids;
      tmp_ids = nullptr;
    } else {
      e = hipMalloc(&f->knn_row_ids, (size_t)num_rows * sizeof(int64_t));
      if (e == hipSuccess) e = hipMemcpyAsync(f->knn_row_ids, ids, (size_t)num_rows * sizeof(int64_t), hipMemcpyDeviceToDevice, s);
    }
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (tmp_ids) (void)hipFree(tmp_ids);
  if (e != hipSuccess || rc != GLX_OK) {
    if (e != hipSuccess) glx_set_error("feature upload failed: %s", hipGetErrorString(e));
    glx_features_destroy(f);
    return e == hipErrorOutOfMemory ? GLX_RESOURCE_EXHAUSTED : (rc != GLX_OK ? rc : GLX_INTERNAL);
  }
  *out = f;
  return GLX_OK;
}

extern "C" int glx_features_view(int device, int64_t num_rows, int32_t dim, const float* X_device,
                                 glx_features** out) {
  return glx_features_view_ex(device, num_rows, dim, X_device, GLX_DTYPE_F32, out);
}

extern "C" int glx_features_view_ex(int device, int64_t num_rows, int32_t dim, const void* X_device, int dtype,
                                    glx_features** out) {
  GLX_REQUIRE(out != nullptr, "out is NULL");
  *out = nullptr;
  GLX_REQUIRE(num_rows >= 0 && dim > 0, "bad shape [%lld, %d]", (long long)num_rows, dim);
  GLX_REQUIRE(num_rows < INT32_MAX, "num_rows must be < 2^31");
  GLX_REQUIRE(num_rows == 0 || X_device != nullptr, "X is NULL");
  GLX_REQUIRE(glx_dtype_known(dtype), "unknown dtype %d", dtype);
  int rc = glx_init_device(device);
  if (rc != GLX_OK) return rc;
  glx_features* f = new (std::nothrow) glx_features();
  GLX_REQUIRE(f != nullptr, "out of host memory");
  memset(static_cast<void*>(f), 0, sizeof(*f));
  f->device = device;
  f->num_rows = num_rows;
  f->dim = dim;
  f->stride = dim;
  f->swizzle_rows = 0;  // a view addresses the caller's rows as they are
  f->X = const_cast<void*>(X_device);
  f->dtype = dtype;
  f->elem_size = glx_dtype_size(dtype);
  f->owns_x = false;
  *out = f;
  return GLX_OK;
}

extern "C" void glx_features_destroy(glx_features* f) {
  if (!f) return;
  GlxDeviceGuard guard(f->device);
  if (f->X && f->owns_x) (void)hipFree(f->X);
  if (f->knn_row_ids) (void)hipFree(f->knn_row_ids);
  if (f->knn_xn) (void)hipFree(f->knn_xn);
  if (f->knn_xn_ready) (void)hipEventDestroy(static_cast<hipEvent_t>(f->knn_xn_ready));
  glx_idmap_free(&f->idmap);
  delete f;
}

extern "C" int glx_features_info(const glx_features* f, int64_t* num_rows, int32_t* dim,
                                 int* has_id_map, int* device) {
  GLX_REQUIRE(f != nullptr, "features is NULL");
  if (num_rows) *num_rows = f->num_rows;
  if (dim) *dim = f->dim;
  if (has_id_map) *has_id_map = f->idmap.any();
  if (device) *device = f->device;
  return GLX_OK;
}

extern "C" int glx_features_dtype(const glx_features* f, int* dtype) {
  GLX_REQUIRE(f != nullptr, "features is NULL");
  GLX_REQUIRE(dtype != nullptr, "dtype is NULL");
  *dtype = f->dtype;
  return GLX_OK;
}

extern "C" int glx_features_convert_host(const float* src, int64_t n, int store_dtype, void* dst) {
  GLX_REQUIRE(n >= 0, "negative n");
  GLX_REQUIRE(glx_dtype_known(store_dtype), "unknown store_dtype %d", store_dtype);
  if (n == 0) return GLX_OK;
  GLX_REQUIRE(src && dst, "NULL data pointer");
  if (store_dtype == GLX_DTYPE_F32) {
    memcpy(dst, src, (size_t)n * sizeof(float));
    return GLX_OK;
  }
  for (int64_t i = 0; i < n; ++i) {
    uint32_t u;
    memcpy(&u, src + i, sizeof(u));
    if (store_dtype == GLX_DTYPE_BF16) static_cast<uint16_t*>(dst)[i] = glx_f32_to_bf16_bits(u);
    else if (store_dtype == GLX_DTYPE_F16) static_cast<uint16_t*>(dst)[i] = glx_f32_to_f16_bits(u);
    else if (store_dtype == GLX_DTYPE_F8E4M3) static_cast<uint8_t*>(dst)[i] = glx_f32_to_f8e4m3_bits(u);
    else static_cast<uint8_t*>(dst)[i] = glx_f32_to_f8e5m2_bits(u);
  }
  return GLX_OK;
}

extern "C" int glx_aggregate(const glx_features* f, int op, const int64_t* node_ids,
                             const int32_t* segment_ids, int32_t num_ids, int32_t num_segments,
                             float default_attr, float* emb_out, int32_t* cnt_out, int ptr_kind,
                             void* stream) {
  GLX_REQUIRE(f != nullptr, "features is NULL");
  GLX_REQUIRE(op >= GLX_AGG_SUM && op <= GLX_AGG_PROD, "unknown aggregator id %d", op);
  GLX_REQUIRE(num_ids >= 0 && num_segments >= 0, "negative sizes");
  GLX_REQUIRE(ptr_kind == GLX_PTR_HOST || ptr_kind == GLX_PTR_DEVICE, "bad ptr_kind");
  GLX_REQUIRE((int64_t)num_segments * f->dim <= INT32_MAX,
              "num_segments * dim exceeds int32 (tensor.h:47)");
  if (num_segments == 0) return GLX_OK;
  GLX_REQUIRE(emb_out && cnt_out && (num_ids == 0 || node_ids), "NULL data pointer");
  GLX_REQUIRE(segment_ids != nullptr || num_ids % num_segments == 0,
              "segment_ids == NULL means equal segments: num_ids must be a multiple of num_segments");
  GlxDeviceGuard guard(f->device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", f->device);
  // outputs go straight into the caller's buffers when those are pinned: the embeddings are by far the largest part
  // of a response (4 * dim bytes per segment)
  GlxHostStage st(f->device, ptr_kind, stream, GlxHostStage::ADMIT | GlxHostStage::DIRECT_PINNED);
  const int64_t* d_ids;
  const int32_t* d_seg;
  float* d_emb;
  int32_t* d_cnt;
  st.in(&d_ids, node_ids, (size_t)num_ids);
  st.in(&d_seg, segment_ids, (size_t)num_ids);
  st.out(&d_emb, emb_out, (size_t)num_segments * f->dim);
  st.out(&d_cnt, cnt_out, (size_t)num_segments);
  int rc = st.begin();
  if (rc == GLX_OK) rc = aggregate_device(f, op, d_ids, d_seg, num_ids, num_segments, default_attr, d_emb, d_cnt, st.s);
  return st.finish(rc);
}

extern "C" int glx_lookup(const glx_features* f, const int64_t* node_ids, int64_t n,
                          float default_attr, float* out, int ptr_kind, void* stream) {
  GLX_REQUIRE(f != nullptr, "features is NULL");
  GLX_REQUIRE(n >= 0, "negative n");
  GLX_REQUIRE(ptr_kind == GLX_PTR_HOST || ptr_kind == GLX_PTR_DEVICE, "bad ptr_kind");
  if (n == 0) return GLX_OK;
  GLX_REQUIRE(node_ids && out, "NULL data pointer");
  GlxDeviceGuard guard(f->device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", f->device);
  int G = 1;
  const int want = (f->dim & 3) == 0 ? f->dim / 4 : f->dim;
  while (G < 64 && G < want) G <<= 1;
  const int64_t threads = n * G;
  // a pinned caller buffer is written by the kernel directly
  GlxHostStage st(f->device, ptr_kind, stream, GlxHostStage::ADMIT | GlxHostStage::DIRECT_PINNED);
  const int64_t* d_ids;
  float* d_out;
  st.in(&d_ids, node_ids, (size_t)n);
  st.out(&d_out, out, (size_t)n * f->dim);
  int rc = st.begin();
  if (rc == GLX_OK) {
    GlxKernelTimer timer(GLX_KERNEL_LOOKUP, st.s);
    const unsigned grid = (unsigned)((threads + 255) / 256);
    auto lookup = glx_lookup_kernel<GLX_DTYPE_F32>;
    if (f->dtype == GLX_DTYPE_BF16) lookup = glx_lookup_kernel<GLX_DTYPE_BF16>;
    else if (f->dtype == GLX_DTYPE_F16) lookup = glx_lookup_kernel<GLX_DTYPE_F16>;
    else if (f->dtype == GLX_DTYPE_F8E4M3) lookup = glx_lookup_kernel<GLX_DTYPE_F8E4M3>;
    else if (f->dtype == GLX_DTYPE_F8E5M2) lookup = glx_lookup_kernel<GLX_DTYPE_F8E5M2>;
    lookup<<<grid, 256, 0, st.s>>>(f->map(), f->X, f->stride, f->swizzle_rows, f->dim, d_ids, n, default_attr, d_out, G);
    timer.stop();
  }
  return st.finish(rc);
}

extern "C" int glx_aggregate_stitch(int device, int op, int32_t num_parts, const float* parts,
                                    const int32_t* cnts, int32_t num_segments, int32_t dim,
                                    float default_attr, float* emb_out, int32_t* cnt_out, void* stream) {
  GLX_REQUIRE(op >= GLX_AGG_SUM && op <= GLX_AGG_PROD, "unknown aggregator %d", op);
  GLX_REQUIRE(num_parts >= 1 && num_segments >= 0 && dim >= 1, "bad sizes");
  if (num_segments == 0) return GLX_OK;
  GLX_REQUIRE(parts && cnts && emb_out && cnt_out, "NULL data pointer");
  int rc = glx_init_device(device);
  if (rc != GLX_OK) return rc;
  GlxDeviceGuard guard(device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", device);
  hipStream_t s = glx_stream(stream);
  const bool vec4 = dim % 4 == 0 && ((uintptr_t)parts % 16 == 0) && ((uintptr_t)emb_out % 16 == 0);
  switch (op) {
    case GLX_AGG_SUM: launch_agg_stitch<GLX_AGG_SUM>(vec4, parts, cnts, num_parts, num_segments, dim, default_attr, emb_out, cnt_out, s); break;
    case GLX_AGG_MEAN: launch_agg_stitch<GLX_AGG_MEAN>(vec4, parts, cnts, num_parts, num_segments, dim, default_attr, emb_out, cnt_out, s); break;
    case GLX_AGG_MAX: launch_agg_stitch<GLX_AGG_MAX>(vec4, parts, cnts, num_parts, num_segments, dim, default_attr, emb_out, cnt_out, s); break;
    case GLX_AGG_MIN: launch_agg_stitch<GLX_AGG_MIN>(vec4, parts, cnts, num_parts, num_segments, dim, default_attr, emb_out, cnt_out, s); break;
    default: launch_agg_stitch<GLX_AGG_PROD>(vec4, parts, cnts, num_parts, num_segments, dim, default_attr, emb_out, cnt_out, s); break;
  }
  GLX_HIP(hipGetLastError());
  return GLX_OK;
}
