// glx frontier dedup: the distinct ids of a multi-part id stream in first-occurrence order, the position of every
// stream element in that list, and the number of distinct ids after each part.  Stands in for what the reference does
// on the host or with sort-based torch calls: graphlearn/examples/pytorch/tgn/temporal_batch_loader.py:99-121
// (torch.cat(...).unique() + an `assoc` array as long as the node type) and SubGraphSampler's node set
// (core/operator/subgraph/subgraph_sampler.h:47-72).
//
// No sort.  An open-addressing table of 32-bit stream POSITIONS (n <= 2^31 - 1): a slot's id is x[slot's position], so
// every int64 value -- INT64_MIN, the empty key of the id -> row maps, included -- is an ordinary id and the table is
// 4 bytes per slot.  Passes, all on the caller's stream:
//   clear    every slot = kEmpty                                             (memset, 4 B per slot)
//   insert   position i claims the first empty slot of its probe sequence (compare-and-swap), or finds the slot whose
//            id equals its own and lowers that slot to min(slot, i).  A slot's id never changes once set, and its
//            position only falls: after the pass slot = the SMALLEST position of its id, whatever order the atomics
//            resolved in.  slot_of[i] remembers where i ended up (which slot that is may differ between runs).
//   flag     first[i] = (table[slot_of[i]] == i), one bit per id, and the number of set bits per tile
//   scan     exclusive scan of the tile counts (one workgroup)
//   scatter  rank of i = tile offset + set bits before i: nodes[rank] = x[i] for first occurrences, which also leave
//            their rank (tagged with bit 31) in their slot; the last position of every part writes part_end
//   inverse  inverse[i] = rank left in table[slot_of[i]]
// Every output is a function of the flags, and the flags of the input alone.
#include "glx_lane_groups.h"

namespace {

constexpr int kMaxParts = 16;
constexpr uint32_t kEmpty = 0xffffffffu;  // no position: positions are < 2^31 - 1, tagged ranks < 0xffffffff
constexpr uint32_t kRankTag = 0x80000000u;
constexpr int kTile = 2048;      // ids per workgroup of the flag / scatter passes ...
constexpr int kTileSmall = 512;  // ... and for streams up to kSmallIds (glx_partition.hip: a short stream on few
constexpr int64_t kSmallIds = 1 << 18;  // workgroups is a chain of dependent round trips)

// The concatenated stream: x[q] = *(int64_t*)(adj[p] + 8 * q) for the last part p with begin[p] <= q, where
// adj[p] = (address of part p) - 8 * begin[p].  Empty parts never win: a later part with the same begin overrides them,
// and trailing ones begin at n.
struct UniqueParts {
  uint64_t adj[kMaxParts];
  uint32_t begin[kMaxParts + 1];  // begin[num] = n
  int32_t num;
};

__device__ __forceinline__ int64_t stream_at(const UniqueParts& x, uint32_t q) {
  uint64_t a = x.adj[0];
  for (int p = 1; p < x.num; ++p) {
    if (q >= x.begin[p]) a = x.adj[p];
  }
  return *reinterpret_cast<const int64_t*>(a + 8ull * q);
}

__global__ __launch_bounds__(256) void glx_unique_insert_kernel(UniqueParts x, uint32_t n, uint32_t* table,
                                                                uint32_t mask, uint32_t* __restrict__ slot_of) {
  const int lane = threadIdx.x & 63;
  const int64_t i64 = blockIdx.x * (int64_t)256 + threadIdx.x;
  const bool active = i64 < (int64_t)n;
  const uint32_t i = (uint32_t)i64;
  const int64_t id = active ? stream_at(x, i) : 0;
  uint32_t h = (uint32_t)glx_mix64((uint64_t)id) & mask;
  bool done = !active;
  while (__any(!done)) {  // wave-uniform: the ballots below need every lane
    // A slot that holds a position keeps its id for good, so a plain load that returns one is final as far as the id
    // goes (the position may since have fallen); "empty" may be stale (another XCD's L2) and only then is the
    // compare-and-swap paid (glx_dist.hip, resolve).
    uint32_t cur = kEmpty;
    if (!done) cur = *reinterpret_cast<const volatile uint32_t*>(&table[h]);
    // claim: every lane that read "empty" tries its own slot in ONE vector compare-and-swap (distinct slots do not wait
    // for each other).  Lanes that share the slot of the first such lane -- the hub id of a skewed stream, every lane
    // of an all-equal one -- stand back and take that lane's outcome: it holds the group's smallest position.
    const bool pend = !done && cur == kEmpty;
    const uint64_t pending = __ballot(pend);
    if (pending) {
      const int leader = __ffsll((long long)pending) - 1;
      const uint32_t hl = (uint32_t)__shfl((int)h, leader);  // (every shuffle outside the branches: all lanes take part)
      const bool follower = pend && lane != leader && h == hl;
      uint32_t got = kEmpty;
      if (pend && !follower) got = atomicCAS(&table[h], kEmpty, i);
      const uint32_t gl = (uint32_t)__shfl((int)got, leader);
      const uint32_t li = (uint32_t)__shfl((int)i, leader);
      if (follower) {
        cur = gl == kEmpty ? li : gl;  // the slot holds the leader's id now, or whoever beat it
      } else if (pend) {
        if (got == kEmpty) done = true;
        else cur = got;
      }
    }
    const bool match = !done && stream_at(x, cur) == id;
    // lower: cur >= the slot's value now, so i > cur needs nothing; otherwise one atomicMin per (wave, slot)
    uint64_t lower = __ballot(match && i < cur);
    while (lower) {
      const int leader = __ffsll((long long)lower) - 1;
      const uint32_t hl = (uint32_t)__shfl((int)h, leader);
      const uint64_t same = __ballot(match && i < cur && h == hl);
      if (lane == leader) atomicMin(&table[h], i);
      lower &= ~same;
    }
    if (match) {
      done = true;
    } else if (!done) {
      h = (h + 1) & mask;
    }
  }
  if (active) slot_of[i] = h;
}

// first[w] bit l: position 64 w + l is the smallest position of its id.  tile_count[b]: set bits of tile b.
__global__ __launch_bounds__(256) void glx_unique_flag_kernel(uint32_t n, int32_t tile, const uint32_t* __restrict__ table,
                                                              const uint32_t* __restrict__ slot_of,
                                                              uint64_t* __restrict__ first, uint32_t* __restrict__ tile_count) {
  __shared__ uint32_t wave_cnt[4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t base = blockIdx.x * (int64_t)tile;
  uint32_t cnt = 0;
  for (int it = 0; it < tile / 256; ++it) {
    const int64_t i = base + it * 256 + threadIdx.x;
    if (base + it * 256 + wid * 64 >= (int64_t)n) break;  // wave-uniform
    const bool is_first = i < (int64_t)n && table[slot_of[i]] == (uint32_t)i;
    const uint64_t b = __ballot(is_first);
    if (lane == 0) first[i >> 6] = b;
    cnt += (uint32_t)__popcll(b);
  }
  if (lane == 0) wave_cnt[wid] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) tile_count[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// In-place exclusive scan of tile_count[ntiles] (single workgroup; the total stays below 2^31).
__global__ __launch_bounds__(1024) void glx_unique_scan_kernel(uint32_t* __restrict__ tile_count, int64_t ntiles) {
  __shared__ uint32_t wave_sum[16];
  __shared__ uint32_t carry_s;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (int64_t base = 0; base < ntiles; base += 1024) {
    const int64_t i = base + threadIdx.x;
    const uint32_t v = i < ntiles ? tile_count[i] : 0;
    uint32_t s = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t y = (uint32_t)__shfl_up((int)s, off);
      if (lane >= off) s += y;
    }
    if (lane == 63) wave_sum[wid] = s;
    __syncthreads();
    uint32_t woff = 0;
    for (int w = 0; w < wid; ++w) woff += wave_sum[w];
    const uint32_t carry = carry_s;
    if (i < ntiles) tile_count[i] = carry + woff + s - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry_s = carry + woff + s;
    __syncthreads();
  }
}

// part_end[p] = distinct ids in parts 0 .. p: the inclusive rank of the part's last position, 0 for parts that end at 0.
__global__ __launch_bounds__(256) void glx_unique_scatter_kernel(UniqueParts x, uint32_t n, int32_t tile,
                                                                 const uint64_t* __restrict__ first,
                                                                 const uint32_t* __restrict__ tile_off,
                                                                 const uint32_t* __restrict__ slot_of,
                                                                 uint32_t* __restrict__ table, bool leave_rank,
                                                                 int64_t* __restrict__ nodes, int64_t* __restrict__ part_end) {
  __shared__ uint32_t word_off[kTile / 64 + 1];  // set bits of this tile before each of its words
  const int lane = threadIdx.x & 63;
  const int64_t base = blockIdx.x * (int64_t)tile;
  const int words = tile / 64;
  if (threadIdx.x < 64) {  // one wave: popcount of every word, scanned
    const int64_t w = (base >> 6) + lane;
    uint32_t c = (lane < words && w * 64 < (int64_t)n) ? (uint32_t)__popcll(first[w]) : 0;
    uint32_t s = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t y = (uint32_t)__shfl_up((int)s, off);
      if (lane >= off) s += y;
    }
    if (lane < words) word_off[lane] = s - c;
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < x.num && x.begin[threadIdx.x + 1] == 0) part_end[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t off = tile_off[blockIdx.x];
  for (int it = 0; it < tile / 256; ++it) {
    const int64_t i = base + it * 256 + threadIdx.x;
    if (i >= (int64_t)n) break;
    const uint64_t b = first[i >> 6];
    const uint32_t rank = off + word_off[(it * 256 + (int)threadIdx.x) >> 6] + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    const bool is_first = (b >> lane) & 1ull;
    if (is_first) {
      nodes[rank] = stream_at(x, (uint32_t)i);
      if (leave_rank) table[slot_of[i]] = rank | kRankTag;
    }
    // does a part end in this group of 256 positions?  (uniform test per part; the one lane on that position writes)
    const int64_t group = base + it * 256;
    for (int p = 0; p < x.num; ++p) {
      const int64_t last = (int64_t)x.begin[p + 1] - 1;
      if (last >= group && last < group + 256 && last == i) part_end[p] = (int64_t)rank + (is_first ? 1 : 0);
    }
  }
}

__global__ __launch_bounds__(256) void glx_unique_inverse_kernel(uint32_t n, const uint32_t* __restrict__ table,
                                                                 const uint32_t* __restrict__ slot_of,
                                                                 int64_t* __restrict__ inverse) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i < (int64_t)n) inverse[i] = (int64_t)(table[slot_of[i]] & ~kRankTag);
}


// Device pointers only; device selected.  n >= 1.
int unique_device(const UniqueParts& x, uint32_t n, int64_t* nodes, int64_t* inverse, int64_t* part_end, hipStream_t s) {
  // Slots: the power of two from 1.5 n up (load <= 2/3 when every id is distinct; linear probing then averages
  // ~2.5 probes for an absent id, ~1.5 for a present one).  The distinct count is not known before the pass.
  uint64_t cap = 1024;
  while (cap < (uint64_t)n + n / 2) cap <<= 1;
  const int32_t tile = (int64_t)n <= kSmallIds ? kTileSmall : kTile;
  const int64_t ntiles = ((int64_t)n + tile - 1) / tile;
  const size_t table_b = glx_align256(cap * sizeof(uint32_t));
  const size_t slot_b = glx_align256((size_t)n * sizeof(uint32_t));
  const size_t first_b = glx_align256((size_t)(((int64_t)n + 63) / 64) * sizeof(uint64_t));
  const size_t tiles_b = glx_align256((size_t)ntiles * sizeof(uint32_t));
  GlxScratch lease;
  int rc = lease.alloc(table_b + slot_b + first_b + tiles_b, s, 1);
  if (rc != GLX_OK) return rc;
  char* at = lease.as<char>();
  uint32_t* table = reinterpret_cast<uint32_t*>(at);
  uint32_t* slot_of = reinterpret_cast<uint32_t*>(at + table_b);
  uint64_t* first = reinterpret_cast<uint64_t*>(at + table_b + slot_b);
  uint32_t* tile_count = reinterpret_cast<uint32_t*>(at + table_b + slot_b + first_b);
  GLX_HIP(hipMemsetAsync(table, 0xff, cap * sizeof(uint32_t), s));
  const unsigned per_id = (unsigned)(((int64_t)n + 255) / 256);
  glx_unique_insert_kernel<<<per_id, 256, 0, s>>>(x, n, table, (uint32_t)(cap - 1), slot_of);
  glx_unique_flag_kernel<<<(unsigned)ntiles, 256, 0, s>>>(n, tile, table, slot_of, first, tile_count);
  glx_unique_scan_kernel<<<1, 1024, 0, s>>>(tile_count, ntiles);
  glx_unique_scatter_kernel<<<(unsigned)ntiles, 256, 0, s>>>(x, n, tile, first, tile_count, slot_of, table,
                                                            inverse != nullptr, nodes, part_end);
  if (inverse != nullptr) glx_unique_inverse_kernel<<<per_id, 256, 0, s>>>(n, table, slot_of, inverse);
  GLX_HIP(hipGetLastError());
  return GLX_OK;
}

}  // namespace

extern "C" int glx_unique(int device, const int64_t* const* parts, const int64_t* part_len, int32_t num_parts,
                          int64_t* nodes_out, int64_t* inverse_out, int64_t* part_end_out, int ptr_kind, void* stream) {
  GLX_REQUIRE(num_parts >= 1 && num_parts <= kMaxParts, "num_parts must be in [1, %d]", kMaxParts);
  GLX_REQUIRE(parts != nullptr && part_len != nullptr && part_end_out != nullptr, "NULL data pointer");
  GLX_REQUIRE(ptr_kind == GLX_PTR_HOST || ptr_kind == GLX_PTR_DEVICE, "bad ptr_kind");
  int64_t n = 0;
  for (int32_t p = 0; p < num_parts; ++p) {
    GLX_REQUIRE(part_len[p] >= 0, "negative length of part %d", p);
    GLX_REQUIRE(part_len[p] <= (int64_t)INT32_MAX - n, "glx_unique takes at most 2^31 - 1 = %d ids in one call", INT32_MAX);
    n += part_len[p];
  }
  for (int32_t p = 0; p < num_parts; ++p) GLX_REQUIRE(part_len[p] == 0 || parts[p] != nullptr, "NULL data pointer (part %d)", p);
  GLX_REQUIRE(n == 0 || nodes_out != nullptr, "NULL data pointer");
  int rc = glx_init_device(device);
  if (rc != GLX_OK) return rc;
  GlxDeviceGuard guard(device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", device);
  GlxHostStage st(device, ptr_kind, stream, GlxHostStage::ADMIT);
  const int64_t* d_part[kMaxParts];
  int64_t *d_nodes = nodes_out, *d_inverse = inverse_out, *d_end;
  for (int32_t p = 0; p < num_parts; ++p) st.in(&d_part[p], parts[p], (size_t)part_len[p]);
  if (st.host) {  // only the m distinct ids go back (out_after below); inverse stays absent when the caller wants none
    st.scratch(&d_nodes, (size_t)n);
    if (inverse_out != nullptr) st.out(&d_inverse, inverse_out, (size_t)n);
  }
  st.out(&d_end, part_end_out, (size_t)num_parts);
  rc = st.begin();
  if (rc == GLX_OK && n == 0) {
    hipError_t e = hipMemsetAsync(d_end, 0, (size_t)num_parts * sizeof(int64_t), st.s);
    if (e != hipSuccess) {
      glx_set_error("hipMemsetAsync failed: %s", hipGetErrorString(e));
      rc = GLX_INTERNAL;
    }
  } else if (rc == GLX_OK) {
    UniqueParts x;
    x.num = num_parts;
    uint32_t begin = 0;
    for (int32_t p = 0; p < kMaxParts; ++p) {  // unused entries: empty parts at the end
      x.begin[p] = begin;
      x.adj[p] = p < num_parts ? (uint64_t)reinterpret_cast<uintptr_t>(d_part[p]) - 8ull * begin : 0;
      if (p < num_parts) begin += (uint32_t)part_len[p];
    }
    x.begin[kMaxParts] = begin;
    rc = unique_device(x, (uint32_t)n, d_nodes, d_inverse, d_end, st.s);
    if (rc == GLX_OK && st.host) {  // host-pointer calls are synchronous: read m, then copy that many ids back
      int64_t m = 0;
      hipError_t e = hipMemcpyAsync(&m, d_end + (num_parts - 1), sizeof(m), hipMemcpyDeviceToHost, st.s);
      if (e == hipSuccess) e = hipStreamSynchronize(st.s);
      if (e != hipSuccess) {
        glx_set_error("glx_unique: reading the distinct count failed: %s", hipGetErrorString(e));
        rc = GLX_INTERNAL;
      } else {
        st.out_after(nodes_out, d_nodes, (size_t)m * sizeof(int64_t));
      }
    }
  }
  return st.finish(rc);
}
