// glx TGN memory: the device-resident message store, the fused message of a node and the memory write of
// torch_geometric's TGNMemory as the reference's TGN example uses it (examples/pytorch/tgn/train_and_eval.py:27-31 and
// :70-78 -- IdentityMessage + LastAggregator --, used at :118 and :130).
//
// Contract (DESIGN.md 4, K-tgn-mem; include/glx.h).  With the Last aggregator and a message function without
// parameters the only stored message of a node that is ever used is its latest event over both roles, so the store is
// ONE pending slot per node in caller-owned buffers: pend_t / pend_seq / pend_other [N] int64, pend_raw [N, R] float32,
// next to memory [N, M] float32 and last_update [N] int64.  The slot of node v holds the event with the largest
// (t, seq) among all events that ever named v as src or dst; seq = seq_base + (position in its update call).
//   glx_tgn_store_update      three launches over the 2B (event, end point) candidates, each a function of the finished
//                             state of the one before, so no result depends on a scheduling order:
//                               maxt    pend_t[v]   = max(pend_t[v], t[p])                      (64-bit signed atomic max)
//                               maxseq  pend_seq[v] = max(pend_seq[v], seq_base + p) for the candidates with
//                                       t[p] == pend_t[v]: every older slot has seq < seq_base, so a slot whose t was
//                                       neither beaten nor equalled stays whole
//                               write   the candidates with t[p] == pend_t[v] and seq_base + p == pend_seq[v] write
//                                       pend_other[v] and copy their raw row, one lane group each (a self loop's two
//                                       candidates write the same words)
//   glx_tgn_message           one lane group per entry: [memory[v] | memory[other] | raw | cos(w dt + b)], bit-exact
//                             copies and the accurate cosf
//   glx_tgn_message_backward  the gradient of the time encoder's w and b through a fixed reduction tree
//   glx_tgn_memory_write      one lane group per entry: rows and last_update in place
// Nothing is allocated, cleared or launched in proportion to N.  No float atomics anywhere.
#include "glx_lane_groups.h"

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool tgn_in(int64_t v, int64_t num_nodes) { return v >= 0 && v < num_nodes; }

// ---- the store ---------------------------------------------------------------------------------------------
struct StoreArgs {
  const int64_t* src;    // [B]
  const int64_t* dst;    // [B]
  const int64_t* t;      // [B]
  const float* raw;      // [B, R]
  int64_t* pend_t;       // [N]
  int64_t* pend_seq;     // [N]
  int64_t* pend_other;   // [N]
  float* pend_raw;       // [N, R]
  int64_t num_nodes, seq_base;
  int32_t batch, raw_dim;
};

// Candidate c of 2B: event p = c mod B in role c / B (0: the src end point, 1: the dst end point), so the lanes of a
// wave hold consecutive events in one role and a hub's candidates share a wave.
__device__ __forceinline__ int64_t tgn_end_point(const StoreArgs& a, int64_t c, int32_t* p_out, int64_t* other_out) {
  const int32_t role = c >= a.batch;
  const int32_t p = (int32_t)(c - (role ? a.batch : 0));
  const int64_t s = a.src[p], d = a.dst[p];
  *p_out = p;
  *other_out = role ? s : d;
  return role ? d : s;
}

constexpr int kAgreeRounds = 4;  // addresses per wave whose lanes are folded into one atomic

// word[v] = max(word[v], val) for the lanes with `want`, at most one atomic per (wave, address) for the first
// kAgreeRounds addresses the wave's lanes name (a hub that is an end point of every event is the first), one per lane
// for what is left.  Every lane of the wave calls it.
__device__ __forceinline__ void tgn_wave_max(int64_t* word, int64_t v, int64_t val, bool want) {
  const int lane = threadIdx.x & 63;
  for (int round = 0; round < kAgreeRounds; ++round) {
    const uint64_t pending = __ballot(want);
    if (!pending) return;  // wave-uniform
    const int leader = __ffsll((long long)pending) - 1;
    const int64_t vl = __shfl(v, leader);
    const bool mine = want && v == vl;
    int64_t m = mine ? val : INT64_MIN;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const int64_t o = __shfl_xor(m, off);
      m = o > m ? o : m;
    }
    if (lane == leader) __hip_atomic_fetch_max(word + v, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (mine) want = false;
  }
  if (want) __hip_atomic_fetch_max(word + v, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A word only rises, so a plain load that already shows a value >= ours settles the candidate without an atomic (a
// stale, lower value only costs the atomic).
__global__ __launch_bounds__(256) void glx_tgn_maxt_kernel(StoreArgs a) {
  const int64_t c = blockIdx.x * (int64_t)256 + threadIdx.x;
  bool want = false;
  int64_t v = 0, tp = 0;
  if (c < 2 * (int64_t)a.batch) {
    int32_t p;
    int64_t other;
    v = tgn_end_point(a, c, &p, &other);
    if (tgn_in(v, a.num_nodes)) {
      tp = a.t[p];
      want = tp > *reinterpret_cast<const volatile int64_t*>(a.pend_t + v);
    }
  }
  tgn_wave_max(a.pend_t, v, tp, want);
}

__global__ __launch_bounds__(256) void glx_tgn_maxseq_kernel(StoreArgs a) {
  const int64_t c = blockIdx.x * (int64_t)256 + threadIdx.x;
  bool want = false;
  int64_t v = 0, seq = 0;
  if (c < 2 * (int64_t)a.batch) {
    int32_t p;
    int64_t other;
    v = tgn_end_point(a, c, &p, &other);
    if (tgn_in(v, a.num_nodes) && a.t[p] == a.pend_t[v]) {
      seq = a.seq_base + p;
      want = seq > *reinterpret_cast<const volatile int64_t*>(a.pend_seq + v);
    }
  }
  tgn_wave_max(a.pend_seq, v, seq, want);
}

// len 32-bit words from src (zeros when src is null) to dst by the G lanes of a group (lane c): 16 bytes at a time
// where both addresses allow it, one word at a time for the rest -- the whole piece when they do not.  Bit copies.
template <int G>
__device__ __forceinline__ void tgn_put(float* dst_f, const float* src_f, int32_t len, int c) {
  uint32_t* const dst = reinterpret_cast<uint32_t*>(dst_f);
  const uint32_t* const src = reinterpret_cast<const uint32_t*>(src_f);
  const bool v4 = ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15) == 0;
  const int32_t n4 = v4 ? len >> 2 : 0;
  for (int32_t k = c; k < n4; k += G) {
    u32x4 x = {0u, 0u, 0u, 0u};
    if (src) x = *reinterpret_cast<const u32x4*>(src + 4 * k);
    *reinterpret_cast<u32x4*>(dst + 4 * k) = x;
  }
  for (int32_t k = 4 * n4 + c; k < len; k += G) dst[k] = src ? src[k] : 0u;
}

// G lanes own candidate c; only the winner of a slot goes on.
template <int G>
__global__ __launch_bounds__(256) void glx_tgn_store_write_kernel(StoreArgs a) {
  const int64_t c = blockIdx.x * (int64_t)(256 / G) + threadIdx.x / G;
  const int l = threadIdx.x & (G - 1);
  if (c >= 2 * (int64_t)a.batch) return;  // whole groups leave
  int32_t p;
  int64_t other;
  const int64_t v = tgn_end_point(a, c, &p, &other);
  if (!tgn_in(v, a.num_nodes)) return;
  if (a.t[p] != a.pend_t[v] || a.seq_base + p != a.pend_seq[v]) return;
  if (l == 0) a.pend_other[v] = other;
  tgn_put<G>(a.pend_raw + v * (int64_t)a.raw_dim, a.raw + p * (int64_t)a.raw_dim, a.raw_dim, l);
}

// ---- the message -------------------------------------------------------------------------------------------
struct MsgArgs {
  const float* memory;         // [N, M]
  const int64_t* last_update;  // [N]
  const int64_t* pend_t;
  const int64_t* pend_seq;
  const int64_t* pend_other;
  const float* pend_raw;       // [N, R]
  const float* time_w;         // [T]
  const float* time_b;         // [T]
  const int64_t* n_id;         // [n]
  float* msg;                  // [n, 2M + R + T]
  float* h;                    // [n, M]
  float* dt;                   // [n]
  int64_t* t_out;              // [n]
  int32_t* has;                // [n]
  int64_t num_nodes;
  int32_t M, R, T, n;
};

template <int G>
__global__ __launch_bounds__(256) void glx_tgn_message_kernel(MsgArgs a) {
  const int64_t i = blockIdx.x * (int64_t)(256 / G) + threadIdx.x / G;
  const int c = threadIdx.x & (G - 1);
  if (i >= a.n) return;  // whole groups leave
  const int64_t v = a.n_id[i];
  const bool in = tgn_in(v, a.num_nodes);
  const float* const mem_v = in ? a.memory + v * (int64_t)a.M : nullptr;
  const int64_t width = 2 * (int64_t)a.M + a.R + a.T;
  float* const row = a.msg + i * width;
  tgn_put<G>(a.h + i * (int64_t)a.M, mem_v, a.M, c);
  const bool has = in && a.pend_seq[v] >= 0;
  if (!has) {
    if (c == 0) {
      a.has[i] = 0;
      a.t_out[i] = in ? a.last_update[v] : 0;
      a.dt[i] = 0.0f;
    }
    tgn_put<G>(row, nullptr, (int32_t)width, c);
    return;
  }
  const int64_t tv = a.pend_t[v];
  // the difference of two int64 wraps instead of overflowing; one conversion, round to nearest
  const float dt = __ll2float_rn((long long)((uint64_t)tv - (uint64_t)a.last_update[v]));
  if (c == 0) {
    a.has[i] = 1;
    a.t_out[i] = tv;
    a.dt[i] = dt;
  }
  const int64_t o = a.pend_other[v];
  tgn_put<G>(row, mem_v, a.M, c);
  tgn_put<G>(row + a.M, tgn_in(o, a.num_nodes) ? a.memory + o * (int64_t)a.M : nullptr, a.M, c);
  tgn_put<G>(row + 2 * a.M, a.pend_raw + v * (int64_t)a.R, a.R, c);
  float* const enc = row + 2 * a.M + a.R;
  for (int32_t j = c; j < a.T; j += G) enc[j] = cosf(fmaf(a.time_w[j], dt, a.time_b[j]));
}

// ---- the gradient of the time encoder ----------------------------------------------------------------------
// The tree, fixed by (n, T) alone (GLX_TGN_BWD_DEPTH in include/glx.h counts its longest path):
//   rows     chunk k is rows [kRows k, kRows k + kRows); wave w of its workgroup folds rows w, w + 4, .. of the chunk
//            in ascending order, lane l column 64 blockIdx.y + l: acc = acc + term from +0.0f, at most kRows / 4 adds
//   waves    (wave 0 + wave 1) + (wave 2 + wave 3) through shared memory: 2 adds
//   chunks   one wave per (w | b, column): lane l folds the partials of chunks l, l + 64, .. ascending from +0.0f,
//            ceil(chunks / 64) adds, then the xor tree over the 64 lanes: 6 adds
constexpr int kRows = GLX_TGN_BWD_ROWS;

struct BwdArgs {
  const float* g;     // [n, width]
  const float* dt;    // [n]
  const int32_t* has; // [n]
  const float* time_w;
  const float* time_b;
  float* partial;     // [chunks, 2, T]
  float* grad_w;      // [T]
  float* grad_b;      // [T]
  int32_t n, width, time_off, T, chunks;
};

__global__ __launch_bounds__(256) void glx_tgn_bwd_rows_kernel(BwdArgs a) {
  __shared__ float part[2][4][64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int32_t j = blockIdx.y * 64 + lane;
  const bool col_ok = j < a.T;
  const float w = col_ok ? a.time_w[j] : 0.0f, b = col_ok ? a.time_b[j] : 0.0f;
  const int64_t first = blockIdx.x * (int64_t)kRows;
  float acc_w = 0.0f, acc_b = 0.0f;
  for (int32_t r = wid; r < kRows; r += 4) {
    const int64_t i = first + r;
    if (i >= a.n) break;              // wave-uniform
    if (!a.has[i] || !col_ok) continue;  // a row without a message contributes nothing, whatever its gradient holds
    const float dt = a.dt[i];
    const float gb = glx_pin(a.g[i * (int64_t)a.width + a.time_off + j] * -sinf(fmaf(w, dt, b)));
    acc_b = acc_b + gb;
    acc_w = acc_w + glx_pin(gb * dt);
  }
  part[0][wid][lane] = acc_w;
  part[1][wid][lane] = acc_b;
  __syncthreads();
  if (wid < 2 && col_ok) {
    const float s = (part[wid][0][lane] + part[wid][1][lane]) + (part[wid][2][lane] + part[wid][3][lane]);
    a.partial[((int64_t)blockIdx.x * 2 + wid) * a.T + j] = s;
  }
}

__global__ __launch_bounds__(256) void glx_tgn_bwd_chunks_kernel(BwdArgs a) {
  const int lane = threadIdx.x & 63;
  const int32_t o = blockIdx.x * 4 + (threadIdx.x >> 6);  // output word: which * T + j
  if (o >= 2 * a.T) return;                               // whole waves leave
  const int32_t which = o / a.T, j = o % a.T;
  float acc = 0.0f;
  for (int32_t k = lane; k < a.chunks; k += 64) acc = acc + a.partial[((int64_t)k * 2 + which) * a.T + j];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc = acc + __shfl_xor(acc, off);
  if (lane == 0) (which ? a.grad_b : a.grad_w)[j] = acc;
}

// ---- the memory write --------------------------------------------------------------------------------------
struct WriteArgs {
  const int64_t* n_id;       // [n]
  const float* new_memory;   // [n, M]
  const int64_t* t_new;      // [n]
  float* memory;             // [N, M]
  int64_t* last_update;      // [N]
  int64_t num_nodes;
  int32_t M, n;
};

template <int G>
__global__ __launch_bounds__(256) void glx_tgn_memory_write_kernel(WriteArgs a) {
  const int64_t i = blockIdx.x * (int64_t)(256 / G) + threadIdx.x / G;
  const int c = threadIdx.x & (G - 1);
  if (i >= a.n) return;  // whole groups leave
  const int64_t v = a.n_id[i];
  if (!tgn_in(v, a.num_nodes)) return;
  if (c == 0) a.last_update[v] = a.t_new[i];
  tgn_put<G>(a.memory + v * (int64_t)a.M, a.new_memory + i * (int64_t)a.M, a.M, c);
}

inline unsigned tgn_blocks(int64_t items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

}  // namespace

// what the entry points check alike, before any device use
#define GLX_TGN_REQUIRE_TABLE(dim_name, dim)                                                                            \
  GLX_REQUIRE(num_nodes >= 0, "negative sizes: num_nodes %lld", (long long)num_nodes);                                  \
  GLX_REQUIRE(num_nodes < INT32_MAX, "num_nodes must be < 2^31");                                                       \
  GLX_REQUIRE(dim >= 0, dim_name " must not be negative, got %d", dim)

extern "C" int glx_tgn_store_update(int device, int64_t num_nodes, int32_t raw_dim, const int64_t* src, const int64_t* dst,
                                    const int64_t* t, const float* raw_msg, int32_t batch, int64_t seq_base,
                                    int64_t* pend_t, int64_t* pend_seq, int64_t* pend_other, float* pend_raw,
                                    void* stream) {
  GLX_TGN_REQUIRE_TABLE("raw_dim", raw_dim);
  GLX_REQUIRE(batch >= 0 && batch <= INT32_MAX / 2, "batch must be in [0, 2^30), got %d", batch);
  GLX_REQUIRE(seq_base >= 0 && seq_base <= INT64_MAX - batch, "seq_base out of range: %lld", (long long)seq_base);
  GLX_REQUIRE(batch == 0 || src != nullptr, "src is NULL");
  GLX_REQUIRE(batch == 0 || dst != nullptr, "dst is NULL");
  GLX_REQUIRE(batch == 0 || t != nullptr, "t is NULL");
  GLX_REQUIRE(batch == 0 || raw_dim == 0 || raw_msg != nullptr, "raw_msg is NULL");
  GLX_REQUIRE(num_nodes == 0 || pend_t != nullptr, "pend_t is NULL");
  GLX_REQUIRE(num_nodes == 0 || pend_seq != nullptr, "pend_seq is NULL");
  GLX_REQUIRE(num_nodes == 0 || pend_other != nullptr, "pend_other is NULL");
  GLX_REQUIRE(num_nodes == 0 || raw_dim == 0 || pend_raw != nullptr, "pend_raw is NULL");
  int rc = glx_init_device(device);
  if (rc != GLX_OK) return rc;
  if (batch == 0 || num_nodes == 0) return GLX_OK;
  GlxDeviceGuard guard(device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", device);
  StoreArgs a;
  a.src = src;
  a.dst = dst;
  a.t = t;
  a.raw = raw_msg;
  a.pend_t = pend_t;
  a.pend_seq = pend_seq;
  a.pend_other = pend_other;
  a.pend_raw = pend_raw;
  a.num_nodes = num_nodes;
  a.seq_base = seq_base;
  a.batch = batch;
  a.raw_dim = raw_dim;
  hipStream_t s = glx_stream(stream);
  const int64_t cands = 2 * (int64_t)batch;
  glx_tgn_maxt_kernel<<<tgn_blocks(cands, 256), 256, 0, s>>>(a);
  glx_tgn_maxseq_kernel<<<tgn_blocks(cands, 256), 256, 0, s>>>(a);
  const int G = glx_group_for((raw_dim + 3) / 4);
  glx_for_group(G, [&](auto g) {
    constexpr int GG = decltype(g)::value;
    glx_tgn_store_write_kernel<GG><<<tgn_blocks(cands, 256 / GG), 256, 0, s>>>(a);
  });
  GLX_HIP(hipGetLastError());
  return GLX_OK;
}

extern "C" int glx_tgn_message(int device, int64_t num_nodes, int32_t mem_dim, int32_t raw_dim, int32_t time_dim,
                               const float* memory, const int64_t* last_update, const int64_t* pend_t,
                               const int64_t* pend_seq, const int64_t* pend_other, const float* pend_raw,
                               const float* time_w, const float* time_b, const int64_t* n_id, int32_t n, float* msg_out,
                               float* h_out, float* dt_out, int64_t* t_out, int32_t* has_out, void* stream) {
  GLX_TGN_REQUIRE_TABLE("raw_dim", raw_dim);
  GLX_REQUIRE(mem_dim >= 1, "mem_dim must be positive, got %d", mem_dim);
  GLX_REQUIRE(time_dim >= 0, "time_dim must not be negative, got %d", time_dim);
  GLX_REQUIRE(n >= 0, "negative sizes: n %d", n);
  GLX_REQUIRE(2 * (int64_t)mem_dim + raw_dim + time_dim <= INT32_MAX, "the message width exceeds int32");
  GLX_REQUIRE(num_nodes == 0 || memory != nullptr, "memory is NULL");
  GLX_REQUIRE(num_nodes == 0 || last_update != nullptr, "last_update is NULL");
  GLX_REQUIRE(num_nodes == 0 || pend_t != nullptr, "pend_t is NULL");
  GLX_REQUIRE(num_nodes == 0 || pend_seq != nullptr, "pend_seq is NULL");
  GLX_REQUIRE(num_nodes == 0 || pend_other != nullptr, "pend_other is NULL");
  GLX_REQUIRE(num_nodes == 0 || raw_dim == 0 || pend_raw != nullptr, "pend_raw is NULL");
  GLX_REQUIRE(time_dim == 0 || (time_w != nullptr && time_b != nullptr), "time_w or time_b is NULL");
  GLX_REQUIRE(n == 0 || n_id != nullptr, "n_id is NULL");
  GLX_REQUIRE(n == 0 || (msg_out != nullptr && h_out != nullptr), "msg_out or h_out is NULL");
  GLX_REQUIRE(n == 0 || (dt_out != nullptr && t_out != nullptr && has_out != nullptr),
              "dt_out, t_out or has_out is NULL");
  int rc = glx_init_device(device);
  if (rc != GLX_OK) return rc;
  if (n == 0) return GLX_OK;
  GlxDeviceGuard guard(device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", device);
  MsgArgs a;
  a.memory = memory;
  a.last_update = last_update;
  a.pend_t = pend_t;
  a.pend_seq = pend_seq;
  a.pend_other = pend_other;
  a.pend_raw = pend_raw;
  a.time_w = time_w;
  a.time_b = time_b;
  a.n_id = n_id;
  a.msg = msg_out;
  a.h = h_out;
  a.dt = dt_out;
  a.t_out = t_out;
  a.has = has_out;
  a.num_nodes = num_nodes;
  a.M = mem_dim;
  a.R = raw_dim;
  a.T = time_dim;
  a.n = n;
  hipStream_t s = glx_stream(stream);
  const int32_t widest = mem_dim > raw_dim ? mem_dim : raw_dim;
  const int G = glx_group_for(((widest > time_dim ? widest : time_dim) + 3) / 4);
  glx_for_group(G, [&](auto g) {
    constexpr int GG = decltype(g)::value;
    glx_tgn_message_kernel<GG><<<tgn_blocks(n, 256 / GG), 256, 0, s>>>(a);
  });
  GLX_HIP(hipGetLastError());
  return GLX_OK;
}

extern "C" int glx_tgn_message_backward(int device, int32_t n, int32_t width, int32_t time_off, int32_t time_dim,
                                        const float* grad_msg, const float* dt, const int32_t* has, const float* time_w,
                                        const float* time_b, float* grad_w, float* grad_b, void* stream) {
  GLX_REQUIRE(n >= 0, "negative sizes: n %d", n);
  GLX_REQUIRE(time_dim >= 1, "time_dim must be positive, got %d", time_dim);
  GLX_REQUIRE(time_off >= 0 && width >= 1 && (int64_t)time_off + time_dim <= width,
              "columns [%d, %d + %d) do not lie in a row of %d", time_off, time_off, time_dim, width);
  GLX_REQUIRE(n == 0 || grad_msg != nullptr, "grad_msg is NULL");
  GLX_REQUIRE(n == 0 || (dt != nullptr && has != nullptr), "dt or has is NULL");
  GLX_REQUIRE(time_w != nullptr && time_b != nullptr, "time_w or time_b is NULL");
  GLX_REQUIRE(grad_w != nullptr && grad_b != nullptr, "grad_w or grad_b is NULL");
  int rc = glx_init_device(device);
  if (rc != GLX_OK) return rc;
  GlxDeviceGuard guard(device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", device);
  hipStream_t s = glx_stream(stream);
  if (n == 0) {
    rc = glx_zero_f32_async(grad_w, (size_t)time_dim, s);
    return rc != GLX_OK ? rc : glx_zero_f32_async(grad_b, (size_t)time_dim, s);
  }
  BwdArgs a;
  a.g = grad_msg;
  a.dt = dt;
  a.has = has;
  a.time_w = time_w;
  a.time_b = time_b;
  a.grad_w = grad_w;
  a.grad_b = grad_b;
  a.n = n;
  a.width = width;
  a.time_off = time_off;
  a.T = time_dim;
  a.chunks = (int32_t)(((int64_t)n + kRows - 1) / kRows);
  GlxScratch lease;
  rc = lease.alloc((size_t)a.chunks * 2 * time_dim * sizeof(float), s, 1);
  if (rc != GLX_OK) return rc;
  a.partial = lease.as<float>();
  glx_tgn_bwd_rows_kernel<<<dim3((unsigned)a.chunks, tgn_blocks(time_dim, 64)), 256, 0, s>>>(a);
  glx_tgn_bwd_chunks_kernel<<<tgn_blocks(2 * (int64_t)time_dim, 4), 256, 0, s>>>(a);
  GLX_HIP(hipGetLastError());
  return GLX_OK;
}

extern "C" int glx_tgn_memory_write(int device, int64_t num_nodes, int32_t mem_dim, const int64_t* n_id, int32_t n,
                                    const float* new_memory, const int64_t* t_new, float* memory, int64_t* last_update,
                                    void* stream) {
  GLX_TGN_REQUIRE_TABLE("mem_dim", mem_dim);
  GLX_REQUIRE(mem_dim >= 1, "mem_dim must be positive, got %d", mem_dim);
  GLX_REQUIRE(n >= 0, "negative sizes: n %d", n);
  GLX_REQUIRE(n == 0 || n_id != nullptr, "n_id is NULL");
  GLX_REQUIRE(n == 0 || new_memory != nullptr, "new_memory is NULL");
  GLX_REQUIRE(n == 0 || t_new != nullptr, "t_new is NULL");
  GLX_REQUIRE(num_nodes == 0 || memory != nullptr, "memory is NULL");
  GLX_REQUIRE(num_nodes == 0 || last_update != nullptr, "last_update is NULL");
  int rc = glx_init_device(device);
  if (rc != GLX_OK) return rc;
  if (n == 0 || num_nodes == 0) return GLX_OK;
  GlxDeviceGuard guard(device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", device);
  WriteArgs a;
  a.n_id = n_id;
  a.new_memory = new_memory;
  a.t_new = t_new;
  a.memory = memory;
  a.last_update = last_update;
  a.num_nodes = num_nodes;
  a.M = mem_dim;
  a.n = n;
  hipStream_t s = glx_stream(stream);
  const int G = glx_group_for((mem_dim + 3) / 4);
  glx_for_group(G, [&](auto g) {
    constexpr int GG = decltype(g)::value;
    glx_tgn_memory_write_kernel<GG><<<tgn_blocks(n, 256 / GG), 256, 0, s>>>(a);
  });
  GLX_HIP(hipGetLastError());
  return GLX_OK;
}
