// glx differentiable aggregation: the gradient of glx_aggregate with respect to the table rows, and the recording
// forward that Max / Min need.  The reference's model layers sit on differentiable segment reductions
// (graphlearn/python/nn/tf/layers/sage_conv.py:69-73, gcn_conv.py:73: unsorted_segment_sum / unsorted_segment_mean);
// its operator API (aggregator.cc:25-86) has no backward of its own.
//
// Contract: segment s of the request is positions [sum(cnt[:s]), sum(cnt[:s]) + cnt[s]) -- what the
// forward's cursor (aggregating_request.cc:86-105) consumed; positions from sum(cnt) on, and positions whose row is
// outside [0, num_rows), give nothing.  grad_x[r, c] starts at +0.0f and adds one float32 term per consumed position
// p with rows[p] == r in ASCENDING p (Sum: grad_out[s(p), c]; Mean: grad_out[s(p), c] / float(cnt[s(p)]); Max / Min:
// grad_out[s(p), c] when arg[s(p), c] == p).  No float atomics anywhere: the result is a function of the inputs alone.
//
// Backward = transpose + gather-reduce:
//   keys      key[p] = rows[p] for a consumed, in-range position, num_rows (the sentinel bucket) otherwise; a ragged
//             request also notes each position's segment (upper bound in the inclusive prefix sums of cnt)
//   sort      STABLE radix sort of (key, p) over ceil(log2(num_rows + 1)) bits: row r's positions end up contiguous
//             and ascending
//   row_ptr   row_ptr[r] = lower bound of r in the sorted keys, r in [0, num_rows]
//   reduce    glx_row_grad_kernel (glx_chunks.h): the mirror image of the forward's grouped kernel -- G lanes own one
//             TABLE row, lane c owns columns [4c, 4c + 4), the row's list entries are fetched coalesced (G at a time)
//             and handed round with cross-lane reads, U grad_out row loads are issued before the first is folded.
// grad_x is float32 or bfloat16 (glx_aggregate_backward_ex): the sum above is float32 either way, and a
// bfloat16 grad_x stores it rounded once per element, to nearest even (glx_f32_to_bf16_bits), in the reduce's final store.
// The workspace is the per-(thread, device, stream) arena; nothing is read back on the host between the launches.
// The transpose (glx_agg_transpose, declared in glx_common.h) also serves the weighted reduce's row gradient
// (glx_aggregate_weighted.hip).
//
// The CHUNKED order (glx_aggregate_backward_chunked) is a second, opt-in contract for the
// same terms, over the chunks of a row's list (entries, selected by a Max / Min arg or not): glx_chunks.h has the
// order, the chunk directory and the kernels, which are the ones of the default order; this file has the term, and the
// two kernels of the chunked order that are no templates of a request (the directory's items, the combine).  Every row
// is still written exactly once, and nothing proportional to [num_rows, dim] is allocated.
#include "glx_chunks.h"

namespace {

// ---- the recording forward (Max / Min) ---------------------------------------------------------------------
struct ArgFwdArgs {
  GlxIdMap map;
  const void* X;
  int64_t stride, swizzle_rows;
  const int64_t* ids;
  GlxSegments seg;
  float* emb;
  int32_t* cnt;
  int32_t* arg;
  int32_t dim, num_segments;
  float default_attr;
  int32_t G;  // lanes per segment (a power of two <= 64)
};

constexpr int kArgU = 4;  // rows in flight per lane

// A group of a.G lanes owns one segment; lane c owns columns [VEC c, VEC c + VEC) of every column tile and folds the
// segment's rows left to right with the forward's own select (agg_combine: Max (l < r) ? r : l, Min (r < l) ? r : l),
// so emb equals glx_aggregate's bit for bit; arg is the position the select last took (-1: it never took one).
template <int OP, int VEC, int DT>
__global__ __launch_bounds__(256) void glx_aggregate_arg_kernel(ArgFwdArgs a) {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  typedef int32_t ivec_t __attribute__((ext_vector_type(VEC)));
  typedef typename AggElem<DT>::raw raw_t;
  const raw_t* __restrict__ X = static_cast<const raw_t*>(a.X);
  const int64_t gid = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / a.G;
  const int c = threadIdx.x & (a.G - 1);
  if (gid >= a.num_segments) return;
  int32_t s0, s1;
  if (a.seg.seg_start && seg_level(a.seg.state) != 0) {
    s0 = a.seg.seg_start[gid];
    s1 = a.seg.seg_start[gid + 1];
  } else {  // a dense sampler response: segment gid = ids [gid * fanout, (gid + 1) * fanout)
    s0 = (int32_t)gid * a.seg.fanout;
    s1 = s0 + a.seg.fanout;
  }
  const int32_t n = s1 - s0;
  if (c == 0) a.cnt[gid] = n;
  const int64_t out_at = gid * (int64_t)a.dim;
  for (int32_t col = c * VEC; col < a.dim; col += a.G * VEC) {
    vec_t acc;
    ivec_t at;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      acc[v] = agg_init<OP>();
      at[v] = -1;
    }
    for (int32_t base = s0; base < s1; base += kArgU) {
      int64_t row[kArgU];
#pragma unroll
      for (int u = 0; u < kArgU; ++u) row[u] = (base + u < s1) ? glx_row_of(a.map, a.ids[base + u]) : -2;
      vec_t val[kArgU];
#pragma unroll
      for (int u = 0; u < kArgU; ++u) {
        if (row[u] >= 0) {
          val[u] = agg_load<DT, VEC>(X + glx_swizzle_row(row[u], a.swizzle_rows) * a.stride + col);
        } else {
#pragma unroll
          for (int v = 0; v < VEC; ++v) val[u][v] = a.default_attr;
        }
      }
#pragma unroll
      for (int u = 0; u < kArgU; ++u) {
        if (row[u] != -2) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            const bool take = OP == GLX_AGG_MAX ? (acc[v] < val[u][v]) : (val[u][v] < acc[v]);
            acc[v] = take ? val[u][v] : acc[v];
            at[v] = take ? base + u : at[v];
          }
        }
      }
    }
    if (n == 0) {  // FinalFunc: aggregator.cc:74-86 (empty -> default)
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] = a.default_attr;
    }
    *reinterpret_cast<vec_t*>(a.emb + out_at + col) = acc;
    *reinterpret_cast<ivec_t*>(a.arg + out_at + col) = at;
  }
}

template <int OP, int DT>
void launch_arg_fwd(ArgFwdArgs a, hipStream_t s) {
  constexpr size_t kElem = sizeof(typename AggElem<DT>::raw);
  const bool vec4 = a.dim % 4 == 0 && a.stride % 4 == 0 && (reinterpret_cast<uintptr_t>(a.X) % (4 * kElem)) == 0 &&
                    glx_aligned16(a.emb) && glx_aligned16(a.arg);
  const int lanes = vec4 ? a.dim / 4 : a.dim;
  int G = 1;
  while (G < 64 && G < lanes) G <<= 1;
  a.G = G;
  const unsigned grid = (unsigned)(((int64_t)a.num_segments * G + 255) / 256);
  if (vec4) glx_aggregate_arg_kernel<OP, 4, DT><<<grid, 256, 0, s>>>(a);
  else glx_aggregate_arg_kernel<OP, 1, DT><<<grid, 256, 0, s>>>(a);
}

template <int OP>
void launch_arg_fwd_dt(const ArgFwdArgs& a, int dtype, hipStream_t s) {
  if (dtype == GLX_DTYPE_BF16) launch_arg_fwd<OP, GLX_DTYPE_BF16>(a, s);
  else if (dtype == GLX_DTYPE_F16) launch_arg_fwd<OP, GLX_DTYPE_F16>(a, s);
  else if (dtype == GLX_DTYPE_F8E4M3) launch_arg_fwd<OP, GLX_DTYPE_F8E4M3>(a, s);
  else if (dtype == GLX_DTYPE_F8E5M2) launch_arg_fwd<OP, GLX_DTYPE_F8E5M2>(a, s);
  else launch_arg_fwd<OP, GLX_DTYPE_F32>(a, s);
}

// ---- backward: transpose -----------------------------------------------------------------------------------
struct ClampCount {
  __host__ __device__ int64_t operator()(int32_t v) const { return v > 0 ? (int64_t)v : 0; }
};

// key / value / segment of every position of the request L describes
__global__ __launch_bounds__(256) void glx_bwd_keys_kernel(const int64_t* __restrict__ rows, int64_t num_rows,
                                                           GlxSegLayout L, uint32_t* __restrict__ keys,
                                                           int32_t* __restrict__ vals, int32_t* __restrict__ seg_of) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p >= L.num_ids) return;
  int32_t sg;
  const bool consumed = seg_of_position(L, p, &sg);
  if (L.seg_end != nullptr) seg_of[p] = sg;
  const int64_t r = rows[p];
  const bool in = consumed && r >= 0 && r < num_rows;
  keys[p] = in ? (uint32_t)r : (uint32_t)num_rows;
  vals[p] = (int32_t)p;
}

__global__ __launch_bounds__(256) void glx_bwd_row_ptr_kernel(const uint32_t* __restrict__ keys, int32_t n, int64_t num_rows,
                                                              int32_t* __restrict__ row_ptr) {
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r > num_rows) return;
  int32_t lo = 0, hi = n;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)keys[mid] < r) lo = mid + 1; else hi = mid;
  }
  row_ptr[r] = lo;
}

}  // namespace

// The transpose of one request (glx_common.h): keys, stable sort, row_ptr.  One lease of workspace slot kSlotRequest
// holds every piece; it ends with the caller's GlxScratch.
int glx_agg_transpose(const int64_t* rows, const int32_t* cnt, int32_t n, int32_t num_segments, int64_t num_rows,
                      hipStream_t s, GlxScratch* lease, GlxAggTranspose* out) {
  int bits = 1;
  while (bits < 32 && ((uint64_t)1 << bits) <= (uint64_t)num_rows) ++bits;  // the sentinel key num_rows fits
  const bool ragged = cnt != nullptr;
  uint32_t* const no_keys = nullptr;
  int32_t* const no_vals = nullptr;
  size_t sort_tmp = 0, scan_tmp = 0;
  GLX_HIP(rocprim::radix_sort_pairs(nullptr, sort_tmp, no_keys, no_keys, no_vals, no_vals, (size_t)n, 0, bits, s));
  if (ragged) {
    GLX_HIP(rocprim::inclusive_scan(nullptr, scan_tmp, rocprim::make_transform_iterator(cnt, ClampCount()),
                                    static_cast<int64_t*>(nullptr), (size_t)num_segments, rocprim::plus<int64_t>(), s));
  }
  const size_t tmp_b = glx_align256(sort_tmp > scan_tmp ? sort_tmp : scan_tmp);
  const size_t ids_b = glx_align256((size_t)n * sizeof(int32_t));
  const size_t end_b = ragged ? glx_align256((size_t)num_segments * sizeof(int64_t)) : 0;
  const size_t ptr_b = glx_align256((size_t)(num_rows + 1) * sizeof(int32_t));
  int rc = lease->alloc(tmp_b + (ragged ? 5 : 4) * ids_b + end_b + ptr_b, s, kSlotRequest);
  if (rc != GLX_OK) return rc;
  char* at = lease->as<char>();
  void* tmp = at;
  at += tmp_b;
  uint32_t* keys = reinterpret_cast<uint32_t*>(at);
  uint32_t* keys_s = reinterpret_cast<uint32_t*>(at + ids_b);
  int32_t* vals = reinterpret_cast<int32_t*>(at + 2 * ids_b);
  int32_t* vals_s = reinterpret_cast<int32_t*>(at + 3 * ids_b);
  at += 4 * ids_b;
  int32_t* seg_of = nullptr;
  int64_t* seg_end = nullptr;
  if (ragged) {
    seg_of = reinterpret_cast<int32_t*>(at);
    seg_end = reinterpret_cast<int64_t*>(at + ids_b);
    at += ids_b + end_b;
  }
  int32_t* row_ptr = reinterpret_cast<int32_t*>(at);
  if (ragged) {
    GLX_HIP(rocprim::inclusive_scan(tmp, scan_tmp, rocprim::make_transform_iterator(cnt, ClampCount()), seg_end,
                                    (size_t)num_segments, rocprim::plus<int64_t>(), s));
  }
  const int32_t fanout = n / num_segments;  // the keys kernel takes it raw: 0 consumes nothing
  const GlxSegLayout L = {seg_end, fanout, n, num_segments};
  glx_bwd_keys_kernel<<<(unsigned)(((int64_t)n + 255) / 256), 256, 0, s>>>(rows, num_rows, L, keys, vals, seg_of);
  GLX_HIP(rocprim::radix_sort_pairs(tmp, sort_tmp, keys, keys_s, vals, vals_s, (size_t)n, 0, bits, s));
  glx_bwd_row_ptr_kernel<<<(unsigned)((num_rows + 1 + 255) / 256), 256, 0, s>>>(keys_s, n, num_rows, row_ptr);
  out->row_ptr = row_ptr;
  out->pos = vals_s;
  out->seg_of = seg_of;
  out->seg_end = seg_end;
  out->fanout = fanout > 0 ? fanout : 1;  // published at least 1: with 0 every list is empty, nothing divides by it
  return GLX_OK;
}

// Inclusive prefix sums of the clamped counts (the segment ends of a ragged request), in a lease of workspace slot
// kSlotRequest.
int glx_agg_segment_ends(const int32_t* cnt, int32_t num_segments, hipStream_t s, GlxScratch* lease,
                         const int64_t** seg_end) {
  size_t scan_tmp = 0;
  GLX_HIP(rocprim::inclusive_scan(nullptr, scan_tmp, rocprim::make_transform_iterator(cnt, ClampCount()),
                                  static_cast<int64_t*>(nullptr), (size_t)num_segments, rocprim::plus<int64_t>(), s));
  const size_t tmp_b = glx_align256(scan_tmp);
  int rc = lease->alloc(tmp_b + (size_t)num_segments * sizeof(int64_t), s, kSlotRequest);
  if (rc != GLX_OK) return rc;
  int64_t* ends = reinterpret_cast<int64_t*>(lease->as<char>() + tmp_b);
  GLX_HIP(rocprim::inclusive_scan(lease->p, scan_tmp, rocprim::make_transform_iterator(cnt, ClampCount()), ends,
                                  (size_t)num_segments, rocprim::plus<int64_t>(), s));
  *seg_end = ends;
  return GLX_OK;
}

namespace {

// ---- backward: reduce --------------------------------------------------------------------------------------
struct BwdArgs {
  const int32_t* row_ptr;  // [num_rows + 1] into pos
  const int32_t* pos;      // request positions by (row, position)
  const int32_t* seg_of;   // [num_ids] segment of a position, or nullptr: position / fanout
  const int32_t* cnt;      // [num_segments], or nullptr: fanout (Mean's divisor)
  const int32_t* arg;      // [num_segments, dim] (Max / Min)
  const float* grad_out;   // [num_segments, dim]
  void* grad_x;            // [num_rows, dim] of `dtype` elements
  int64_t num_rows;
  int32_t dim, fanout;
  int dtype;               // GLX_DTYPE_F32 or GLX_DTYPE_BF16: grad_x's element type
};

constexpr int kBwdU = 4;  // grad_out rows in flight per lane

// The term of one list entry for the lane's VEC columns from `col` on: Sum g, Mean g / float(count), Max / Min g where
// arg names the entry's position (an entry arg does not select adds nothing, and is still a list entry).
template <int OP, int VEC>
struct BwdTerm {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  typedef int32_t ivec_t __attribute__((ext_vector_type(VEC)));
  static constexpr bool kArg = OP == GLX_AGG_MAX || OP == GLX_AGG_MIN;
  static constexpr bool kDiv = OP == GLX_AGG_MEAN;
  struct Loaded {
    vec_t g;
    ivec_t w;
  };
  const BwdArgs& a;
  int32_t col;
  // the RAW count, not seg_count: counts that promise more than the request has still divide by what they say
  __device__ __forceinline__ float divisor(int32_t seg) const { return (float)(a.cnt ? a.cnt[seg] : a.fanout); }
  __device__ __forceinline__ void load(Loaded* ld, int32_t, int32_t seg) const {
    const int64_t at = (int64_t)seg * a.dim + col;
    ld->g = *reinterpret_cast<const vec_t*>(a.grad_out + at);
    if (kArg) ld->w = *reinterpret_cast<const ivec_t*>(a.arg + at);
  }
  __device__ __forceinline__ void fold(vec_t* acc, const Loaded& ld, int32_t p, float dv) const {
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      if (kArg) {
        if (ld.w[v] == p) (*acc)[v] = (*acc)[v] + ld.g[v];
      } else if (kDiv) {
        (*acc)[v] = (*acc)[v] + ld.g[v] / dv;
      } else {
        (*acc)[v] = (*acc)[v] + ld.g[v];
      }
    }
  }
};

// the request of glx_row_grad_launch (glx_chunks.h)
template <int OP>
struct BwdReq {
  static constexpr int kU = kBwdU;
  BwdArgs a;
  __host__ __device__ const int32_t* row_ptr() const { return a.row_ptr; }
  __device__ GlxPosList list() const { return {a.pos, a.seg_of, a.fanout}; }
  __host__ __device__ int64_t num_rows() const { return a.num_rows; }
  __host__ __device__ int32_t dim() const { return a.dim; }
  __host__ __device__ void* grad_x() const { return a.grad_x; }
  int dtype() const { return a.dtype; }
  template <int VEC>
  __device__ BwdTerm<OP, VEC> term(int32_t col) const { return {a, col}; }
};

// ch == nullptr: the default order; otherwise the chunked one over that directory
template <int OP>
void launch_bwd(const BwdArgs& a, const GlxChunkDir* ch, hipStream_t s) {
  bool vec4 = a.dim % 4 == 0 && glx_aligned16(a.grad_out) && glx_aligned_vec4(a.grad_x, a.dtype);
  if (OP == GLX_AGG_MAX || OP == GLX_AGG_MIN) vec4 = vec4 && glx_aligned16(a.arg);
  if (vec4) glx_row_grad_launch<4>(BwdReq<OP>{a}, ch, s);
  else glx_row_grad_launch<1>(BwdReq<OP>{a}, ch, s);
}

// Device pointers only, device selected; num_ids, num_segments, num_rows >= 1.
int backward_device(int op, const int64_t* rows, const int32_t* cnt, const int32_t* arg, int32_t n, int32_t num_segments,
                    int64_t num_rows, int32_t dim, const float* grad_out, void* grad_x, int grad_x_dtype, bool chunked,
                    hipStream_t s) {
  GlxScratch lease, chunk_lease;
  GlxAggTranspose t;
  int rc = glx_agg_transpose(rows, cnt, n, num_segments, num_rows, s, &lease, &t);
  if (rc != GLX_OK) return rc;
  GlxChunkDir chunks;
  const GlxChunkDir* ch = nullptr;
  if (chunked) {
    rc = glx_row_chunk_dir(t, n, num_rows, dim, s, &chunk_lease, &chunks);
    if (rc != GLX_OK) return rc;
    ch = &chunks;
  }
  BwdArgs a;
  a.row_ptr = t.row_ptr;
  a.pos = t.pos;
  a.seg_of = t.seg_of;
  a.cnt = cnt;
  a.arg = arg;
  a.grad_out = grad_out;
  a.grad_x = grad_x;
  a.num_rows = num_rows;
  a.dim = dim;
  a.fanout = t.fanout;
  a.dtype = grad_x_dtype;
  switch (op) {
    case GLX_AGG_SUM: launch_bwd<GLX_AGG_SUM>(a, ch, s); break;
    case GLX_AGG_MEAN: launch_bwd<GLX_AGG_MEAN>(a, ch, s); break;
    case GLX_AGG_MAX: launch_bwd<GLX_AGG_MAX>(a, ch, s); break;
    default: launch_bwd<GLX_AGG_MIN>(a, ch, s); break;
  }
  GLX_HIP(hipGetLastError());
  return GLX_OK;
}

// ---- the items and the combine pass of the chunked order (glx_chunks.h) ---------------------------------------
// work item t belongs to the last list whose first slot is at or below t (lists without chunks share their successor's)
__global__ __launch_bounds__(256) void glx_chunk_items_kernel(const int32_t* __restrict__ slot0, int64_t num_lists,
                                                              int32_t max_items, int32_t* __restrict__ item_list) {
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= max_items || t >= slot0[num_lists]) return;
  int64_t lo = 0, hi = num_lists;  // the first index whose slot0 exceeds t: slot0[num_lists] does
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (slot0[mid] > t) hi = mid; else lo = mid + 1;
  }
  item_list[t] = (int32_t)(lo - 1);
}

// G lanes own work item t and leave unless it is the first of its list; lane c owns columns [VEC c, VEC c + VEC) of
// each column tile.  kBwdU partial-sum loads are issued before the first is added.
template <int G, int VEC, int DT>
__global__ __launch_bounds__(256) void glx_chunks_combine_kernel(GlxChunkDir ch, void* dst, int32_t dim) {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  typedef typename AggElem<DT>::raw raw_t;
  const int64_t t = blockIdx.x * (int64_t)(256 / G) + threadIdx.x / G;
  const int c = threadIdx.x & (G - 1);
  if (GLX_CHUNK_IDLE(ch, t)) return;  // whole groups leave
  const int32_t r = ch.item_list[t];
  if (!GLX_CHUNK_FIRST(ch, t, r)) return;
  const int32_t chunks = ch.slot0[r + 1] - (int32_t)t;
  raw_t* const out = static_cast<raw_t*>(dst) + r * (int64_t)dim;
  for (int32_t col = c * VEC; col < dim; col += G * VEC) {
    vec_t acc;
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.0f;
    for (int32_t k = 0; k < chunks; k += kBwdU) {
      vec_t val[kBwdU];
#pragma unroll
      for (int u = 0; u < kBwdU; ++u) {
        if (k + u < chunks) val[u] = *reinterpret_cast<const vec_t*>(ch.partial + (t + k + u) * dim + col);
      }
#pragma unroll
      for (int u = 0; u < kBwdU; ++u) {
        if (k + u < chunks) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[v] = acc[v] + val[u][v];
        }
      }
    }
    agg_store<DT, VEC>(out + col, acc);
  }
}

}  // namespace

void glx_chunk_items(const int32_t* slot0, int64_t num_lists, int32_t max_items, int32_t* item_list, hipStream_t s) {
  glx_chunk_items_kernel<<<(unsigned)(((int64_t)max_items + 255) / 256), 256, 0, s>>>(slot0, num_lists, max_items,
                                                                                       item_list);
}

int glx_row_chunk_dir(const GlxAggTranspose& t, int32_t n, int64_t num_rows, int32_t dim, hipStream_t s,
                      GlxScratch* lease, GlxChunkDir* out) {
  return glx_chunk_dir(GlxRowLists{t.row_ptr}, num_rows, n, dim, kSlotRowChunks,
                       "chunked row gradient: scan the long rows' chunk counts", s, lease, out);
}

void glx_chunks_combine(const GlxChunkDir& ch, void* out, int out_dtype, int32_t dim, bool vec4, hipStream_t s) {
  const int G = glx_group_for(vec4 ? dim / 4 : dim);
  const unsigned blocks = (unsigned)(((int64_t)ch.max_items + (256 / G) - 1) / (256 / G));
  glx_for_group(G, [&](auto g) {
    glx_for_train_dtype(out_dtype, [&](auto t) {
      constexpr int kG = decltype(g)::value, kDT = decltype(t)::value;
      if (vec4) glx_chunks_combine_kernel<kG, 4, kDT><<<blocks, 256, 0, s>>>(ch, out, dim);
      else glx_chunks_combine_kernel<kG, 1, kDT><<<blocks, 256, 0, s>>>(ch, out, dim);
    });
  });
}

extern "C" int glx_aggregate_arg(const glx_features* f, int op, const int64_t* node_ids, const int32_t* segment_ids,
                                 int32_t num_ids, int32_t num_segments, float default_attr, float* emb_out,
                                 int32_t* cnt_out, int32_t* arg_out, int ptr_kind, void* stream) {
  GLX_REQUIRE(f != nullptr, "features is NULL");
  GLX_REQUIRE(op >= GLX_AGG_SUM && op <= GLX_AGG_PROD, "unknown aggregator id %d", op);
  GLX_REQUIRE(op == GLX_AGG_MAX || op == GLX_AGG_MIN, "glx_aggregate_arg records the argument of Max and Min only, not of %s",
              glx_agg_op_name(op));
  GLX_REQUIRE(num_ids >= 0 && num_segments >= 0, "negative sizes");
  GLX_REQUIRE(ptr_kind == GLX_PTR_HOST || ptr_kind == GLX_PTR_DEVICE, "bad ptr_kind");
  GLX_REQUIRE((int64_t)num_segments * f->dim <= INT32_MAX, "num_segments * dim exceeds int32 (tensor.h:47)");
  if (num_segments == 0) return GLX_OK;
  GLX_REQUIRE(emb_out && cnt_out && arg_out && (num_ids == 0 || node_ids), "NULL data pointer");
  GLX_REQUIRE(segment_ids != nullptr || num_ids % num_segments == 0,
              "segment_ids == NULL means equal segments: num_ids must be a multiple of num_segments");
  GlxDeviceGuard guard(f->device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", f->device);
  GlxHostStage st(f->device, ptr_kind, stream, GlxHostStage::ADMIT | GlxHostStage::DIRECT_PINNED);
  const int64_t* d_ids;
  const int32_t* d_seg;
  float* d_emb;
  int32_t *d_cnt, *d_arg;
  st.in(&d_ids, node_ids, (size_t)num_ids);
  st.in(&d_seg, segment_ids, (size_t)num_ids);
  st.out(&d_emb, emb_out, (size_t)num_segments * f->dim);
  st.out(&d_cnt, cnt_out, (size_t)num_segments);
  st.out(&d_arg, arg_out, (size_t)num_segments * f->dim);
  int rc = st.begin();
  GlxScratch lease;
  if (rc == GLX_OK) {
    rc = lease.alloc(((size_t)num_segments + 1 + kSegScratchExtra) * sizeof(int32_t), st.s, kSlotRequest);
  }
  ArgFwdArgs a;
  if (rc == GLX_OK) rc = glx_segments_prepare(d_seg, num_ids, num_segments, lease.as<int32_t>(), st.s, &a.seg);
  if (rc == GLX_OK) {
    a.map = f->map();
    a.X = f->X;
    a.stride = f->stride;
    a.swizzle_rows = f->swizzle_rows;
    a.ids = d_ids;
    a.emb = d_emb;
    a.cnt = d_cnt;
    a.arg = d_arg;
    a.dim = f->dim;
    a.num_segments = num_segments;
    a.default_attr = default_attr;
    a.G = 1;
    if (op == GLX_AGG_MAX) launch_arg_fwd_dt<GLX_AGG_MAX>(a, f->dtype, st.s);
    else launch_arg_fwd_dt<GLX_AGG_MIN>(a, f->dtype, st.s);
  }
  return st.finish(rc);
}

// the body of glx_aggregate_backward_ex and glx_aggregate_backward_chunked, which have checked grad_x_dtype
static int aggregate_backward(int device, int op, const int64_t* rows, const int32_t* cnt, const int32_t* arg,
                              int32_t num_ids, int32_t num_segments, int64_t num_rows, int32_t dim,
                              const float* grad_out, void* grad_x, int grad_x_dtype, bool chunked, int ptr_kind,
                              void* stream) {
  GLX_REQUIRE(op >= GLX_AGG_SUM && op <= GLX_AGG_PROD, "unknown aggregator id %d", op);
  GLX_REQUIRE(op != GLX_AGG_PROD, "the Prod aggregator has no backward (its gradient divides by the element)");
  GLX_REQUIRE(num_ids >= 0 && num_segments >= 0 && num_rows >= 0, "negative sizes");
  GLX_REQUIRE(dim > 0, "dim must be positive, got %d", dim);
  GLX_REQUIRE(num_rows < INT32_MAX, "num_rows must be < 2^31");
  GLX_REQUIRE(ptr_kind == GLX_PTR_HOST || ptr_kind == GLX_PTR_DEVICE, "bad ptr_kind");
  GLX_REQUIRE(num_ids == 0 || rows != nullptr, "rows is NULL");
  GLX_REQUIRE(num_segments == 0 || grad_out != nullptr, "grad_out is NULL");
  GLX_REQUIRE(num_rows == 0 || grad_x != nullptr, "grad_x is NULL");
  GLX_REQUIRE(num_segments == 0 || arg != nullptr || (op != GLX_AGG_MAX && op != GLX_AGG_MIN),
              "arg is NULL: the %s backward needs the argument glx_aggregate_arg recorded", glx_agg_op_name(op));
  int rc = glx_init_device(device);
  if (rc != GLX_OK) return rc;
  if (num_rows == 0) return GLX_OK;
  GlxDeviceGuard guard(device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", device);
  GlxHostStage st(device, ptr_kind, stream, GlxHostStage::ADMIT);
  const bool with_arg = op == GLX_AGG_MAX || op == GLX_AGG_MIN;
  const int64_t* d_rows;
  const int32_t *d_cnt, *d_arg = nullptr;
  const float* d_go;
  void* d_gx;
  st.in(&d_rows, rows, (size_t)num_ids);
  st.in(&d_cnt, cnt, (size_t)num_segments);
  if (with_arg) st.in(&d_arg, arg, (size_t)num_segments * dim);
  st.in(&d_go, grad_out, (size_t)num_segments * dim);
  st.out_bytes(&d_gx, grad_x, (size_t)num_rows * dim * (size_t)glx_dtype_size(grad_x_dtype));
  rc = st.begin();
  if (rc == GLX_OK) {
    if (num_ids == 0 || num_segments == 0) {  // nothing was consumed: every row is zeros
      rc = glx_zero_elems_async(d_gx, (size_t)num_rows * dim, grad_x_dtype, st.s);
    } else {
      rc = backward_device(op, d_rows, d_cnt, d_arg, num_ids, num_segments, num_rows, dim, d_go, d_gx, grad_x_dtype,
                           chunked, st.s);
    }
  }
  return st.finish(rc);
}

extern "C" int glx_aggregate_backward_ex(int device, int op, const int64_t* rows, const int32_t* cnt,
                                         const int32_t* arg, int32_t num_ids, int32_t num_segments, int64_t num_rows,
                                         int32_t dim, const float* grad_out, void* grad_x, int grad_x_dtype,
                                         int ptr_kind, void* stream) {
  GLX_REQUIRE_TRAIN_DTYPE(grad_x_dtype, "glx_aggregate_backward_ex: grad_x_dtype");
  return aggregate_backward(device, op, rows, cnt, arg, num_ids, num_segments, num_rows, dim, grad_out, grad_x,
                            grad_x_dtype, false, ptr_kind, stream);
}

extern "C" int glx_aggregate_backward_chunked(int device, int op, const int64_t* rows, const int32_t* cnt,
                                              const int32_t* arg, int32_t num_ids, int32_t num_segments,
                                              int64_t num_rows, int32_t dim, const float* grad_out, void* grad_x,
                                              int grad_x_dtype, int ptr_kind, void* stream) {
  GLX_REQUIRE_TRAIN_DTYPE(grad_x_dtype, "glx_aggregate_backward_chunked: grad_x_dtype");
  return aggregate_backward(device, op, rows, cnt, arg, num_ids, num_segments, num_rows, dim, grad_out, grad_x,
                            grad_x_dtype, true, ptr_kind, stream);
}

extern "C" int glx_aggregate_backward(int device, int op, const int64_t* rows, const int32_t* cnt, const int32_t* arg,
                                      int32_t num_ids, int32_t num_segments, int64_t num_rows, int32_t dim,
                                      const float* grad_out, float* grad_x, int ptr_kind, void* stream) {
  return glx_aggregate_backward_ex(device, op, rows, cnt, arg, num_ids, num_segments, num_rows, dim, grad_out, grad_x,
                                   GLX_DTYPE_F32, ptr_kind, stream);
}
