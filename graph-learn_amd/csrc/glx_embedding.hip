// glx trainable embedding tables: the coalesced row gradient of a lookup and the fused sparse optimizer steps.  The
// reference trains tables in two places: the id embeddings of DeepWalk / node2vec (examples/tf/node2vec/node2vec.py:49-50)
// and one EmbeddingColumn per categorical attribute (python/nn/tf/data/feature_column.py:128-157).
//
// Contract (include/glx.h).
//   glx_rows_coalesce    rows[n] int64, g[n, dim] float32.  A position whose row is outside [0, num_rows) is dropped;
//                        the U distinct remaining rows go ascending to urows_out[0 .. U), urows_out[U .. n) = -1,
//                        *num_unique_out = U.  Row u's positions p_0 < p_1 < .. are cut into chunks of
//                        GLX_COALESCE_CHUNK list entries; a chunk's partial is +0.0f plus g[p, c] in ascending p, and
//                        ug_out[u, c] is +0.0f plus the partials in ascending chunk: one fadd_rn each.  ug_out rows from
//                        U on are not written.  Bit-exact; no float atomics.
//   glx_embedding_update for each entry u with urows[u] in [0, num_rows): SGD / Adagrad / Adam on row urows[u] of W and of
//                        the state tables, every operation one correctly rounded float32 operation.
//
// Coalesce = transpose + chunked gather-reduce, nothing proportional to num_rows:
//   keys     key[p] = rows[p], or the sentinel num_rows for a dropped position (glx_bwd_keys_kernel's rule)
//   sort     STABLE radix sort of (key, p) over ceil(log2(num_rows + 1)) bits
//   flags    per sorted position i: is it the head of its run, and is it the head of a chunk of a run that has more
//            than one chunk; one inclusive scan of both counts (packed in one 64-bit word) numbers the distinct rows
//            and the partial-sum slots
//   reduce   one lane group per CHUNK (launched over the n sorted positions; a position that heads no chunk leaves):
//            a run of one chunk is written to ug_out directly (+0.0f + partial == partial), a chunk of a longer run
//            goes to its partial-sum slot
//   combine  one lane group per window of GLX_COALESCE_CHUNK + 1 sorted positions: a run of more than one chunk is
//            longer than that, so a window holds at most one such run's head; its partial sums are added in order.
#include <string.h>  // rocprim's texture_cache_iterator uses memset

#include <rocprim/rocprim.hpp>

#include "glx_lane_groups.h"

// Two roundings per product-and-add: glx_pin / glx_fold_rn (glx_lane_groups.h) pin the product; the pragma is for the
// front end.
#pragma clang fp contract(off)

namespace {

constexpr int kChunk = GLX_COALESCE_CHUNK;
constexpr int kWindow = kChunk + 1;  // sorted positions per group of the combine pass
constexpr int kU = 4;                // row loads in flight per lane

// ---- coalesce: keys, flags -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void glx_emb_keys_kernel(const int64_t* __restrict__ rows, int32_t n, int64_t num_rows,
                                                           uint32_t* __restrict__ keys, int32_t* __restrict__ vals) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int64_t r = rows[p];
  keys[p] = (r >= 0 && r < num_rows) ? (uint32_t)r : (uint32_t)num_rows;
  vals[p] = (int32_t)p;
}

// low word: 1 at the head of a run; high word: 1 at the head of a chunk of a run with more than one chunk
constexpr uint64_t kHead = 1ull, kMulti = 1ull << 32;

__global__ __launch_bounds__(256) void glx_emb_flags_kernel(const uint32_t* __restrict__ keys, int32_t n, uint32_t sentinel,
                                                            uint64_t* __restrict__ flags) {
  const int64_t i64 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i64 >= n) return;
  const int32_t i = (int32_t)i64;
  const uint32_t k = keys[i];
  uint64_t f = 0;
  if (k != sentinel) {
    int32_t off = 0;  // i - (first position of the run)
    if (i > 0 && keys[i - 1] == k) {
      int32_t lo = 0, hi = i;  // lower bound of k in keys[0 .. i)
      while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < k) lo = mid + 1; else hi = mid;
      }
      off = i - lo;
    }
    if (off == 0) f |= kHead;
    if (off % kChunk == 0) {
      const bool more = i < n - kChunk && keys[i + kChunk] == k;  // the run goes on past this chunk
      if (off > 0 || more) f |= kMulti;
    }
  }
  flags[i] = f;
}

// ---- coalesce: reduce ----------------------------------------------------------------------------------------------
struct CoalesceArgs {
  const uint32_t* keys;   // [n] sorted
  const int32_t* pos;     // [n] request positions by (row, position)
  const uint64_t* scan;   // [n] inclusive scan of the flags
  const float* g;         // [n, dim]
  float* ug;              // [n, dim]
  float* partial;         // [n / 128 + 1, dim]
  int64_t* urows;         // [n]
  int64_t* num_unique;    // one word
  int32_t n, dim;
};

// G lanes own sorted position i.  Every group writes its share of the bookkeeping (the -1 tail of urows, position 0
// the count); a group whose position heads a chunk folds the chunk's g rows in ascending list order: lane c fetches
// list entry base + c, every lane reads entry j from lane j, kU row loads are issued before the first is folded.
template <int G, int VEC>
__global__ __launch_bounds__(256) void glx_emb_reduce_kernel(CoalesceArgs a) {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  const int64_t i64 = blockIdx.x * (int64_t)(256 / G) + threadIdx.x / G;
  const int c = threadIdx.x & (G - 1);
  if (i64 >= a.n) return;  // whole groups leave
  const int32_t i = (int32_t)i64;
  const uint64_t total = a.scan[a.n - 1];
  const int32_t U = (int32_t)(uint32_t)total;
  if (c == 0) {
    if (i >= U) a.urows[i] = -1;
    if (i == 0) *a.num_unique = U;
  }
  const uint64_t here = a.scan[i], before = i > 0 ? a.scan[i - 1] : 0;
  const uint64_t f = here - before;
  if (f == 0) return;  // no chunk starts here
  const uint32_t key = a.keys[i];
  const int32_t u = (int32_t)(uint32_t)here - 1;
  if ((f & kHead) && c == 0) a.urows[u] = (int64_t)key;
  // the chunk: [i, end), end = the first position of [i + 1, min(i + kChunk, n)) with another key
  int32_t lo = i + 1, hi = a.n - i > kChunk ? i + kChunk : a.n;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (a.keys[mid] == key) lo = mid + 1; else hi = mid;
  }
  const int32_t len = lo - i;
  float* const out = (f & kMulti) ? a.partial + (int64_t)((int32_t)(here >> 32) - 1) * a.dim : a.ug + (int64_t)u * a.dim;
  for (int32_t col_pass = 0; col_pass < a.dim; col_pass += G * VEC) {
    const int32_t col = col_pass + c * VEC;
    const bool col_ok = col < a.dim;
    const int32_t col_ld = col_ok ? col : 0;  // lanes past the end re-read the first columns, unused
    vec_t acc;
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.0f;
    for (int32_t base = 0; base < len; base += G) {
      const int32_t my_p = base + c < len ? a.pos[i + base + c] : 0;
      const int32_t m = (len - base) < G ? (len - base) : G;
      for (int32_t j = 0; j < m; j += kU) {
        int32_t p[kU];
#pragma unroll
        for (int w = 0; w < kU; ++w) p[w] = __shfl(my_p, (j + w) & (G - 1), G);
        vec_t val[kU];
#pragma unroll
        for (int w = 0; w < kU; ++w) {
          if (j + w < m) val[w] = *reinterpret_cast<const vec_t*>(a.g + (int64_t)p[w] * a.dim + col_ld);
        }
#pragma unroll
        for (int w = 0; w < kU; ++w) {
          if (j + w < m) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = acc[v] + val[w][v];
          }
        }
      }
    }
    if (col_ok) *reinterpret_cast<vec_t*>(out + col) = acc;
  }
}

// G lanes own the window of sorted positions [kWindow w, kWindow w + kWindow): at most one of them heads a run of more
// than one chunk.  That run's partial sums lie in consecutive slots; ug_out[u] = +0.0f plus them in ascending chunk.
template <int G, int VEC>
__global__ __launch_bounds__(256) void glx_emb_combine_kernel(CoalesceArgs a) {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  const int64_t w = blockIdx.x * (int64_t)(256 / G) + threadIdx.x / G;
  const int c = threadIdx.x & (G - 1);
  const int64_t first = w * kWindow;
  if (first >= a.n) return;  // whole groups leave
  int32_t found = -1;
  for (int32_t t = c; t < kWindow; t += G) {
    const int64_t i = first + t;
    if (i < a.n) {
      const uint64_t f = a.scan[i] - (i > 0 ? a.scan[i - 1] : 0);
      if ((f & kHead) && (f & kMulti)) found = (int32_t)i;
    }
  }
#pragma unroll
  for (int off = G >> 1; off > 0; off >>= 1) {
    const int32_t o = __shfl_xor(found, off, G);
    found = o > found ? o : found;
  }
  if (found < 0) return;  // the same in every lane of the group
  const int32_t i = found;
  const uint64_t here = a.scan[i];
  const uint32_t key = a.keys[i];
  const int32_t u = (int32_t)(uint32_t)here - 1;
  const int64_t slot0 = (int64_t)((int32_t)(here >> 32) - 1);
  int32_t chunks = 1;  // chunk k exists when position i + k kChunk still carries the key
  while ((int64_t)i + (int64_t)chunks * kChunk < a.n && a.keys[i + chunks * kChunk] == key) ++chunks;
  float* const out = a.ug + (int64_t)u * a.dim;
  for (int32_t col_pass = 0; col_pass < a.dim; col_pass += G * VEC) {
    const int32_t col = col_pass + c * VEC;
    if (col >= a.dim) continue;
    vec_t acc;
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.0f;
    for (int32_t k = 0; k < chunks; k += kU) {
      vec_t val[kU];
#pragma unroll
      for (int x = 0; x < kU; ++x) {
        if (k + x < chunks) val[x] = *reinterpret_cast<const vec_t*>(a.partial + (slot0 + k + x) * a.dim + col);
      }
#pragma unroll
      for (int x = 0; x < kU; ++x) {
        if (k + x < chunks) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[v] = acc[v] + val[x][v];
        }
      }
    }
    *reinterpret_cast<vec_t*>(out + col) = acc;
  }
}

template <int VEC>
void launch_coalesce_vec(const CoalesceArgs& a, hipStream_t s) {
  const int G = glx_group_for((a.dim + VEC - 1) / VEC);
  const unsigned blocks = (unsigned)(((int64_t)a.n + (256 / G) - 1) / (256 / G));
  const int64_t windows = ((int64_t)a.n + kWindow - 1) / kWindow;
  const unsigned cblocks = (unsigned)((windows + (256 / G) - 1) / (256 / G));
  glx_for_group(G, [&](auto g) {
    glx_emb_reduce_kernel<decltype(g)::value, VEC><<<blocks, 256, 0, s>>>(a);
    glx_emb_combine_kernel<decltype(g)::value, VEC><<<cblocks, 256, 0, s>>>(a);
  });
}

// Device pointers only, device selected; n >= 1.
int coalesce_device(const int64_t* rows, int32_t n, int64_t num_rows, int32_t dim, const float* g, int64_t* urows,
                    float* ug, int64_t* num_unique, hipStream_t s) {
  int bits = 1;
  while (bits < 32 && ((uint64_t)1 << bits) <= (uint64_t)num_rows) ++bits;  // the sentinel key num_rows fits
  uint32_t* const no_keys = nullptr;
  int32_t* const no_vals = nullptr;
  uint64_t* const no_flags = nullptr;
  size_t sort_tmp = 0, scan_tmp = 0;
  GLX_HIP(rocprim::radix_sort_pairs(nullptr, sort_tmp, no_keys, no_keys, no_vals, no_vals, (size_t)n, 0, bits, s));
  GLX_HIP(rocprim::inclusive_scan(nullptr, scan_tmp, no_flags, no_flags, (size_t)n, rocprim::plus<uint64_t>(), s));
  const size_t tmp_b = glx_align256(sort_tmp > scan_tmp ? sort_tmp : scan_tmp);
  const size_t ids_b = glx_align256((size_t)n * sizeof(int32_t));
  const size_t flag_b = glx_align256((size_t)n * sizeof(uint64_t));
  // a run of L > kChunk entries has ceil(L / kChunk) < L / (kChunk / 2) chunks: at most n / (kChunk / 2) slots
  const size_t part_b = glx_align256(((size_t)n / (kChunk / 2) + 1) * dim * sizeof(float));
  GlxScratch lease;
  int rc = lease.alloc(tmp_b + 4 * ids_b + 2 * flag_b + part_b, s, 1);
  if (rc != GLX_OK) return rc;
  char* at = lease.as<char>();
  void* tmp = at;
  at += tmp_b;
  uint32_t* keys = reinterpret_cast<uint32_t*>(at);
  uint32_t* keys_s = reinterpret_cast<uint32_t*>(at + ids_b);
  int32_t* vals = reinterpret_cast<int32_t*>(at + 2 * ids_b);
  int32_t* vals_s = reinterpret_cast<int32_t*>(at + 3 * ids_b);
  at += 4 * ids_b;
  uint64_t* flags = reinterpret_cast<uint64_t*>(at);
  uint64_t* scan = reinterpret_cast<uint64_t*>(at + flag_b);
  at += 2 * flag_b;
  const unsigned nblocks = (unsigned)(((int64_t)n + 255) / 256);
  glx_emb_keys_kernel<<<nblocks, 256, 0, s>>>(rows, n, num_rows, keys, vals);
  GLX_HIP(rocprim::radix_sort_pairs(tmp, sort_tmp, keys, keys_s, vals, vals_s, (size_t)n, 0, bits, s));
  glx_emb_flags_kernel<<<nblocks, 256, 0, s>>>(keys_s, n, (uint32_t)num_rows, flags);
  GLX_HIP(rocprim::inclusive_scan(tmp, scan_tmp, flags, scan, (size_t)n, rocprim::plus<uint64_t>(), s));
  CoalesceArgs a;
  a.keys = keys_s;
  a.pos = vals_s;
  a.scan = scan;
  a.g = g;
  a.ug = ug;
  a.partial = reinterpret_cast<float*>(at);
  a.urows = urows;
  a.num_unique = num_unique;
  a.n = n;
  a.dim = dim;
  if (dim % 4 == 0 && glx_aligned16(g) && glx_aligned16(ug)) launch_coalesce_vec<4>(a, s);
  else launch_coalesce_vec<1>(a, s);
  GLX_HIP(hipGetLastError());
  return GLX_OK;
}

// ---- the optimizer steps -------------------------------------------------------------------------------------------
struct UpdateArgs {
  float* W;
  float* s1;
  float* s2;
  const int64_t* urows;
  const float* ug;
  int64_t num_rows;
  int32_t dim, n;
  float alpha, eps, beta1, c1, beta2, c2;
};

// G lanes own entry u; lane c owns columns [VEC c, VEC c + VEC) of each column tile.  Every row is read once and each
// written row written once.  Every float operation below is one rounding: the build forbids contraction, the products
// pass through `glx_pin` besides, and the divide and the square root are the correctly rounded ones.
template <int ALGO, int G, int VEC>
__global__ __launch_bounds__(256) void glx_emb_update_kernel(UpdateArgs a) {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  const int64_t u = blockIdx.x * (int64_t)(256 / G) + threadIdx.x / G;
  const int c = threadIdx.x & (G - 1);
  if (u >= a.n) return;  // whole groups leave
  const int64_t r = a.urows[u];
  if (r < 0 || r >= a.num_rows) return;  // the -1 tail of a coalesce, or any other entry outside the table
  const int64_t at = r * (int64_t)a.dim;
  const float* const gr = a.ug + u * (int64_t)a.dim;
  for (int32_t col = c * VEC; col < a.dim; col += G * VEC) {
    const vec_t g = *reinterpret_cast<const vec_t*>(gr + col);
    vec_t w = *reinterpret_cast<const vec_t*>(a.W + at + col);
    if (ALGO == GLX_EMB_SGD) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) w[v] = w[v] - glx_pin(a.alpha * g[v]);
    } else if (ALGO == GLX_EMB_ADAGRAD) {
      vec_t st = *reinterpret_cast<const vec_t*>(a.s1 + at + col);
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        st[v] = glx_fold_rn(st[v], g[v], g[v]);
        const float den = glx_pin(sqrtf(st[v])) + a.eps;
        const float q = glx_pin(g[v] / den);
        w[v] = w[v] - glx_pin(a.alpha * q);
      }
      *reinterpret_cast<vec_t*>(a.s1 + at + col) = st;
    } else {
      vec_t m = *reinterpret_cast<const vec_t*>(a.s1 + at + col);
      vec_t sv = *reinterpret_cast<const vec_t*>(a.s2 + at + col);
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        m[v] = glx_pin(a.beta1 * m[v]) + glx_pin(a.c1 * g[v]);
        const float gg = glx_pin(g[v] * g[v]);
        sv[v] = glx_pin(a.beta2 * sv[v]) + glx_pin(a.c2 * gg);
        const float den = glx_pin(sqrtf(sv[v])) + a.eps;
        const float q = glx_pin(m[v] / den);
        w[v] = w[v] - glx_pin(a.alpha * q);
      }
      *reinterpret_cast<vec_t*>(a.s1 + at + col) = m;
      *reinterpret_cast<vec_t*>(a.s2 + at + col) = sv;
    }
    *reinterpret_cast<vec_t*>(a.W + at + col) = w;
  }
}

template <int ALGO, int VEC>
void launch_update_vec(const UpdateArgs& a, hipStream_t s) {
  const int G = glx_group_for((a.dim + VEC - 1) / VEC);
  const unsigned blocks = (unsigned)(((int64_t)a.n + (256 / G) - 1) / (256 / G));
  glx_for_group(G, [&](auto g) { glx_emb_update_kernel<ALGO, decltype(g)::value, VEC><<<blocks, 256, 0, s>>>(a); });
}

template <int ALGO>
void launch_update(const UpdateArgs& a, hipStream_t s) {
  const bool vec4 =
      a.dim % 4 == 0 && glx_aligned16(a.W) && glx_aligned16(a.ug) && glx_aligned16(a.s1) && glx_aligned16(a.s2);
  if (vec4) launch_update_vec<ALGO, 4>(a, s);
  else launch_update_vec<ALGO, 1>(a, s);
}

}  // namespace

extern "C" int glx_rows_coalesce(int device, const int64_t* rows, int32_t n, int64_t num_rows, int32_t dim, const float* g,
                                 int64_t* urows_out, float* ug_out, int64_t* num_unique_out, int ptr_kind, void* stream) {
  GLX_REQUIRE(n >= 0 && num_rows >= 0, "negative sizes: n %d, num_rows %lld", n, (long long)num_rows);
  GLX_REQUIRE(dim > 0, "dim must be positive, got %d", dim);
  GLX_REQUIRE(num_rows < INT32_MAX, "num_rows must be < 2^31");
  GLX_REQUIRE((int64_t)n * dim <= INT32_MAX, "n * dim exceeds int32");
  GLX_REQUIRE(ptr_kind == GLX_PTR_HOST || ptr_kind == GLX_PTR_DEVICE, "bad ptr_kind");
  GLX_REQUIRE(n == 0 || rows != nullptr, "rows is NULL");
  GLX_REQUIRE(n == 0 || g != nullptr, "g is NULL");
  GLX_REQUIRE(n == 0 || urows_out != nullptr, "urows_out is NULL");
  GLX_REQUIRE(n == 0 || ug_out != nullptr, "ug_out is NULL");
  GLX_REQUIRE(num_unique_out != nullptr, "num_unique_out is NULL");
  int rc = glx_init_device(device);
  if (rc != GLX_OK) return rc;
  GlxDeviceGuard guard(device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", device);
  GlxHostStage st(device, ptr_kind, stream, GlxHostStage::ADMIT);
  const int64_t* d_rows;
  const float* d_g;
  const float* d_ug_before = nullptr;
  int64_t *d_urows, *d_count;
  float* d_ug;
  st.in(&d_rows, rows, (size_t)n);
  st.in(&d_g, g, (size_t)n * dim);
  // rows of ug_out from U on are not written: a staged host buffer takes its present contents along
  if (st.host) st.in(&d_ug_before, static_cast<const float*>(ug_out), (size_t)n * dim);
  st.out(&d_urows, urows_out, (size_t)n);
  st.out(&d_ug, ug_out, (size_t)n * dim);
  st.out(&d_count, num_unique_out, (size_t)1);
  rc = st.begin();
  if (rc == GLX_OK) {
    hipError_t e = hipSuccess;
    if (n == 0) {
      e = hipMemsetAsync(d_count, 0, sizeof(int64_t), st.s);
    } else if (st.host) {
      e = hipMemcpyAsync(d_ug, d_ug_before, (size_t)n * dim * sizeof(float), hipMemcpyDeviceToDevice, st.s);
    }
    if (e != hipSuccess) {
      glx_set_error("glx_rows_coalesce: %s", hipGetErrorString(e));
      rc = GLX_INTERNAL;
    } else if (n > 0) {
      rc = coalesce_device(d_rows, n, num_rows, dim, d_g, d_urows, d_ug, d_count, st.s);
    }
  }
  return st.finish(rc);
}

extern "C" int glx_embedding_update(int device, int algo, float* W, float* state1, float* state2, int64_t num_rows,
                                    int32_t dim, const int64_t* urows, const float* ug, int32_t n, float alpha, float eps,
                                    float beta1, float c1, float beta2, float c2, void* stream) {
  GLX_REQUIRE(algo == GLX_EMB_SGD || algo == GLX_EMB_ADAGRAD || algo == GLX_EMB_ADAM, "unknown algo %d", algo);
  GLX_REQUIRE(n >= 0 && num_rows >= 0, "negative sizes: n %d, num_rows %lld", n, (long long)num_rows);
  GLX_REQUIRE(dim > 0, "dim must be positive, got %d", dim);
  GLX_REQUIRE(num_rows < INT32_MAX, "num_rows must be < 2^31");
  GLX_REQUIRE((int64_t)n * dim <= INT32_MAX, "n * dim exceeds int32");
  GLX_REQUIRE(num_rows == 0 || W != nullptr, "W is NULL");
  GLX_REQUIRE(n == 0 || urows != nullptr, "urows is NULL");
  GLX_REQUIRE(n == 0 || ug != nullptr, "ug is NULL");
  if (algo == GLX_EMB_SGD) {
    GLX_REQUIRE(state1 == nullptr && state2 == nullptr, "SGD keeps no state: state1 and state2 must be NULL");
  } else if (algo == GLX_EMB_ADAGRAD) {
    GLX_REQUIRE(num_rows == 0 || state1 != nullptr, "state1 is NULL: Adagrad needs its accumulator");
    GLX_REQUIRE(state2 == nullptr, "Adagrad keeps one state table: state2 must be NULL");
  } else {
    GLX_REQUIRE(num_rows == 0 || state1 != nullptr, "state1 is NULL: Adam needs its first moment");
    GLX_REQUIRE(num_rows == 0 || state2 != nullptr, "state2 is NULL: Adam needs its second moment");
  }
  int rc = glx_init_device(device);
  if (rc != GLX_OK) return rc;
  if (n == 0 || num_rows == 0) return GLX_OK;
  GlxDeviceGuard guard(device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", device);
  UpdateArgs a;
  a.W = W;
  a.s1 = state1;
  a.s2 = state2;
  a.urows = urows;
  a.ug = ug;
  a.num_rows = num_rows;
  a.dim = dim;
  a.n = n;
  a.alpha = alpha;
  a.eps = eps;
  a.beta1 = beta1;
  a.c1 = c1;
  a.beta2 = beta2;
  a.c2 = c2;
  hipStream_t s = glx_stream(stream);
  if (algo == GLX_EMB_SGD) launch_update<GLX_EMB_SGD>(a, s);
  else if (algo == GLX_EMB_ADAGRAD) launch_update<GLX_EMB_ADAGRAD>(a, s);
  else launch_update<GLX_EMB_ADAM>(a, s);
  GLX_HIP(hipGetLastError());
  return GLX_OK;
}
