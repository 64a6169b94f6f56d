// glx pair scores: the per-pair, optionally multi-head, dot product of two gathered rows, with its gradients with
// respect to both tables.  The reference's unsupervised models score an edge as the dot product of its two endpoint
// embeddings, against sampled negatives (examples/tf/sage/train.py:56-57, examples/tf/bipartite_sage/train.py:59-60,
// examples/tf/ultra_gcn/ultra_gcn.py:92-95, python/nn/tf/loss.py:58).
//
// Contract (include/glx.h).  xa[num_rows_a, dim], xb[num_rows_b, dim] float32 (they may be one
// table), C = dim / heads, column c belongs to head c / C.  ia[num_pairs / repeat], ib[num_pairs] int64: pair p joins
// row ia[p / repeat] of xa with row ib[p] of xb -- repeat = K scores a [B, K] negative-sampler response against its B
// sources.  An index outside its table reads a row of default_attr.
//   forward    out[p, h] = sum over the columns c of head h of xa_row(p)[c] * xb_row(p)[c]; one lane group per pair, a
//              lane-to-column mapping and a cross-lane tree fixed by (dim, heads, alignment) alone: the same bits on
//              every call, checked against a bound (the order over the columns is the mapping's)
//   backward   side 0 (xa): grad[r, c] = +0.0f, then for each pair p with ia[p / repeat] == r in ascending p
//              fadd_rn(., fmul_rn(g[p, head(c)], xb_row(p)[c])); side 1 (xb): pairs with ib[p] == r, factor xa_row(p)[c].
//              An own index outside the table receives nothing.  Bit-exact.
// No float atomics anywhere.
//
// The tables are float32 or bfloat16, both of one type (the _ex entry points).  bfloat16 rows are upcast
// as they are loaded -- exact -- so out stays float32 and equals the float32 call on the upcast tables bit for bit (the
// same VEC, plan and tree); a bfloat16 grad_self is the float32 sum above rounded once per element, to nearest even
// (glx_f32_to_bf16_bits), in the kernel's final store.  g and out are always float32.
#include "glx_lane_groups.h"

// Two roundings per term of the backward: glx_fold_rn (glx_lane_groups.h) pins the product; the pragma is for the
// front end.
#pragma clang fp contract(off)

namespace {

constexpr int kWU = 4;  // row loads in flight per lane

// ---- forward -----------------------------------------------------------------------------------------------
struct PairFwdArgs {
  const void* xa;      // [num_rows_a, dim] of `dtype` elements
  const void* xb;      // [num_rows_b, dim] of `dtype` elements
  int dtype;           // GLX_DTYPE_F32 or GLX_DTYPE_BF16, of both tables
  const int64_t* ia;   // [num_pairs / repeat]
  const int64_t* ib;   // [num_pairs]
  float* out;          // [num_pairs, heads]
  int64_t num_rows_a, num_rows_b;
  int32_t dim, heads, C, num_pairs, repeat;
  GlxHeadDots hd;
  float default_attr;
};

// G lanes own one PAIR p and write out[p, 0 .. heads): glx_head_dots (glx_lane_groups.h) of the pair's two rows.
// The `repeat` pairs of one source are neighbouring groups of a workgroup: the shared row comes out of the L1 / L2.
// bfloat16 tables are upcast as they are loaded: the same products in the same tree.
template <int G, int VEC, bool SUB, int DT>
__global__ __launch_bounds__(256) void glx_pair_dot_kernel(PairFwdArgs a) {
  typedef typename AggElem<DT>::raw raw_t;
  const int64_t p = blockIdx.x * (int64_t)(256 / G) + threadIdx.x / G;
  const int c = threadIdx.x & (G - 1);
  if (p >= a.num_pairs) return;  // whole groups leave
  float* const out = a.out + p * (int64_t)a.heads;
  const int64_t ra = a.ia[p / a.repeat], rb = a.ib[p];
  const raw_t* const xa =
      (ra >= 0 && ra < a.num_rows_a) ? static_cast<const raw_t*>(a.xa) + ra * (int64_t)a.dim : nullptr;
  const raw_t* const xb =
      (rb >= 0 && rb < a.num_rows_b) ? static_cast<const raw_t*>(a.xb) + rb * (int64_t)a.dim : nullptr;
  // the null-pointer form, not glx_row: its clamped pointer costs this kernel up to two VGPRs
  const GlxRowOf<DT> rowa = {xa, xa != nullptr}, rowb = {xb, xb != nullptr};
  glx_head_dots<G, VEC, SUB, false>(rowa, rowb, a.default_attr, a.dim, a.heads, a.C, a.hd, 1.0f, c, out);
}

template <int VEC>
void launch_pair_fwd_vec(PairFwdArgs a, hipStream_t s) {
  const GlxHeadDotPlan plan = glx_head_dot_plan(a.dim, a.C, VEC);
  const int G = plan.G;
  a.hd = plan.hd;
  const unsigned blocks = (unsigned)(((int64_t)a.num_pairs + (256 / G) - 1) / (256 / G));
  glx_for_group(G, [&](auto g) {
    glx_for_train_dtype(a.dtype, [&](auto t) {
      constexpr int kG = decltype(g)::value, kDT = decltype(t)::value;
      if (plan.sub_groups) glx_pair_dot_kernel<kG, VEC, true, kDT><<<blocks, 256, 0, s>>>(a);
      else glx_pair_dot_kernel<kG, VEC, false, kDT><<<blocks, 256, 0, s>>>(a);
    });
  });
}

void launch_pair_fwd(const PairFwdArgs& a, hipStream_t s) {
  // the same VEC, and so the same plan and reduction tree, for bfloat16 tables as for the float32 ones of their values
  const bool vec4 =
      a.dim % 4 == 0 && a.C % 4 == 0 && glx_aligned_vec4(a.xa, a.dtype) && glx_aligned_vec4(a.xb, a.dtype);
  if (vec4) launch_pair_fwd_vec<4>(a, s);
  else launch_pair_fwd_vec<1>(a, s);
}

// ---- backward ----------------------------------------------------------------------------------------------
struct PairBwdArgs {
  GlxAggTranspose t;         // of the own side's index array: row r's entries are t.pos[t.row_ptr[r] .. t.row_ptr[r + 1])
  const int64_t* other_idx;  // the other side's index array
  const float* g;            // [num_pairs, heads]
  const void* x_other;       // [num_rows_other, dim] of `dtype` elements
  void* grad_self;           // [num_rows_self, dim] of `dtype` elements
  int dtype;                 // GLX_DTYPE_F32 or GLX_DTYPE_BF16, of both
  int64_t num_rows_self, num_rows_other;
  int32_t dim, heads, C;
  int32_t own_rep;    // pairs per entry of the own index array: repeat (side 0) or 1 (side 1)
  int32_t other_rep;  // pairs per entry of the other index array: 1 (side 0) or repeat (side 1)
  float default_attr;
};

// The sibling of K5-w's glx_row_grad_kernel (glx_chunks.h) with the factor's row gathered too: G lanes own table row r.
// Its list of own-side entries, each expanded to own_rep consecutive pairs, is one run of (l1 - l0) * own_rep pairs in
// ascending p (ascending entries give ascending pairs).  Lane c fetches pair base + c of the run (its number and the
// other side's row, already tested against the table), every lane reads entry j from lane j; kWU row loads and their
// g are issued before the first is folded.  Every row is written, an empty list writes zeros.  A bfloat16 x_other is
// upcast as it is loaded, the sum is float32, and a bfloat16 grad_self rounds the finished sum once, in the store.
template <int G, int VEC, int DT>
__global__ __launch_bounds__(256) void glx_pair_dot_bwd_kernel(PairBwdArgs a) {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  typedef typename AggElem<DT>::raw raw_t;
  const raw_t* __restrict__ x_other = static_cast<const raw_t*>(a.x_other);
  const int64_t r = blockIdx.x * (int64_t)(256 / G) + threadIdx.x / G;
  const int c = threadIdx.x & (G - 1);
  if (r >= a.num_rows_self) return;  // whole groups leave
  const int32_t l0 = a.t.row_ptr[r];
  const int32_t total = (a.t.row_ptr[r + 1] - l0) * a.own_rep;  // at most num_pairs
  raw_t* const out = static_cast<raw_t*>(a.grad_self) + r * (int64_t)a.dim;
  for (int32_t col_pass = 0; col_pass < a.dim; col_pass += G * VEC) {
    const int32_t col = col_pass + c * VEC;
    const bool col_ok = col < a.dim;
    const int32_t col_ld = col_ok ? col : 0;  // lanes past the end re-read the first columns, unused
    const int32_t head = col_ld / a.C;
    vec_t acc;
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.0f;
    for (int32_t base = 0; base < total; base += G) {
      int32_t my_p = 0, my_row = -1;
      if (base + c < total) {
        const int32_t e = base + c;
        my_p = a.t.pos[l0 + e / a.own_rep] * a.own_rep + e % a.own_rep;
        const int64_t o = a.other_idx[my_p / a.other_rep];
        my_row = (o >= 0 && o < a.num_rows_other) ? (int32_t)o : -1;
      }
      const int32_t m = (total - base) < G ? (total - base) : G;
      for (int32_t j = 0; j < m; j += kWU) {
        int32_t pr[kWU], row[kWU];
#pragma unroll
        for (int u = 0; u < kWU; ++u) {
          const int src = (j + u) & (G - 1);
          pr[u] = __shfl(my_p, src, G);
          row[u] = __shfl(my_row, src, G);
        }
        vec_t val[kWU];
        float gt[kWU];
#pragma unroll
        for (int u = 0; u < kWU; ++u) {
          if (j + u < m) {
            gt[u] = a.g[(int64_t)pr[u] * a.heads + head];
            if (row[u] >= 0) {
              val[u] = agg_load<DT, VEC>(x_other + row[u] * (int64_t)a.dim + col_ld);
            } else {
#pragma unroll
              for (int v = 0; v < VEC; ++v) val[u][v] = a.default_attr;
            }
          }
        }
#pragma unroll
        for (int u = 0; u < kWU; ++u) {
          if (j + u < m) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = glx_fold_rn(acc[v], gt[u], val[u][v]);
          }
        }
      }
    }
    if (col_ok) agg_store<DT, VEC>(out + col, acc);  // lanes past the last column store nothing
  }
}

template <int VEC>
void launch_pair_bwd_vec(const PairBwdArgs& a, hipStream_t s) {
  const int G = glx_group_for((a.dim + VEC - 1) / VEC);
  const unsigned blocks = (unsigned)((a.num_rows_self + (256 / G) - 1) / (256 / G));
  glx_for_group(G, [&](auto g) {
    glx_for_train_dtype(a.dtype, [&](auto t) {
      glx_pair_dot_bwd_kernel<decltype(g)::value, VEC, decltype(t)::value><<<blocks, 256, 0, s>>>(a);
    });
  });
}

void launch_pair_bwd(const PairBwdArgs& a, hipStream_t s) {
  const bool vec4 = a.dim % 4 == 0 && a.C % 4 == 0 && glx_aligned_vec4(a.x_other, a.dtype) &&
                    glx_aligned_vec4(a.grad_self, a.dtype);
  if (vec4) launch_pair_bwd_vec<4>(a, s);
  else launch_pair_bwd_vec<1>(a, s);
}

}  // namespace

// what the two entry points check alike, before any device use
#define GLX_PAIR_REQUIRE()                                                                                              \
  GLX_REQUIRE(num_pairs >= 0, "negative sizes: num_pairs %d", num_pairs);                                               \
  GLX_REQUIRE(dim > 0, "dim must be positive, got %d", dim);                                                            \
  GLX_REQUIRE(heads > 0, "heads must be positive, got %d", heads);                                                      \
  GLX_REQUIRE(dim % heads == 0, "dim %d is not a multiple of heads %d", dim, heads);                                    \
  GLX_REQUIRE(repeat >= 1, "repeat must be at least 1, got %d", repeat);                                                \
  GLX_REQUIRE(num_pairs % repeat == 0, "num_pairs %d is not a multiple of repeat %d", num_pairs, repeat);               \
  GLX_REQUIRE((int64_t)num_pairs * heads <= INT32_MAX, "num_pairs * heads exceeds int32");                              \
  GLX_REQUIRE(ptr_kind == GLX_PTR_HOST || ptr_kind == GLX_PTR_DEVICE, "bad ptr_kind")

extern "C" int glx_pair_dot_ex(int device, const void* xa, int64_t num_rows_a, const void* xb, int64_t num_rows_b,
                               int x_dtype, int32_t dim, int32_t heads, const int64_t* ia, const int64_t* ib,
                               int32_t num_pairs, int32_t repeat, float default_attr, float* out, int ptr_kind,
                               void* stream) {
  GLX_REQUIRE_TRAIN_DTYPE(x_dtype, "glx_pair_dot_ex: x_dtype");
  GLX_PAIR_REQUIRE();
  GLX_REQUIRE(num_rows_a >= 0 && num_rows_b >= 0, "negative sizes: num_rows");
  GLX_REQUIRE(num_rows_a < INT32_MAX && num_rows_b < INT32_MAX, "num_rows must be < 2^31");
  GLX_REQUIRE(num_rows_a == 0 || xa != nullptr, "xa is NULL");
  GLX_REQUIRE(num_rows_b == 0 || xb != nullptr, "xb is NULL");
  GLX_REQUIRE(num_pairs == 0 || ia != nullptr, "ia is NULL");
  GLX_REQUIRE(num_pairs == 0 || ib != nullptr, "ib is NULL");
  GLX_REQUIRE(num_pairs == 0 || out != nullptr, "out is NULL");
  int rc = glx_init_device(device);
  if (rc != GLX_OK) return rc;
  if (num_pairs == 0) return GLX_OK;
  GlxDeviceGuard guard(device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", device);
  GlxHostStage st(device, ptr_kind, stream, GlxHostStage::ADMIT);
  PairFwdArgs a;
  a.dtype = x_dtype;
  st.in_bytes(&a.xa, xa, (size_t)num_rows_a * dim * (size_t)glx_dtype_size(x_dtype));
  st.in_bytes(&a.xb, xb, (size_t)num_rows_b * dim * (size_t)glx_dtype_size(x_dtype));
  st.in(&a.ia, ia, (size_t)(num_pairs / repeat));
  st.in(&a.ib, ib, (size_t)num_pairs);
  st.out(&a.out, out, (size_t)num_pairs * heads);
  rc = st.begin();
  if (rc == GLX_OK) {
    a.num_rows_a = num_rows_a;
    a.num_rows_b = num_rows_b;
    a.dim = dim;
    a.heads = heads;
    a.C = dim / heads;
    a.num_pairs = num_pairs;
    a.repeat = repeat;
    a.default_attr = default_attr;
    launch_pair_fwd(a, st.s);
  }
  return st.finish(rc);
}

extern "C" int glx_pair_dot(int device, const float* xa, int64_t num_rows_a, const float* xb, int64_t num_rows_b,
                            int32_t dim, int32_t heads, const int64_t* ia, const int64_t* ib, int32_t num_pairs,
                            int32_t repeat, float default_attr, float* out, int ptr_kind, void* stream) {
  return glx_pair_dot_ex(device, xa, num_rows_a, xb, num_rows_b, GLX_DTYPE_F32, dim, heads, ia, ib, num_pairs, repeat,
                         default_attr, out, ptr_kind, stream);
}

extern "C" int glx_pair_dot_backward_ex(int device, int side, const int64_t* ia, const int64_t* ib, int32_t num_pairs,
                                        int32_t repeat, const float* g, int32_t heads, const void* x_other,
                                        int64_t num_rows_other, int32_t dim, int64_t num_rows_self,
                                        float default_attr, void* grad_self, int x_dtype, int ptr_kind,
                                        void* stream) {
  GLX_REQUIRE_TRAIN_DTYPE(x_dtype, "glx_pair_dot_backward_ex: x_dtype");
  GLX_PAIR_REQUIRE();
  GLX_REQUIRE(side == 0 || side == 1, "side must be 0 (xa) or 1 (xb), got %d", side);
  GLX_REQUIRE(num_rows_other >= 0 && num_rows_self >= 0, "negative sizes: num_rows");
  GLX_REQUIRE(num_rows_other < INT32_MAX && num_rows_self < INT32_MAX, "num_rows must be < 2^31");
  GLX_REQUIRE(num_pairs == 0 || ia != nullptr, "ia is NULL");
  GLX_REQUIRE(num_pairs == 0 || ib != nullptr, "ib is NULL");
  GLX_REQUIRE(num_pairs == 0 || g != nullptr, "g is NULL");
  GLX_REQUIRE(num_rows_other == 0 || x_other != nullptr, "x_other is NULL");
  GLX_REQUIRE(num_rows_self == 0 || grad_self != nullptr, "grad_self is NULL");
  int rc = glx_init_device(device);
  if (rc != GLX_OK) return rc;
  if (num_rows_self == 0) return GLX_OK;
  GlxDeviceGuard guard(device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", device);
  GlxHostStage st(device, ptr_kind, stream, GlxHostStage::ADMIT);
  const int64_t* d_ia;
  const int64_t* d_ib;
  PairBwdArgs a;
  a.dtype = x_dtype;
  const size_t elem = (size_t)glx_dtype_size(x_dtype);
  st.in(&d_ia, ia, (size_t)(num_pairs / repeat));
  st.in(&d_ib, ib, (size_t)num_pairs);
  st.in(&a.g, g, (size_t)num_pairs * heads);
  st.in_bytes(&a.x_other, x_other, (size_t)num_rows_other * dim * elem);
  st.out_bytes(&a.grad_self, grad_self, (size_t)num_rows_self * dim * elem);
  rc = st.begin();
  GlxScratch lease;
  if (rc == GLX_OK) {
    if (num_pairs == 0) {  // no pair: every row is zeros
      rc = glx_zero_elems_async(a.grad_self, (size_t)num_rows_self * dim, x_dtype, st.s);
    } else {
      // one position per segment; side 0 sorts the num_pairs / repeat entries of ia only
      const int32_t own_n = side == 0 ? num_pairs / repeat : num_pairs;
      rc = glx_agg_transpose(side == 0 ? d_ia : d_ib, nullptr, own_n, own_n, num_rows_self, st.s, &lease, &a.t);
      if (rc == GLX_OK) {
        a.other_idx = side == 0 ? d_ib : d_ia;
        a.num_rows_self = num_rows_self;
        a.num_rows_other = num_rows_other;
        a.dim = dim;
        a.heads = heads;
        a.C = dim / heads;
        a.own_rep = side == 0 ? repeat : 1;
        a.other_rep = side == 0 ? 1 : repeat;
        a.default_attr = default_attr;
        launch_pair_bwd(a, st.s);
      }
    }
  }
  return st.finish(rc);
}

extern "C" int glx_pair_dot_backward(int device, int side, const int64_t* ia, const int64_t* ib, int32_t num_pairs,
                                     int32_t repeat, const float* g, int32_t heads, const float* x_other,
                                     int64_t num_rows_other, int32_t dim, int64_t num_rows_self, float default_attr,
                                     float* grad_self, int ptr_kind, void* stream) {
  return glx_pair_dot_backward_ex(device, side, ia, ib, num_pairs, repeat, g, heads, x_other, num_rows_other, dim,
                                  num_rows_self, default_attr, grad_self, GLX_DTYPE_F32, ptr_kind, stream);
}
