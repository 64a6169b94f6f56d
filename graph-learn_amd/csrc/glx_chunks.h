// The CHUNKED order of the training path's deterministic sums: a
// list of more than GLX_COALESCE_CHUNK entries is LONG and is cut into chunks of that many entries; a chunk's partial
// is +0.0f plus its terms in ascending entry, the list's sum +0.0f plus its partials in ascending chunk.  Every other
// list is short, has no chunk, and keeps the default order's bits.  This header is the one place that knows
//   the lists        GlxRowLists (a table row's transposed list of positions), GlxSegLists (a segment's positions)
//   the directory    GlxChunkDir, built on the device by glx_chunk_dir: one scan, one search per work item; neither the
//                    number of long lists nor of chunks reaches the host
//   a chunk          GLX_CHUNK_IDLE: work item t is past the directory; glx_chunk_of: t is entries [c0, c1) of its
//                    list; GLX_CHUNK_FIRST: t opens its list
//   the row gradient glx_row_grad_launch and its kernel pair, shared by glx_aggregate_grad.hip and
//                    glx_aggregate_weighted.hip, which differ in their term alone
//   the combine      glx_chunks_combine: one lane group per long list adds its partial sums in order
//   the workspace    GlxTrainSlot: who holds which slot while a nested call leases another
#ifndef GLX_CHUNKS_H_
#define GLX_CHUNKS_H_
#include "glx_prims.h"
#include "glx_segment_lanes.h"

constexpr int kGlxChunk = GLX_COALESCE_CHUNK;

// The workspace slots (GlxScratch, glx_common.h) of the training path.  A slot has one lease at a time, so a call that
// leases inside another call's lease needs a slot of its own: each line says who holds the slot, and for how long.
enum GlxTrainSlot {
  kSlotRequest = 1,       // the request's transpose or segment ends: the entry point, for its whole body
  kSlotRowChunks = 2,     // the row directory and its partial sums: the chunked row gradient, inside glx_weighted_bwd_x
                          // or the aggregate backward
  kSlotAlpha = 2,         // the same slot: dot attention's alpha in the default order, whose row gradients lease none
  kSlotChunkScan = 3,     // the temporary of glx_chunk_dir's scan: given back before the builder returns
  kSlotAlphaChunked = 4,  // dot attention's alpha in the chunked order: read across the chunked glx_weighted_bwd_x
  kSlotSegChunks = 5,     // the segment directory and its partial sums: chunked dot attention, across its launches
};

// What a list is: entries [*begin, *end) of list i.
struct GlxRowLists {
  const int32_t* row_ptr;  // GlxAggTranspose's: [num_rows + 1] into pos
  __device__ __forceinline__ void bounds(int64_t i, int32_t* begin, int32_t* end) const {
    *begin = row_ptr[i];
    *end = row_ptr[i + 1];
  }
};
struct GlxSegLists {
  GlxSegLayout seg;  // the consumed positions of a segment
  __device__ __forceinline__ void bounds(int64_t i, int32_t* begin, int32_t* end) const {
    seg_bounds(seg, i, begin, end);
  }
};

// The chunk directory of one request's lists.  A long list of L entries has fewer than L / (GLX_COALESCE_CHUNK / 2)
// chunks, so n / (GLX_COALESCE_CHUNK / 2) + 1 work items and partial-sum rows hold every request of n entries; the
// launches cover max_items and idle work items leave when slot0 says so.  A kernel argument.
struct GlxChunkDir {
  const int32_t* slot0;      // [num_lists + 1] exclusive scan of the lists' chunk counts: list i's first work item /
                             // partial slot; slot0[num_lists] = the number of work items
  const int32_t* item_list;  // [max_items] the list of work item t; its chunk is t - slot0[list]
  float* partial;            // [max_items, dim] partial sum of work item t
  int64_t num_lists;
  int32_t max_items;         // n / (GLX_COALESCE_CHUNK / 2) + 1
};

// chunks of list i: ceil(entries / kGlxChunk) for a long list, none otherwise (and none for the extra element
// num_lists, which makes the exclusive scan end with the total)
template <typename LISTS>
struct GlxChunkCount {
  LISTS lists;
  int64_t num_lists;
  __device__ int32_t operator()(int64_t i) const {
    if (i >= num_lists) return 0;
    int32_t begin, end;
    lists.bounds(i, &begin, &end);
    return end - begin > kGlxChunk ? (end - begin + kGlxChunk - 1) / kGlxChunk : 0;
  }
};

// item_list[t] = the last list whose first slot is at or below t, for every work item of the directory
// (glx_aggregate_grad.hip)
void glx_chunk_items(const int32_t* slot0, int64_t num_lists, int32_t max_items, int32_t* item_list, hipStream_t s);

// The directory and the partial sums of `num_lists` lists of n entries in all, in one lease of workspace `slot`, valid
// for work queued on `s` until the lease ends.  `what` names the scan in an error's text.
template <typename LISTS>
int glx_chunk_dir(const LISTS& lists, int64_t num_lists, int32_t n, int32_t dim, int slot, const char* what,
                  hipStream_t s, GlxScratch* lease, GlxChunkDir* out) {
  const int32_t max_items = n / (kGlxChunk / 2) + 1;
  const size_t slot_b = glx_align256((size_t)(num_lists + 1) * sizeof(int32_t));
  const size_t item_b = glx_align256((size_t)max_items * sizeof(int32_t));
  const size_t part_b = (size_t)max_items * dim * sizeof(float);
  const int rc = lease->alloc(slot_b + item_b + part_b, s, slot);
  if (rc != GLX_OK) return rc;
  char* const at = lease->as<char>();
  int32_t* const slot0 = reinterpret_cast<int32_t*>(at);
  int32_t* const item_list = reinterpret_cast<int32_t*>(at + slot_b);
  const auto counts = rocprim::make_transform_iterator(rocprim::counting_iterator<int64_t>(0),
                                                       GlxChunkCount<LISTS>{lists, num_lists});
  GLX_TRY(glx_prim_leased(s, kSlotChunkScan, what, [&](void* tmp, size_t& bytes) {
    return rocprim::exclusive_scan(tmp, bytes, counts, slot0, (int32_t)0, (size_t)(num_lists + 1),
                                   rocprim::plus<int32_t>(), s);
  }));
  glx_chunk_items(slot0, num_lists, max_items, item_list, s);
  *out = GlxChunkDir{slot0, item_list, reinterpret_cast<float*>(at + slot_b + item_b), num_lists, max_items};
  return GLX_OK;
}

// the row directory of a transpose, in slot kSlotRowChunks (glx_aggregate_grad.hip: the one instance of the builder
// over rows)
int glx_row_chunk_dir(const GlxAggTranspose& t, int32_t n, int64_t num_rows, int32_t dim, hipStream_t s,
                      GlxScratch* lease, GlxChunkDir* out);

// Is work item t past the directory?  The launches cover max_items, and whole groups leave here.  Every chunk kernel
// starts with `if (GLX_CHUNK_IDLE(ch, t)) return;`.  A macro and not a function: behind a __forceinline__ function,
// whether it takes the kernel's directory argument by reference, by value or as a member, the compiler schedules the
// kernels that follow the test differently from the same test spelled in the kernel -- other registers, other
// instruction order (profiles/chunked_order/isa.txt) -- and these kernels are held to the instructions they were
// measured with.  `d` and `t` are named more than once: pass plain variables.
#define GLX_CHUNK_IDLE(d, t) ((t) >= (d).max_items || (t) >= (d).slot0[(d).num_lists])

// the list of work item t (not idle) and the entries [*c0, *c1) of its chunk
template <typename LISTS>
__device__ __forceinline__ void glx_chunk_of(const GlxChunkDir& d, const LISTS& lists, int64_t t, int32_t* list,
                                             int32_t* c0, int32_t* c1) {
  *list = d.item_list[t];
  int32_t begin, end;
  lists.bounds(*list, &begin, &end);
  *c0 = begin + ((int32_t)t - d.slot0[*list]) * kGlxChunk;
  *c1 = end - *c0 > kGlxChunk ? *c0 + kGlxChunk : end;
}

// Is work item t of the directory the first of its list, `list` = d.item_list[t] -- the one that speaks for the whole
// list?  Its partial sums are slots [t, d.slot0[list + 1]).  A macro for GLX_CHUNK_IDLE's reason.
#define GLX_CHUNK_FIRST(d, t, list) ((d).slot0[list] == (t))

// One lane group per long list: out[list] = +0.0f plus the list's partial sums in ascending chunk, one fadd_rn each,
// stored as out_dtype elements (bfloat16: rounded once, here).  vec4: the 4-column mapping of the fold before it.
// (glx_aggregate_grad.hip)
void glx_chunks_combine(const GlxChunkDir& ch, void* out, int out_dtype, int32_t dim, bool vec4, hipStream_t s);

// ---- the gradient with respect to the table rows ------------------------------------------------------------------
// One request, REQ, says what the two kernels and their launch need and nothing else:
//   REQ::kU            term loads in flight per lane
//   row_ptr()          the transpose's row_ptr; list() its GlxPosList
//   num_rows(), dim(), grad_x(), dtype()     grad_x[num_rows, dim] of dtype elements
//   term<VEC>(col)     the term of one column tile (glx_list_fold, glx_lane_groups.h)

// G lanes own table row r and walk its whole list (glx_list_fold): the ascending-position order.  Every row is
// written, an empty list writes zeros.  SHORT (the chunked order): a long row is left to the chunk and combine kernels;
// every other row gets exactly what the default order gives it.
template <typename REQ, int G, int VEC, int DT, bool SHORT>
__global__ __launch_bounds__(256) void glx_row_grad_kernel(REQ q) {
  typedef typename AggElem<DT>::raw raw_t;
  const int64_t r = blockIdx.x * (int64_t)(256 / G) + threadIdx.x / G;
  const int c = threadIdx.x & (G - 1);
  if (r >= q.num_rows()) return;  // whole groups leave
  int32_t l0, l1;
  GlxRowLists{q.row_ptr()}.bounds(r, &l0, &l1);
  if (SHORT && l1 - l0 > kGlxChunk) return;
  raw_t* const out = static_cast<raw_t*>(q.grad_x()) + r * (int64_t)q.dim();
  glx_list_fold<G, VEC, REQ::kU, DT>(q.list(), l0, l1, c, q.dim(), out,
                                     [&](int32_t col) { return q.template term<VEC>(col); });
}

// G lanes own work item t of the row directory: one chunk of a long row, folded by the same walk into the item's
// float32 partial sum.  Whole groups leave past the directory.
template <typename REQ, int G, int VEC>
__global__ __launch_bounds__(256) void glx_row_grad_chunk_kernel(REQ q, GlxChunkDir ch) {
  const int64_t t = blockIdx.x * (int64_t)(256 / G) + threadIdx.x / G;
  const int c = threadIdx.x & (G - 1);
  if (GLX_CHUNK_IDLE(ch, t)) return;
  int32_t r, l0, l1;
  glx_chunk_of(ch, GlxRowLists{q.row_ptr()}, t, &r, &l0, &l1);
  glx_list_fold<G, VEC, REQ::kU, GLX_DTYPE_F32>(q.list(), l0, l1, c, q.dim(), ch.partial + t * (int64_t)q.dim(),
                                                [&](int32_t col) { return q.template term<VEC>(col); });
}

// ch == nullptr: the default order, one launch; otherwise the chunked one over that directory -- short rows, chunks,
// combine.  The smallest group that covers a row in one tile; rows wider than 64 lanes take column tiles.
template <int VEC, typename REQ>
void glx_row_grad_launch(const REQ& q, const GlxChunkDir* ch, hipStream_t s) {
  const int G = glx_group_for((q.dim() + VEC - 1) / VEC);
  const unsigned blocks = (unsigned)((q.num_rows() + (256 / G) - 1) / (256 / G));
  glx_for_group(G, [&](auto g) {
    constexpr int kG = decltype(g)::value;
    glx_for_train_dtype(q.dtype(), [&](auto t) {
      constexpr int kDT = decltype(t)::value;
      if (ch == nullptr) glx_row_grad_kernel<REQ, kG, VEC, kDT, false><<<blocks, 256, 0, s>>>(q);
      else glx_row_grad_kernel<REQ, kG, VEC, kDT, true><<<blocks, 256, 0, s>>>(q);
    });
    if (ch != nullptr) {
      const unsigned cblocks = (unsigned)(((int64_t)ch->max_items + (256 / kG) - 1) / (256 / kG));
      glx_row_grad_chunk_kernel<REQ, kG, VEC><<<cblocks, 256, 0, s>>>(q, *ch);
    }
  });
  if (ch != nullptr) glx_chunks_combine(*ch, q.grad_x(), q.dtype(), q.dim(), VEC == 4, s);
}

#endif  // GLX_CHUNKS_H_
