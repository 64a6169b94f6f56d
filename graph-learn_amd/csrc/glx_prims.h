// glx internal header: rocprim device primitives (sort, scan, run-length encode, reduce-by-key) that take temporary
// storage.  rocprim's protocol is two calls: one with a null temporary that only reports the size, one that runs.
// The two helpers below do both calls around one allocation.  `call` is one rocprim entry point with every other
// argument bound:
//     call(void* tmp, size_t& bytes) -> hipError_t
// `what` names the step in the error text.  Callers that size SEVERAL primitives and carve them out of one lease
// (glx_agg_transpose, glx_agg_segment_ends, glx_rows_coalesce, glx_negative_sample) stay hand-written: DESIGN.md.
#ifndef GLX_PRIMS_H_
#define GLX_PRIMS_H_
#include "glx_common.h"  // first: rocprim's texture_cache_iterator uses memset without including <string.h>

#include <rocprim/rocprim.hpp>

inline int glx_prim_fail(const char* what, const char* stage, hipError_t e) {
  glx_set_error("%s: %s failed: %s", what, stage, hipGetErrorString(e));
  return e == hipErrorOutOfMemory ? GLX_RESOURCE_EXHAUSTED : GLX_INTERNAL;
}

// Temporary from hipMalloc, released before the return; `s` is synchronised first.  hipMalloc / hipFree synchronise
// the device: build-time paths only.
template <typename Call>
int glx_prim_temp(hipStream_t s, const char* what, Call&& call) {
  size_t bytes = 0;
  hipError_t e = call(nullptr, bytes);
  if (e != hipSuccess) return glx_prim_fail(what, "size query", e);
  GlxTemp tmp;
  e = hipMalloc(&tmp.p, bytes ? bytes : 16);
  if (e != hipSuccess) return glx_prim_fail(what, "allocation", e);
  e = call(tmp.p, bytes);
  if (e != hipSuccess) return glx_prim_fail(what, "run", e);
  e = hipStreamSynchronize(s);  // tmp is freed right after
  if (e != hipSuccess) return glx_prim_fail(what, "run", e);
  return GLX_OK;
}

// Temporary leased from workspace `slot` of `s`; no synchronise, the lease ends on return (work on one stream is
// ordered).  Per-request paths.
template <typename Call>
int glx_prim_leased(hipStream_t s, int slot, const char* what, Call&& call) {
  size_t bytes = 0;
  hipError_t e = call(nullptr, bytes);
  if (e != hipSuccess) return glx_prim_fail(what, "size query", e);
  GlxScratch lease;
  const int rc = lease.alloc(bytes ? bytes : 8, s, slot);
  if (rc != GLX_OK) {
    char cause[384];  // glx_scratch_alloc's text: the HIP error string, or the slot being leased already
    snprintf(cause, sizeof(cause), "%s", glx_last_error());
    glx_set_error("%s: allocation failed: %s", what, cause);
    return rc;
  }
  e = call(lease.p, bytes);
  if (e != hipSuccess) return glx_prim_fail(what, "run", e);
  return GLX_OK;
}

#endif  // GLX_PRIMS_H_
