// glx_columns: the per-row properties of a node or edge type beside the float block -- int attributes, timestamp,
// weight, label -- as ONE device table of fixed-width records (NodeStorage::GetWeight / GetLabel / GetTimestamp /
// GetAttribute, memory_node_storage.cc:88-138; EdgeStorage's, memory_edge_storage.cc:90-125).
//
// Record of row r, fields the type lacks left out:
//   int_attrs int64[i_num] | timestamp int64 | weight float32 | label int32 | zero padding
// padded to a multiple of 8 bytes, and to a multiple of 16 once it is 16 bytes or longer: the 8-byte fields come
// first, so every field is naturally aligned, a record never straddles more 16-byte pieces than it needs, and one id
// translation plus one contiguous read serves every column a request asks for (a random access costs a whole line
// whatever it uses: the argument for the 16-byte adj records).
#include <string.h>

#include <new>

#include "glx_common.h"

struct glx_columns {
  int device;
  int64_t num_rows;
  int32_t i_num;
  bool has_weight, has_label, has_timestamp;
  int32_t stride;  // bytes per record: 0 (no column at all), 8, or a multiple of 16
  char* data;      // [max(num_rows, 1) * stride], 256-byte aligned; nullptr when stride == 0
  GlxIdMapStorage idmap;       // own map (ids given), or
  const glx_features* map_of;  // the borrowed one, or neither: id r is row r
  GlxIdMap map() const { return map_of ? map_of->map() : idmap.view(num_rows); }
};

namespace {

struct ColLayout {
  int32_t i_num;
  int32_t ts_slot;  // 8-byte slot of the timestamp, -1: none
  int32_t wl_slot;  // 8-byte slot that holds weight and / or label (the weight, when present, in its low dword), -1: neither
  int32_t l_hi;     // 1: the label is the slot's high dword (a weight precedes it), 0: its low dword
  int32_t has_w, has_l;
  int32_t stride;   // bytes
};

ColLayout layout_of(int32_t i_num, bool has_w, bool has_l, bool has_ts) {
  ColLayout L;
  L.i_num = i_num;
  int32_t slots = i_num;
  L.ts_slot = has_ts ? slots++ : -1;
  L.wl_slot = (has_w || has_l) ? slots++ : -1;
  L.l_hi = (has_w && has_l) ? 1 : 0;
  L.has_w = has_w;
  L.has_l = has_l;
  int64_t bytes = (int64_t)slots * 8;
  if (bytes >= 16) bytes = (bytes + 15) / 16 * 16;
  L.stride = (int32_t)bytes;
  return L;
}

struct ColDefaults {
  uint32_t weight_bits;  // a float moved as its bits: NaN payloads survive
  int32_t label;
  int64_t timestamp;
  int64_t int_attr;
};

struct ColOut {
  uint32_t* w;
  int32_t* l;
  int64_t* ts;
  int64_t* ia;
};

// Builds the records from the separate columns: one thread per (row, 8-byte slot).
__global__ __launch_bounds__(256) void glx_columns_pack_kernel(ColLayout L, int64_t num_rows, const uint32_t* __restrict__ w,
                                                               const int32_t* __restrict__ l, const int64_t* __restrict__ ts,
                                                               const int64_t* __restrict__ ia, uint64_t* __restrict__ table) {
  const int64_t slots = L.stride / 8;
  const int64_t total = num_rows * slots;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += step) {
    const int64_t r = t / slots;
    const int32_t s = (int32_t)(t - r * slots);
    uint64_t v = 0;
    if (s < L.i_num) {
      v = (uint64_t)ia[r * (int64_t)L.i_num + s];
    } else if (s == L.ts_slot) {
      v = (uint64_t)ts[r];
    } else if (s == L.wl_slot) {
      const uint32_t lo = L.has_w ? w[r] : (uint32_t)l[r];
      const uint32_t hi = (L.has_w && L.has_l) ? (uint32_t)l[r] : 0u;
      v = ((uint64_t)hi << 32) | lo;
    }
    table[t] = v;
  }
}

// A type without any column: every answer is the "type lacks it" constant, whatever the id.
__global__ __launch_bounds__(256) void glx_columns_const_kernel(int64_t n, ColOut out) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += step) {
    if (out.w) out.w[i] = 0u;  // 0.0f
    if (out.l) out.l[i] = -1;
    if (out.ts) out.ts[i] = -1;
  }
}

__device__ __forceinline__ uint32_t pick4(const uint4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

// Records of 8 or 16 bytes: one thread per id, one load per id; consecutive lanes store consecutive outputs.
template <int STRIDE>
__global__ __launch_bounds__(256) void glx_columns_narrow_kernel(GlxIdMap map, const char* __restrict__ table, ColLayout L,
                                                                 const int64_t* __restrict__ ids, int64_t n, ColDefaults d,
                                                                 ColOut out) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += step) {
    const int64_t row = glx_row_of(map, ids[i]);
    const bool known = row >= 0;
    const char* rec = table + (known ? row : 0) * (int64_t)STRIDE;  // an unknown id reads row 0 and keeps the default
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (STRIDE == 16) {
      v = *reinterpret_cast<const uint4*>(rec);
    } else {
      const uint2 q = *reinterpret_cast<const uint2*>(rec);
      v.x = q.x;
      v.y = q.y;
    }
    if (out.ia && L.i_num > 0) {  // i_num is 1 or 2 here
      for (int32_t j = 0; j < L.i_num; ++j) {
        const int64_t a = (int64_t)(((uint64_t)pick4(v, 2 * j + 1) << 32) | pick4(v, 2 * j));
        out.ia[i * (int64_t)L.i_num + j] = known ? a : d.int_attr;
      }
    }
    if (out.ts) {
      int64_t a = -1;
      if (L.ts_slot >= 0) {
        a = (int64_t)(((uint64_t)pick4(v, 2 * L.ts_slot + 1) << 32) | pick4(v, 2 * L.ts_slot));
        a = known ? a : d.timestamp;
      }
      out.ts[i] = a;
    }
    if (out.w) out.w[i] = L.has_w ? (known ? pick4(v, 2 * L.wl_slot) : d.weight_bits) : 0u;
    if (out.l) out.l[i] = L.has_l ? (known ? (int32_t)pick4(v, 2 * L.wl_slot + L.l_hi) : d.label) : -1;
  }
}

// Wider records: W lanes per id (W = LOG2W's power of two, the smallest that covers the record with 16 bytes per lane,
// at most 64; longer records take several rounds).  A wave takes 64 ids at a time: lane l translates id l -- one
// translation per id, one coalesced read of the ids -- and the groups then walk through the 64 rows, 64 / W at a time,
// fetching them from the lane that translated them.  A group writes its row's int attributes as one contiguous span.
template <int LOG2W>
__global__ __launch_bounds__(256) void glx_columns_wide_kernel(GlxIdMap map, const char* __restrict__ table, ColLayout L,
                                                               const int64_t* __restrict__ ids, int64_t n, ColDefaults d,
                                                               ColOut out) {
  constexpr int W = 1 << LOG2W;
  constexpr int GROUPS = 64 / W;  // ids a wave serves per step
  const int lane = threadIdx.x & 63;
  const int sub = lane & (W - 1);   // this lane's 16-byte piece of the record
  const int grp = lane >> LOG2W;
  const int32_t pieces = L.stride >> 4;
  const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t wave0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t tiles = (n + 63) >> 6;
  for (int64_t tile = wave0; tile < tiles; tile += waves) {
    const int64_t base = tile << 6;
    const int64_t mine = base + lane;
    const int64_t my_row = mine < n ? glx_row_of(map, ids[mine]) : -1;
#pragma unroll 1
    for (int t = 0; t < W; ++t) {
      const int j = t * GROUPS + grp;  // the id of the tile this group serves now
      const int64_t row = __shfl(my_row, j);
      const int64_t i = base + j;
      const bool live = i < n;
      const bool known = row >= 0;
      const char* rec = table + (known ? row : 0) * (int64_t)L.stride;  // an unknown id reads row 0, keeps the default
      for (int32_t p = sub; p < pieces; p += W) {
        const uint4 v = *reinterpret_cast<const uint4*>(rec + ((int64_t)p << 4));
        if (!live) continue;
        const int32_t s0 = 2 * p, s1 = 2 * p + 1;  // the two 8-byte slots of this piece
        int64_t a0 = (int64_t)(((uint64_t)v.y << 32) | v.x), a1 = (int64_t)(((uint64_t)v.w << 32) | v.z);
        if (out.ia) {
          int64_t* o = out.ia + i * (int64_t)L.i_num;
          const int64_t b0 = known ? a0 : d.int_attr, b1 = known ? a1 : d.int_attr;
          if (s1 < L.i_num && (reinterpret_cast<uintptr_t>(o + s0) & 15) == 0) {
            *reinterpret_cast<longlong2*>(o + s0) = make_longlong2(b0, b1);
          } else {
            if (s0 < L.i_num) o[s0] = b0;
            if (s1 < L.i_num) o[s1] = b1;
          }
        }
        if (out.ts && L.ts_slot >= 0 && (L.ts_slot >> 1) == p) {
          const int64_t a = (L.ts_slot & 1) ? a1 : a0;
          out.ts[i] = known ? a : d.timestamp;
        }
        if (L.wl_slot >= 0 && (L.wl_slot >> 1) == p) {
          const uint32_t lo = (L.wl_slot & 1) ? v.z : v.x, hi = (L.wl_slot & 1) ? v.w : v.y;
          if (out.w && L.has_w) out.w[i] = known ? lo : d.weight_bits;
          if (out.l && L.has_l) out.l[i] = known ? (int32_t)(L.l_hi ? hi : lo) : d.label;
        }
      }
      // columns the type lacks: the constant, written once per id
      if (live && sub == 0) {
        if (out.ts && L.ts_slot < 0) out.ts[i] = -1;
        if (out.w && !L.has_w) out.w[i] = 0u;
        if (out.l && !L.has_l) out.l[i] = -1;
      }
    }
  }
}

template <int LOG2W>
void launch_wide(const glx_columns* c, const ColLayout& L, const int64_t* d_ids, int64_t n, const ColDefaults& d,
                 const ColOut& out, hipStream_t s) {
  int64_t blocks = (n + 255) / 256;  // a wave per 64 ids
  if (blocks > 16384) blocks = 16384;
  glx_columns_wide_kernel<LOG2W><<<(unsigned)blocks, 256, 0, s>>>(c->map(), c->data, L, d_ids, n, d, out);
}

void columns_lookup_device(const glx_columns* c, const int64_t* d_ids, int64_t n, const ColDefaults& d, const ColOut& out,
                           hipStream_t s) {
  const ColLayout L = layout_of(c->i_num, c->has_weight, c->has_label, c->has_timestamp);
  int64_t blocks = (n + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  if (c->stride == 0) {
    glx_columns_const_kernel<<<(unsigned)blocks, 256, 0, s>>>(n, out);
  } else if (c->stride == 8) {
    glx_columns_narrow_kernel<8><<<(unsigned)blocks, 256, 0, s>>>(c->map(), c->data, L, d_ids, n, d, out);
  } else if (c->stride == 16) {
    glx_columns_narrow_kernel<16><<<(unsigned)blocks, 256, 0, s>>>(c->map(), c->data, L, d_ids, n, d, out);
  } else {
    const int32_t pieces = c->stride / 16;
    int log2w = 1;
    while (log2w < 6 && (1 << log2w) < pieces) ++log2w;
    switch (log2w) {
      case 1: launch_wide<1>(c, L, d_ids, n, d, out, s); break;
      case 2: launch_wide<2>(c, L, d_ids, n, d, out, s); break;
      case 3: launch_wide<3>(c, L, d_ids, n, d, out, s); break;
      case 4: launch_wide<4>(c, L, d_ids, n, d, out, s); break;
      case 5: launch_wide<5>(c, L, d_ids, n, d, out, s); break;
      default: launch_wide<6>(c, L, d_ids, n, d, out, s); break;
    }
  }
}

}  // namespace

extern "C" int glx_columns_create(int device, int64_t num_rows, int32_t i_num, const float* weights, const int32_t* labels,
                                  const int64_t* timestamps, const int64_t* int_attrs, const int64_t* ids,
                                  const glx_features* map_of, int ptr_kind, void* stream, glx_columns** out) {
  GLX_REQUIRE(out != nullptr, "out is NULL");
  *out = nullptr;
  GLX_REQUIRE(num_rows >= 0, "negative num_rows %lld", (long long)num_rows);
  GLX_REQUIRE(i_num >= 0, "negative i_num %d", i_num);
  GLX_REQUIRE(i_num <= (1 << 20), "i_num %d is beyond 2^20", i_num);
  GLX_REQUIRE(i_num > 0 || int_attrs == nullptr, "int_attrs given with i_num == 0");
  GLX_REQUIRE(i_num == 0 || num_rows == 0 || int_attrs != nullptr, "int_attrs is NULL with i_num == %d", i_num);
  GLX_REQUIRE(ids == nullptr || map_of == nullptr, "both ids and map_of given: a table has one id map");
  GLX_REQUIRE(ptr_kind == GLX_PTR_HOST || ptr_kind == GLX_PTR_DEVICE, "bad ptr_kind");
  GLX_REQUIRE(ids == nullptr || num_rows < INT32_MAX, "num_rows must be < 2^31 with an id map");
  GLX_REQUIRE(map_of == nullptr || map_of->num_rows == num_rows, "map_of holds %lld rows, the table %lld",
              map_of ? (long long)map_of->num_rows : 0ll, (long long)num_rows);
  GLX_REQUIRE(map_of == nullptr || map_of->device == device, "map_of lives on device %d, the table on %d",
              map_of ? map_of->device : 0, device);
  int rc = glx_init_device(device);
  if (rc != GLX_OK) return rc;
  GlxDeviceGuard guard(device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", device);
  hipStream_t s = glx_stream(stream);
  glx_columns* c = new (std::nothrow) glx_columns();
  GLX_REQUIRE(c != nullptr, "out of host memory");
  memset(static_cast<void*>(c), 0, sizeof(*c));
  c->device = device;
  c->num_rows = num_rows;
  c->i_num = i_num;
  c->has_weight = weights != nullptr;
  c->has_label = labels != nullptr;
  c->has_timestamp = timestamps != nullptr;
  c->map_of = map_of;
  const ColLayout L = layout_of(i_num, c->has_weight, c->has_label, c->has_timestamp);
  c->stride = L.stride;
  hipError_t e = hipSuccess;
  GlxTemp tw, tl, tt, ti, tids;
  const uint32_t* d_w = reinterpret_cast<const uint32_t*>(weights);
  const int32_t* d_l = labels;
  const int64_t *d_t = timestamps, *d_i = int_attrs, *d_ids = ids;
  if (ptr_kind == GLX_PTR_HOST && num_rows > 0) {
    auto stage = [&](GlxTemp& tmp, const void* h, size_t bytes, const void** d) {
      if (h == nullptr || e != hipSuccess) return;
      e = hipMalloc(&tmp.p, bytes);
      if (e == hipSuccess) e = hipMemcpyAsync(tmp.p, h, bytes, hipMemcpyHostToDevice, s);
      *d = tmp.p;
    };
    stage(tw, weights, (size_t)num_rows * 4, reinterpret_cast<const void**>(&d_w));
    stage(tl, labels, (size_t)num_rows * 4, reinterpret_cast<const void**>(&d_l));
    stage(tt, timestamps, (size_t)num_rows * 8, reinterpret_cast<const void**>(&d_t));
    stage(ti, int_attrs, (size_t)num_rows * i_num * 8, reinterpret_cast<const void**>(&d_i));
    stage(tids, ids, (size_t)num_rows * 8, reinterpret_cast<const void**>(&d_ids));
  }
  if (e == hipSuccess && c->stride > 0) {
    const size_t bytes = (size_t)(num_rows > 0 ? num_rows : 1) * (size_t)c->stride;
    e = hipMalloc(reinterpret_cast<void**>(&c->data), bytes);
    if (e == hipSuccess && num_rows == 0) e = hipMemsetAsync(c->data, 0, bytes, s);  // row 0 is read for unknown ids
    if (e == hipSuccess && num_rows > 0) {
      const int64_t total = num_rows * (int64_t)(c->stride / 8);
      int64_t blocks = (total + 255) / 256;
      if (blocks > 65536) blocks = 65536;
      glx_columns_pack_kernel<<<(unsigned)blocks, 256, 0, s>>>(L, num_rows, d_w, d_l, d_t, d_i,
                                                              reinterpret_cast<uint64_t*>(c->data));
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess && ids != nullptr && num_rows > 0) rc = glx_idmap_build_auto(d_ids, num_rows, &c->idmap, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess || rc != GLX_OK) {
    if (e != hipSuccess) glx_set_error("column upload failed: %s", hipGetErrorString(e));
    glx_columns_destroy(c);
    return e == hipErrorOutOfMemory ? GLX_RESOURCE_EXHAUSTED : (rc != GLX_OK ? rc : GLX_INTERNAL);
  }
  *out = c;
  return GLX_OK;
}

extern "C" void glx_columns_destroy(glx_columns* c) {
  if (!c) return;
  GlxDeviceGuard guard(c->device);
  if (c->data) (void)hipFree(c->data);
  glx_idmap_free(&c->idmap);
  delete c;
}

extern "C" int glx_columns_info(const glx_columns* c, int64_t* num_rows, int32_t* i_num, int* has_weight, int* has_label,
                                int* has_timestamp, int32_t* record_bytes, int* id_map, int* device) {
  GLX_REQUIRE(c != nullptr, "columns is NULL");
  if (num_rows) *num_rows = c->num_rows;
  if (i_num) *i_num = c->i_num;
  if (has_weight) *has_weight = c->has_weight;
  if (has_label) *has_label = c->has_label;
  if (has_timestamp) *has_timestamp = c->has_timestamp;
  if (record_bytes) *record_bytes = c->stride;
  if (id_map) *id_map = c->map_of ? GLX_COLUMNS_MAP_BORROWED : (c->idmap.any() ? GLX_COLUMNS_MAP_OWN : GLX_COLUMNS_MAP_DENSE);
  if (device) *device = c->device;
  return GLX_OK;
}

extern "C" int glx_columns_lookup(const glx_columns* c, const int64_t* ids, int64_t n, float default_weight,
                                  int32_t default_label, int64_t default_timestamp, int64_t default_int_attr,
                                  float* weights_out, int32_t* labels_out, int64_t* timestamps_out, int64_t* int_attrs_out,
                                  int ptr_kind, void* stream) {
  GLX_REQUIRE(c != nullptr, "columns is NULL");
  GLX_REQUIRE(n >= 0, "negative n");
  GLX_REQUIRE(ptr_kind == GLX_PTR_HOST || ptr_kind == GLX_PTR_DEVICE, "bad ptr_kind");
  if (n == 0) return GLX_OK;
  GLX_REQUIRE(ids != nullptr, "NULL data pointer");
  if (c->i_num == 0) int_attrs_out = nullptr;  // [n * 0]: nothing to write
  if (!weights_out && !labels_out && !timestamps_out && !int_attrs_out) return GLX_OK;
  GlxDeviceGuard guard(c->device);
  GLX_REQUIRE(guard.ok, "cannot select device %d", c->device);
  GlxHostStage st(c->device, ptr_kind, stream, GlxHostStage::ADMIT | GlxHostStage::DIRECT_PINNED);
  const int64_t* d_ids;
  ColOut out;
  st.in(&d_ids, ids, (size_t)n);
  st.out(reinterpret_cast<float**>(&out.w), weights_out, (size_t)n);
  st.out(&out.l, labels_out, (size_t)n);
  st.out(&out.ts, timestamps_out, (size_t)n);
  st.out(&out.ia, int_attrs_out, (size_t)n * (size_t)c->i_num);
  int rc = st.begin();
  if (rc == GLX_OK) {
    ColDefaults d;
    memcpy(&d.weight_bits, &default_weight, sizeof(float));
    d.label = default_label;
    d.timestamp = default_timestamp;
    d.int_attr = default_int_attr;
    columns_lookup_device(c, d_ids, n, d, out, st.s);
  }
  return st.finish(rc);
}
