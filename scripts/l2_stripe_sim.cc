// l2_stripe_sim: how many 128-byte lines leave the per-XCD L2s when glx_aggregate_grp_kernel reduces a request of
// uniform segments under a given workgroup -> (segment block, column slice) mapping.  Host-only model of the launch:
//   * workgroup b is dealt to XCD b % 8 (the observed placement); each XCD runs `resident` workgroups at a time, in
//     dispatch order, and the resident ones advance together one row position at a time (row u of every segment of
//     every resident workgroup, then row u + 1, ...);
//   * a workgroup holds 256 / G segments and touches, per segment, the 8-byte ids once (one coalesced chunk) and, per
//     id, its row's column slice: (D / n) * 4 bytes at byte offset slice * (D / n) * 4 of the (swizzled) row;
//   * 8 private L2s: 4 MiB each, 128-byte lines, 16-way LRU, set = line index mod the number of sets.  A miss is one
//     line fetched over the fabric.  Output stores are non-temporal and not counted.
// Usage: l2_stripe_sim <ids.npy> <fanout> <dim> <num_rows> <mapping>...   mapping = rr:<n> | stripe:<n>:<chunk> |
// perm:<n>:<order.npy> (segments reduced in the order the int32 permutation gives, with today's rr mapping).
// Prints one line per mapping: fetched lines, accesses, hit rate.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

constexpr int kXcds = 8;
constexpr int kLineBytes = 128;
constexpr int kWays = 16;
constexpr int64_t kL2Bytes = 4 << 20;
constexpr int kSets = (int)(kL2Bytes / kLineBytes / kWays);
constexpr int kSwizzleBits = 12;  // glx_common.h GLX_SWIZZLE_BITS

struct L2 {
  std::vector<uint64_t> tag = std::vector<uint64_t>((size_t)kSets * kWays, ~0ull);
  std::vector<uint64_t> stamp = std::vector<uint64_t>((size_t)kSets * kWays, 0);
  uint64_t clock = 0, hits = 0, misses = 0;
  void access(uint64_t line) {
    const size_t set = (size_t)(line % kSets) * kWays;
    ++clock;
    size_t victim = set;
    for (size_t w = set; w < set + kWays; ++w) {
      if (tag[w] == line) {
        stamp[w] = clock;
        ++hits;
        return;
      }
      if (stamp[w] < stamp[victim]) victim = w;
    }
    tag[victim] = line;
    stamp[victim] = clock;
    ++misses;
  }
};

// .npy v1/v2/v3, little-endian int32 or int64, 1-D (or C-order N-D: flattened)
std::vector<int64_t> load_npy(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    exit(2);
  }
  unsigned char pre[10];
  if (fread(pre, 1, 10, f) != 10 || memcmp(pre, "\x93NUMPY", 6) != 0) {
    fprintf(stderr, "%s: not a .npy file\n", path);
    exit(2);
  }
  uint32_t hlen = pre[8] | (pre[9] << 8);
  if (pre[6] >= 2) {
    unsigned char ext[2];
    if (fread(ext, 1, 2, f) != 2) exit(2);
    hlen |= (uint32_t)ext[0] << 16 | (uint32_t)ext[1] << 24;
  }
  std::string hdr(hlen, '\0');
  if (fread(&hdr[0], 1, hlen, f) != hlen) exit(2);
  int width = 0;
  if (hdr.find("'<i4'") != std::string::npos) width = 4;
  if (hdr.find("'<i8'") != std::string::npos) width = 8;
  if (width == 0 || hdr.find("'fortran_order': True") != std::string::npos) {
    fprintf(stderr, "%s: want little-endian int32 / int64 in C order (%s)\n", path, hdr.c_str());
    exit(2);
  }
  const long start = ftell(f);
  fseek(f, 0, SEEK_END);
  const size_t n = (size_t)(ftell(f) - start) / width;
  fseek(f, start, SEEK_SET);
  std::vector<int64_t> out(n);
  if (width == 8) {
    if (fread(out.data(), 8, n, f) != n) exit(2);
  } else {
    std::vector<int32_t> tmp(n);
    if (fread(tmp.data(), 4, n, f) != n) exit(2);
    for (size_t i = 0; i < n; ++i) out[i] = tmp[i];
  }
  fclose(f);
  return out;
}

int64_t swizzle_row(int64_t r, int64_t swizzle_rows) {  // glx_swizzle_row
  if (r >= swizzle_rows) return r;
  const uint32_t hi = (uint32_t)(r >> kSwizzleBits);
  const uint32_t m = (hi * 0x9E3779B1u) >> (32 - kSwizzleBits);
  return r ^ (int64_t)m;
}

// the kernel's agg_stripe_block
uint32_t stripe_block(uint32_t j, uint32_t P, uint32_t chunk, uint32_t full) {
  if (j >= full) return j;
  const uint32_t span = P * chunk;
  const uint32_t run = j / span;
  const uint32_t r = j - run * span;
  const uint32_t k = r / P;
  return run * span + (r - k * P) * chunk + k;
}

struct Result {
  uint64_t fetched, accesses;
};

Result simulate(const std::vector<int64_t>& ids, const std::vector<int64_t>& seg_order, int fanout, int dim,
                int64_t num_rows, int n, int chunk, int resident) {
  const int64_t num_segments = (int64_t)ids.size() / fanout;
  const int ncols = dim / n;
  const int lanes = ncols / 4;
  const int G = lanes >= 64 ? 64 : lanes >= 32 ? 32 : lanes >= 16 ? 16 : 8;
  const int segs_per_block = 256 / G;
  const int64_t seg_blocks = (num_segments + segs_per_block - 1) / segs_per_block;
  const int64_t grid = seg_blocks * n;
  const int P = kXcds / n;
  uint32_t full = 0;
  if (chunk > 0 && P > 1) full = (uint32_t)(seg_blocks / ((int64_t)P * chunk) * ((int64_t)P * chunk));
  const int64_t swz = (num_rows >> kSwizzleBits) << kSwizzleBits;
  const uint64_t row_bytes = (uint64_t)dim * 4;
  const uint64_t id_base = ((uint64_t)num_rows * row_bytes + (1ull << 30)) / kLineBytes * kLineBytes;  // ids after the table
  const int lines_per_piece = (ncols * 4 + kLineBytes - 1) / kLineBytes;
  std::vector<L2> l2(kXcds);
  uint64_t accesses = 0;
  // per XCD: its workgroups in dispatch order, run `resident` at a time
  for (int x = 0; x < kXcds; ++x) {
    L2& c = l2[x];
    for (int64_t b0 = x; b0 < grid; b0 += (int64_t)kXcds * resident) {
      std::vector<std::pair<int64_t, int>> wave;  // (first segment, slice)
      for (int64_t b = b0; b < grid && b < b0 + (int64_t)kXcds * resident; b += kXcds) {
        const int slice = (int)(b % n);
        uint32_t j = (uint32_t)(b / n);
        if (chunk > 0) j = stripe_block(j, P, chunk, full);
        wave.emplace_back((int64_t)j * segs_per_block, slice);
      }
      // ids: one coalesced chunk per segment (fanout * 8 bytes), read before the rows
      for (auto& w : wave) {
        for (int k = 0; k < segs_per_block && w.first + k < num_segments; ++k) {
          const int64_t sg = seg_order.empty() ? w.first + k : seg_order[w.first + k];
          const uint64_t lo = id_base + (uint64_t)sg * fanout * 8, hi = lo + (uint64_t)fanout * 8;
          for (uint64_t l = lo / kLineBytes; l <= (hi - 1) / kLineBytes; ++l, ++accesses) c.access(l);
        }
      }
      for (int u = 0; u < fanout; ++u) {
        for (auto& w : wave) {
          for (int k = 0; k < segs_per_block && w.first + k < num_segments; ++k) {
            const int64_t sg = seg_order.empty() ? w.first + k : seg_order[w.first + k];
            int64_t r = ids[(size_t)(sg * fanout + u)];
            if (r < 0 || r >= num_rows) r = 0;  // an unknown id reads row 0
            const uint64_t lo = (uint64_t)swizzle_row(r, swz) * row_bytes + (uint64_t)w.second * ncols * 4;
            for (int l = 0; l < lines_per_piece; ++l, ++accesses) c.access(lo / kLineBytes + l);
          }
        }
      }
    }
  }
  uint64_t fetched = 0;
  for (auto& c : l2) fetched += c.misses;
  return {fetched, accesses};
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 6) {
    fprintf(stderr, "usage: %s ids.npy fanout dim num_rows mapping... [resident=<W>]\n", argv[0]);
    return 2;
  }
  const std::vector<int64_t> ids = load_npy(argv[1]);
  const int fanout = atoi(argv[2]), dim = atoi(argv[3]);
  const int64_t num_rows = atoll(argv[4]);
  int resident = 256;  // workgroups in flight per XCD: 32 CUs x 8 of 256 threads
  for (int i = 5; i < argc; ++i) {
    if (strncmp(argv[i], "resident=", 9) == 0) resident = atoi(argv[i] + 9);
  }
  if (fanout <= 0 || dim % 4 != 0 || ids.size() % fanout != 0) {
    fprintf(stderr, "bad fanout / dim for %zu ids\n", ids.size());
    return 2;
  }
  printf("# %zu ids, %zu segments of %d, D = %d, %lld rows, %d workgroups resident per XCD, 8 x %lld KiB L2 (%d-way, %d-B lines)\n",
         ids.size(), ids.size() / fanout, fanout, dim, (long long)num_rows, resident, (long long)(kL2Bytes >> 10), kWays,
         kLineBytes);
  printf("# %-22s %14s %14s %9s\n", "mapping", "fetched_lines", "accesses", "hit_rate");
  for (int i = 5; i < argc; ++i) {
    const std::string m = argv[i];
    if (m.rfind("resident=", 0) == 0) continue;
    int n = 1, chunk = 0;
    std::vector<int64_t> order;
    if (m.rfind("rr:", 0) == 0) {
      n = atoi(m.c_str() + 3);
    } else if (m.rfind("stripe:", 0) == 0) {
      if (sscanf(m.c_str() + 7, "%d:%d", &n, &chunk) != 2 || chunk <= 0) return 2;
    } else if (m.rfind("perm:", 0) == 0) {
      n = atoi(m.c_str() + 5);
      order = load_npy(strchr(m.c_str() + 5, ':') + 1);
      if (order.size() != ids.size() / fanout) {
        fprintf(stderr, "permutation length %zu != segments\n", order.size());
        return 2;
      }
    } else {
      fprintf(stderr, "unknown mapping %s\n", m.c_str());
      return 2;
    }
    if (n != 1 && n != 2 && n != 4 && n != 8) return 2;
    const Result r = simulate(ids, order, fanout, dim, num_rows, n, chunk, resident);
    printf("%-24s %14llu %14llu %9.4f\n", m.substr(0, m.rfind("perm:", 0) == 0 ? 6 : m.size()).c_str(),
           (unsigned long long)r.fetched, (unsigned long long)r.accesses,
           1.0 - (double)r.fetched / (double)r.accesses);
    fflush(stdout);
  }
  return 0;
}
