// How the batched calls lay their tables out in one pinned block and one upload, and the array of first workgroups their launches
// bisect (seg_device.h seg_find).  No HIP in here, like the *_plan.h headers: a CPU program can include this header and check the offsets
// on its own (tests/cpp/seg_table_check.cpp).
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

namespace dgs {
namespace segtab {

// Offsets handed out front to back: take() rounds the end up to `align` (a power of two), places `bytes` there and returns the place.
struct Layout {
  size_t end = 0;
  size_t take(const size_t bytes, const size_t align) {
    const size_t at = (end + align - 1) & ~(align - 1);
    end = at + bytes;
    return at;
  }
};

// The first workgroup of each of `m` items, then the number of workgroups: m + 1 entries.  An item that owns no workgroup repeats its
// successor's first, which seg_find never picks.
template <class Item>
std::vector<int> first_array(const Item* items, const size_t m, int Item::*first, const int total) {
  std::vector<int> f(m + 1);
  for (size_t j = 0; j < m; j++) f[j] = items[j].*first;
  f[m] = total;
  return f;
}

// A stage over many scans (compact.h seg_upload; the RANSAC rounds of floor_detection_batch.hip): entries | heads | first workgroups | first search
// workgroups go up in one copy of `up` bytes; behind them, in the pinned block only, the totals and the statistics come down.
struct StageTable {
  size_t entries, heads, first, knn_first, up, totals, stats, all;
};
inline StageTable stage_table(const size_t m, const size_t entry_bytes, const size_t head_bytes) {   // head_bytes 0: a stage without heads
  Layout L;
  StageTable T;
  T.entries = L.take(m * entry_bytes, 64);
  T.heads = L.take(m * head_bytes, 64);
  T.first = L.take((m + 1) * sizeof(int), 64);
  T.knn_first = L.take((m + 1) * sizeof(int), 64);
  T.up = T.totals = L.take(m * sizeof(int), 64);
  T.stats = L.take(m * 4 * sizeof(double), 64);
  T.all = L.end;
  return T;
}
// the part of `block` that goes up, zeroed, with the entries and the first workgroups (m + 1 of them) at their places
inline void place(char* block, const StageTable& T, const void* entries, const size_t entries_bytes, const std::vector<int>& first) {
  std::memset(block, 0, T.up);
  std::memcpy(block + T.entries, entries, entries_bytes);
  std::memcpy(block + T.first, first.data(), first.size() * sizeof(int));
}

// A chunk of the batched covariance pass (cov_batch.hip ensure_covariances): entries | first search workgroups | first covariance
// workgroups, the chunks back to back, each from a multiple of 64 on; L.end is a multiple of 64 afterwards.
struct ChunkTable {
  size_t entries, knn_first, cov_first, end;
};
inline ChunkTable chunk_table(Layout& L, const size_t count, const size_t entry_bytes) {
  ChunkTable T;
  T.entries = L.take(count * entry_bytes, 64);
  T.knn_first = L.take((count + 1) * sizeof(int), alignof(int));
  T.cov_first = L.take((count + 1) * sizeof(int), alignof(int));
  T.end = L.end;
  L.take(0, 64);
  return T;
}

}  // namespace segtab
}  // namespace dgs
