// Host-side driver of a batch whose pairs advance together, one launch (or launch group) per round: FAST_GICP / FAST_VGICP (gicp.hip),
// ICP_HIP (icp.hip), GICP_HIP (pcl_gicp.hip).  Pinned staging, the chunked launch loop with its done-counter poll, the fixed-slices
// table, the walk order of a source, the window of a trajectory getter.  The kernels' side of the fixed slices: slice_rows.h.
// (NDT's chunk loop does more per chunk -- deferred side build, early fitness, the third stream -- and stays in ndt_align.hip.)
#pragma once
#include <algorithm>

#include "handle.h"

namespace dgs {

// Pinned staging of one batch of n pairs: [0, 64) the two done flags of run_rounds_polled | inits | items | pair states read back,
// every block 64-byte aligned.  The accessors read h->pinned when called: valid after ensure().
template <class Init, class Item, class Pair>
struct BatchStaging {
  dgs_handle* h;
  size_t off_init, off_items, off_pairs, bytes;
  BatchStaging(dgs_handle* h_, int n) : h(h_) {
    size_t o = 64;
    off_init = o;
    o = (o + (size_t)n * sizeof(Init) + 63) & ~(size_t)63;
    off_items = o;
    o = (o + (size_t)n * sizeof(Item) + 63) & ~(size_t)63;
    off_pairs = o;
    bytes = o + (size_t)n * sizeof(Pair);
  }
  int ensure() const { return ensure_pinned(h, bytes) != DGS_OK ? DGS_ERR_HIP : DGS_OK; }
  Init* inits() const { return reinterpret_cast<Init*>(reinterpret_cast<char*>(h->pinned) + off_init); }
  Item* items() const { return reinterpret_cast<Item*>(reinterpret_cast<char*>(h->pinned) + off_items); }
  Pair* pairs() const { return reinterpret_cast<Pair*>(reinterpret_cast<char*>(h->pinned) + off_pairs); }
  // the device pair states -> pairs(), synchronously.  what: "ICP state", ... for the error text
  int read_back(const DevBuf<Pair>& dev, int n, const char* what) const {
    if (hipMemcpyAsync(pairs(), dev.ptr, (size_t)n * sizeof(Pair), hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess ||
        hipGetLastError() != hipSuccess) {
      h->err = std::string("reading the ") + what + " back failed";
      return DGS_ERR_HIP;
    }
    return DGS_OK;
  }
};

// Rounds in chunks with a done-counter poll between them: no host round trip per round.  launch_round() enqueues one round on h->stream;
// every chunk is followed by a copy of done_counter[0] (pairs that have finished, counted by their closing workgroups) into one of two
// pinned flags and an event.  While the device runs chunk k + 1 the host waits for chunk k's event and stops once every live pair is done:
// at most one chunk of launches (whose workgroups return at once) is enqueued in vain.  The last chunk is cut at max_rounds.
template <class F>
int run_rounds_polled(dgs_handle* h, int n_live, long max_rounds, int chunk, F&& launch_round) {
  hipStream_t st = h->stream;
  volatile int* flags = reinterpret_cast<volatile int*>(h->pinned);
  flags[0] = flags[1] = 0;
  if (ensure_poll_events(h) != DGS_OK) return DGS_ERR_HIP;
  hipEvent_t* ev = h->ev_poll;
  long queued = 0;
  auto enqueue = [&](int slot) -> int {
    for (int e = 0; e < chunk && queued < max_rounds; e++, queued++) launch_round();
    DGS_HIP_TRY(h, hipGetLastError());
    DGS_HIP_TRY(h, hipMemcpyAsync(const_cast<int*>(&flags[slot]), h->done_counter.ptr, sizeof(int), hipMemcpyDeviceToHost, st));
    DGS_HIP_TRY(h, hipEventRecord(ev[slot], st));
    return DGS_OK;
  };
  int cur = 0;
  int rc = enqueue(0);
  while (rc == DGS_OK) {
    const bool more = queued < max_rounds;
    if (more) rc = enqueue(cur ^ 1);
    if (rc != DGS_OK) break;
    hipError_t e = hipEventSynchronize(ev[cur]);
    if (e != hipSuccess) { h->err = std::string("hipEventSynchronize: ") + hipGetErrorString(e); rc = DGS_ERR_HIP; break; }
    if (flags[cur] >= n_live || !more) break;
    cur ^= 1;
  }
  return rc;
}

// Fixed slices: every pair owns a number of workgroups that is a function of its own size only, so its sums -- and with them its result --
// do not depend on which other pairs share the batch.  Workgroup -> pair comes from the table upload() makes (h->slice_blk_pair); one row
// of row_stride doubles per workgroup in h->slice_rows.
struct SliceTable {
  std::vector<int> slice0, n_slices, blk;   // blk: pageable, read by upload()'s copy -- the caller syncs the stream before this object goes
  int total_slices = 0;
  SliceTable(int n, CloudState* const* srcs, int points_per_slice) : slice0(n), n_slices(n) {
    for (int i = 0; i < n; i++) add(i, srcs[i]->n, points_per_slice);
  }
  // live sizes: 0 for a pair that never becomes active, so that it owns no slice (and no workgroup) whatever its cloud holds
  SliceTable(const std::vector<int64_t>& live_n, int points_per_slice) : slice0(live_n.size()), n_slices(live_n.size()) {
    for (size_t i = 0; i < live_n.size(); i++) add((int)i, live_n[i], points_per_slice);
  }
  void add(int i, int64_t points, int points_per_slice) {
    slice0[i] = total_slices;
    n_slices[i] = (int)((points + points_per_slice - 1) / points_per_slice);
    total_slices += n_slices[i];
  }
  int upload(dgs_handle* h, int row_stride) {
    DGS_HIP_TRY(h, h->slice_blk_pair.reserve((size_t)std::max(total_slices, 1)));
    DGS_HIP_TRY(h, h->slice_rows.reserve((size_t)std::max(total_slices, 1) * row_stride));
    blk.assign((size_t)std::max(total_slices, 1), 0);
    for (size_t i = 0; i < slice0.size(); i++) std::fill_n(blk.begin() + slice0[i], n_slices[i], (int)i);
    DGS_HIP_TRY(h, hipMemcpyAsync(h->slice_blk_pair.ptr, blk.data(), blk.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    return DGS_OK;
  }
};

// A fixed-slices walk takes the source in Hilbert order whatever other index the cloud carries (a resident cloud that was the target of a
// large batch holds a k-d ordered one, and keeps a second, Hilbert-ordered index in `walk`): the order of a pair's double sums is a
// function of its points alone.
inline int ensure_walk_order(dgs_handle* h, CloudState& s) {
  if (!s.bvh.valid) {
    int rc = bvh_build(h, s.bvh, s.pts.ptr, s.n);
    if (rc) return rc;
  }
  if (s.bvh.kd && !s.walk.valid) return bvh_build(h, s.walk, s.pts.ptr, s.n);
  return DGS_OK;
}
inline const float4* walk_sorted(const CloudState& s) { return (s.bvh.valid && s.bvh.kd) ? s.walk.sorted.ptr : s.bvh.sorted.ptr; }

// Window of a trajectory getter: *len entries were recorded for `pair` (cap per pair), *m of them fit the caller's capacity, the first
// is entry *offset of the device arrays.
inline int traj_window(const std::vector<int>& last_iters, int cap, int pair, int capacity, int* len, int* m, size_t* offset) {
  if (pair < 0 || (size_t)pair >= last_iters.size()) return DGS_ERR_INVALID_ARGUMENT;
  *len = std::min(last_iters[pair], cap);
  *m = std::min(*len, std::max(capacity, 0));
  *offset = (size_t)pair * cap;
  return DGS_OK;
}

}  // namespace dgs
