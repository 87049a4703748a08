// dgs_handle: per-registration-object state (one per pcl::Registration instance on the reference side).
#pragma once
#include "building_cloud.h"
#include "common.h"
#include "cov_batch_plan.h"
#include "sac.h"

namespace dgs {

struct EventPair {
  hipEvent_t start, stop;
};

struct Profiler {
  bool enabled = false;
  std::vector<EventPair> pool;                 // all events ever created
  std::vector<int> pending[DGS_K_COUNT];       // indices into pool, recorded but not yet read
  std::vector<int> weight;                     // per pool slot: by how much its bracket advances `launches` (1; a batched covariance pass: its clouds)
  size_t next_free = 0;
  double total_ms[DGS_K_COUNT] = {0};
  int64_t launches[DGS_K_COUNT] = {0};
};

struct IcpPair;   // icp.hip
struct IcpItem;
struct PgPair;    // pcl_gicp.hip
struct PgItem;
struct PgInit;
struct PgTarget;
struct GicpTarget;   // gicp.hip

// Exact-NN index over a point cloud (nn_bvh.hip): Hilbert-sorted points, implicit complete 8-ary tree of AABBs.
struct Bvh {
  int64_t n = 0;            // points
  int leaves = 0;           // number of leaf slots (power of two), each covers kLeafSize sorted points
  int levels = 0;
  DevBuf<float4> sorted;    // points in Hilbert order, w = original index (bit-cast int)
  DevBuf<float4> node_lo;   // AABB min per node (heap order, root = 0); w unused
  DevBuf<float4> node_hi;
  DevBuf<uint32_t> keys, keys_alt;
  DevBuf<uint32_t> vals, vals_alt;
  DevBuf<unsigned> kd_bbox;   // k-d order build: boxes of the ranges of the current level
  bool kd = false;          // points are in k-d (median split) order instead of Hilbert order
  bool valid = false;
  void release() {
    sorted.release(); node_lo.release(); node_hi.release(); keys.release(); keys_alt.release(); vals.release(); vals_alt.release(); kd_bbox.release();
    valid = false;
  }
};

// Sparse 64-ary voxel hierarchy over a target cloud for one-lane-per-query exact 1-NN distances (nn_grid.hip).  Belongs to a
// handle (rebuilt at every setInputTarget: one sort of the target plus a few passes), not to a cached cloud: the dense tables
// (one entry per COARSE cell) are a fixed 8 MB budget per handle whatever the cloud.
constexpr int64_t kNnGridL2Cells = 8192;   // L2 cells (16 x 16 x 16 fine cells each) the tables are sized for
struct NnGridParams {   // decided on the device (grid_params_kernel): no host round trip between the tree build and this one
  float org[3];         // corner of fine cell (0, 0, 0)
  float c, inv_c;       // fine cell size; a coarse cell is 4 x 4 x 4 fine cells, an L2 cell 4 x 4 x 4 coarse cells
  int n2[3];            // L2 cells per axis
  int n;
};
struct __attribute__((aligned(16))) NnCoarse {
  unsigned long long mask;   // occupied fine cells, bit x | y << 2 | z << 4
  int base;                  // rank (in key order) of the first occupied fine cell: index into cstart
  int pad;
};
struct NnGrid {
  DevBuf<float4> sorted;                   // target points ordered by (L2 cell, coarse sub-cell, fine sub-cell)
  DevBuf<NnCoarse> coarse;                 // [L2 cell * 64 + coarse sub-cell]
  DevBuf<unsigned long long> occ2;         // [L2 cell] occupied coarse cells
  DevBuf<int> cstart;                      // first point of every occupied fine cell, in key order; entry [runs] = n
  DevBuf<uint32_t> keys, keys_alt, vals, vals_alt, run_keys;   // run_keys is kept: the next build clears exactly those cells
  DevBuf<int> run_counts, scalars;         // scalars[0] = number of runs
  DevBuf<NnGridParams> params;
  DevBuf<unsigned> hist;
  // query side: squared NN distance per query of a batch, the two queues of still-open queries {query number, best so far}
  DevBuf<float> dist, q_best;
  DevBuf<unsigned> q_items;
  DevBuf<int> q_count;
  DevBuf<double> hook;   // 128-byte staging block of the test hook
  int64_t n = 0, n_prev = 0;
  bool valid = false;
  void release() {
    sorted.release(); coarse.release(); occ2.release(); cstart.release(); keys.release(); keys_alt.release(); vals.release(); vals_alt.release();
    run_keys.release(); run_counts.release(); scalars.release(); params.release(); hist.release();
    dist.release(); q_best.release(); q_items.release(); q_count.release(); hook.release();
    n = n_prev = 0; valid = false;
  }
};

// A cloud resident in HBM with everything derived from the points alone: the exact-NN index and (GICP) the regularised
// k-NN covariances.  Owned by a handle (setInputTarget / setInputSource copies) or by a dgs_cloud object that outlives
// many registrations (keyframe clouds of the loop detector).
struct CloudState {
  DevBuf<float4> pts;
  int64_t n = 0;
  Bvh bvh;
  DevBuf<double> cov;  // 6 doubles per point: xx, xy, xz, yy, yz, zz
  bool cov_valid = false;
  int cov_k = 0, cov_reg = -1;
  Bvh walk;            // ICP_HIP / GICP_HIP (batch_rounds.h ensure_walk_order): a Hilbert-ordered index kept for the correspondence walk when `bvh` is k-d ordered (the cloud was a batch target)
  DevBuf<double> pcov; // GICP_HIP: pcl::GeneralizedIterativeClosestPoint's covariances, 9 doubles per point (row-major), keyed by (k, epsilon)
  bool pcov_valid = false;
  int pcov_k = 0;
  double pcov_eps = 0.0;
  void invalidate() { bvh.valid = false; cov_valid = false; walk.valid = false; pcov_valid = false; }
  void release() {
    pts.release(); cov.release(); pcov.release(); bvh.release(); walk.release();
    n = 0;
    invalidate();
  }
};

// PrefilteringNodelet::cloud_callback (prefilter.hip): the chain's stage buffers, its own NN index and k-NN lists, and what the test
// hooks read back.  Separate from everything a registration uses.
struct PfScratch {
  DevBuf<float4> in, a, b, c, d, e;    // staged host input; distance / down-sampling / outlier / height / flatten outputs
  DevBuf<unsigned char> flags;         // keep flag per point of the pass being compacted
  DevBuf<int> blk;                     // per-workgroup kept counts, scanned in place to offsets
  DevBuf<int> cnt;                     // [0] kept points of the last compaction
  CloudState cloud;                    // cloud of the k-NN pass being run (radius, statistical, normal) with its index
  DevBuf<int> nbr;                     // its k-NN lists: [position in index order * 32 + slot]
  DevBuf<float> mean_d;                // statistical pass: mean neighbour distance per point (input order)
  DevBuf<double> stats;                // statistical pass: mean, stddev, threshold, variance
  int64_t stat_n = 0;
  DevBuf<float4> normals;              // normal pass: normalised flipped normal per point (input order)
  DevBuf<float> cov9;                  // normal pass: computeMeanAndCovarianceMatrix's 9 floats per point
  int64_t normal_n = 0;
};

// MapCloudGenerator::generate (map_cloud.hip): the keyframe / chunk tables, the chunk boxes, the key table and the last map.
// Separate from everything a registration or the prefilter uses.
struct McFrame;   // map_cloud.hip
struct McChunk;
struct McEpoch;
struct McScratch {
  DevBuf<float4> in;                   // staged host input, all keyframes back to back
  DevBuf<McFrame> frames;              // per keyframe: points, size, float pose
  DevBuf<McChunk> chunks;              // per chunk of a keyframe: keyframe, first point, points
  DevBuf<float> boxes;                 // per chunk: transformed min3, max3, finite points, pad
  DevBuf<McEpoch> epochs;              // growth replay: per run of points inserted under one box, its min and the later key offsets
  DevBuf<int> found;                   // [0] running minimum of the find-first pass; [4..7] its result: index, x, y, z (bit-cast)
  DevBuf<unsigned long long> table;    // open-addressing key table / all keys of the sort path
  DevBuf<unsigned long long> keys, keys_alt;   // unique keys, unsorted and sorted
  DevBuf<long long> cnt;               // [0] selected keys, [1] table overflow flag
  DevBuf<unsigned char> temp;          // rocPRIM temporary storage
  DevBuf<float4> out;                  // the last map
  int64_t n_out = 0;
  double bb_min[3] = {0, 0, 0}, bb_max[3] = {0, 0, 0};
  int depth = 0, growths = 0;
  int find_launches = 0;               // find-first launches of the last map (growth events + the first point + stale boxes)
  int used_sort = 0;                   // the last map took the sort path
};

// LineBasedScanmatcher::line_extraction (line_extraction.hip): the two round clouds, the hypotheses of a round and what sac.h's kernels
// need around them (SacScratch), the inlier / cluster lists, the clustering's sort and union-find arrays, and what the test hook reads back.  Separate from everything
// a registration, the prefilter or the map cloud uses.
struct LnHyp;     // line_extraction.hip
struct LnRound;
struct LnScratch {
  DevBuf<float4> a, b;                 // the remaining points of this round and of the next
  DevBuf<float4> inl, clu, sorted;     // inliers / cluster members (w = position in the round's cloud); inliers in projection order
  DevBuf<unsigned char> flags, cflags; // inlier / keep flag per point; cluster flag per point
  DevBuf<int> blk, cnt;                // compaction offsets; [0] inliers, [1] cluster members, [2] points kept
  SacScratch sac;                      // two point indices per draw; the permutation is the identity between rounds
  DevBuf<LnHyp> hyps;                  // the good draws in order, at most max_iterations + 1
  DevBuf<LnRound> round;
  DevBuf<uint32_t> keys, keys_alt, vals, vals_alt;
  DevBuf<float> sproj;                 // projection on the line per sorted inlier
  DevBuf<int> parent, csize, cminpos;  // union-find over sorted inliers; members and lowest position per root
  DevBuf<unsigned char> temp;          // sort temporary storage
  std::vector<dgs_line_extraction_round> rounds;        // the last extraction
  std::vector<std::vector<int32_t>> inlier_lists, cluster_lists;   // with record_lists
  int64_t counts4[4] = {0, 0, 0, 0};
};

// LineBasedScanmatcher::align_global (line_align.hip): the uploaded lines and edges, one record, gate code and fitness per hypothesis,
// the survivor list and the result record.  Separate from everything a registration, the prefilter, the map cloud or the line
// extraction uses.
struct LaHyp;     // line_align.hip
struct LaResult;
struct LaScratch {
  DevBuf<double> in;                   // source lines, target table, source edges, target edges: one upload
  DevBuf<LaHyp> hyps;                  // per hypothesis h = es * Et + et
  DevBuf<unsigned char> keep, gate;    // survivor flag and gate code per hypothesis
  DevBuf<int> blk, cnt, surv, slot;    // compaction offsets; [0] survivors; survivors' h in order; position in that list per h (-1: gated)
  DevBuf<double> fit;                  // 5 doubles per hypothesis: the four fitness values and the score
  DevBuf<LaResult> result;
  int64_t n_hyp = 0;                   // of the last call: what the test hook may read
  int64_t counts4[4] = {0, 0, 0, 0};   // launches, host waits, hypotheses, survivors
};
// LineBasedScanmatcher::align_local, batched (line_align_local.hip): scratch of its own, nothing shared with align_global's.
struct LalHyp;    // line_align_local.hip
struct LalScratch {
  DevBuf<unsigned char> in;            // one upload: item table, workgroup tables, source lines, target tables, both edge lists
  DevBuf<unsigned char> tab;           // edges_on_device: the item and workgroup tables (`in` then holds source lines, target lines, target tables)
  DevBuf<LalHyp> hyps;                 // per hypothesis of both phases, at the item's offsets
  DevBuf<double> fit;                  // 5 doubles per hypothesis
  DevBuf<double> keys;                 // line pairs: nn_key(real_distance) per (snapshot line, target line)
  DevBuf<double> base;                 // the first phase's aligned lines per item (the snapshot), laid out like the source lines
  DevBuf<unsigned char> out;           // one download: a record per item, then the aligned lines
  std::vector<int64_t> off1, off2;     // of the last call: first hypothesis per item and phase (n_items + 1 entries; phase 1 after all of phase 0)
  int64_t counts8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};
// edge_extraction, batched (line_edges.hip): scratch of its own; the two aligners read `edges` when their edges_on_device is set.
struct LeSeg;     // line_edges.hip
struct LeScratch {
  DevBuf<double> lines;                // the public entry points' upload: 6 doubles per line (the aligners pass their own)
  DevBuf<LeSeg> segs;                  // n_seg + 1 records
  DevBuf<unsigned char> cnt;           // edges (0..4) per pair p = the segment's first pair + i * n + j; 0 for j <= i
  DevBuf<int> blk;                     // edges per workgroup of pairs, scanned in place; [workgroups] = all edges
  DevBuf<int> eoff;                    // first edge per segment, n_seg + 1 entries
  DevBuf<double> edges;                // 9 doubles per edge, all segments back to back
  PinnedBlock stage;                   // the segment table's upload, behind it the edge offsets' download
  std::vector<int> eoff_host;          // of the last extraction
  int64_t counts4[4] = {0, 0, 0, 0};   // launches, host waits, pairs i < j, edges
};
// are_buildings_overlapped over all pairs and align_overlapped_buildings, batched (building_overlap.hip): scratch of its own.
struct BoHyp;     // building_overlap.hip
struct BoScratch {
  DevBuf<unsigned char> in;            // pair search, one upload: line offsets, centres, line end points
  DevBuf<double> shr;                  // x1 y1 x2 y2 of every shrunken line
  DevBuf<unsigned long long> bits;     // pair flags: row i, word j / 64, bit j % 64
  DevBuf<int> row;                     // pairs per row, then their exclusive scan (n_buildings + 1 entries)
  DevBuf<unsigned char> out;           // one download: the count, then the pairs
  DevBuf<unsigned char> ain;           // alignment, one upload: item table, workgroup table, lines, edges
  DevBuf<BoHyp> hyps;                  // per hypothesis of the batch, at the item's offset
  DevBuf<unsigned char> aout;          // one download: a record per item, then the aligned lines
  std::vector<int64_t> off;            // of the last alignment call: first hypothesis per item (n_items + 1 entries)
  int64_t counts8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// What detect() found in one scan, for the single call and for every scan of a batch: the getters of both read it
// (floor_detection.hip fd_get_*).  The single call fills host_filtered and inliers while it runs, the batch when a getter asks.
struct FdScan {
  int64_t n = 0, n_clipped = 0, n_filtered = 0;
  bool have_normals = false, have_host = false, have_inliers = false;
  int32_t status = 1;                  // DGS_FD_TOO_FEW_POINTS
  float coeffs[4] = {0.f, 0.f, 0.f, 0.f};
  dgs_floor_detection_trace trace{};
  std::vector<float4> host_filtered;   // the filtered cloud on the host: the inlier list is made there
  std::vector<int32_t> inliers;
  void reset() {                       // before a detect: nothing found; the host vectors keep their room
    n = n_clipped = n_filtered = 0;
    have_normals = have_host = have_inliers = false;
    status = 1;
    for (float& c : coeffs) c = 0.f;
    trace = dgs_floor_detection_trace{};
    trace.winner_rank = -1;
    trace.sample[0] = trace.sample[1] = trace.sample[2] = -1;
    host_filtered.clear();
    inliers.clear();
  }
};

// FloorDetectionNodelet::detect (floor_detection.hip): the stage clouds, the normal pass's own index and lists, the draw list and
// hypotheses of the RANSAC, and what the getters read back.  Separate from everything a registration, the prefilter, the map cloud
// or the line code uses.
struct FdHyp;     // floor_detection_body.h
struct FdScratch {
  DevBuf<float4> in, tilted, clipped, kept, filtered;   // staged host input; after the tilt; after the clips; after the normal filter; back-transformed
  DevBuf<unsigned char> flags, nflags; // keep flag per point of the pass being compacted; the prefilter rule's flags of pf_normal_kernel (unread)
  DevBuf<int> blk, cnt;                // compaction offsets; [0] kept points of the last compaction
  CloudState cloud;                    // the clipped cloud with its index (normal pass)
  DevBuf<int> nbr;                     // its k-NN lists
  DevBuf<float4> normals;
  DevBuf<float> cov9;
  SacScratch sac;                      // three point indices per draw; the permutation is the identity between detects
  DevBuf<FdHyp> hyps;                  // the good draws in order, at most max_iterations + 1
  FdScan scan;                         // of the last detect
};

// calc_fitness_score over a batch of (cloud1, cloud2, relpose) edges between resident clouds, and the batched Hilbert index build in
// front of it (fitness_batch.hip): tables, keys and rows of its own; everything above is left untouched.
struct FbEdge;    // fitness_batch.hip
struct FbSeg;
struct FbScratch {
  DevBuf<unsigned char> tab;           // walk, one upload: the row prefix (n_edges + 1 ints), then the edge table
  DevBuf<double> rows;                 // one partial row {sum, used} per (edge, slice); then {sum, used} per edge
  PinnedBlock stage;                   // the walk's upload, and behind it the download
  DevBuf<FbSeg> segs;                  // build: per cloud to be indexed, its points, its index arrays and its offsets in the shared arrays
  DevBuf<float> mm;                    // build: per cloud kSegBoxBlocks partial boxes, then the boxes
  DevBuf<unsigned long long> keys, keys_alt;   // build: (cloud number << 30) | hilbert30, all clouds back to back
  DevBuf<uint32_t> vals, vals_alt;     // build: index of the point in its own cloud
  PinnedBlock bstage;                  // the build's upload: marked, nobody waits for it
  int64_t counts8[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // launches, host waits, edges, indices built, partial rows
};

// The buffers of the chain "key per point -> stable radix sort of (key, point index) -> run-length encode -> exclusive scan of the run
// lengths" that every structure keyed by voxel cell is built with (voxel_cells.h runs it).  What a build leaves behind for later calls
// -- the key of every run and the scalar block, scalars[0] = number of runs -- is a RunTable of its own: a chain writes the table its
// caller names, so a call that borrows the rest (dgs_voxel_grid_filter) leaves the NDT model's table alone.
template <class Key>
struct RunTable {
  DevBuf<Key> keys;
  DevBuf<int> scalars;
  void release() { keys.release(); scalars.release(); }
};
template <class Key>
struct KeyRuns {
  DevBuf<Key> keys, sorted_keys;
  DevBuf<uint32_t> vals, sorted_vals;    // index of the point in its cloud; sorted: a run's points in point-index order
  DevBuf<int> run_counts, run_offsets;   // only the first scalars[0] entries, which the run-length encoding writes, are counts
  RunTable<Key> table;
  // n keys, and as many runs at most, into `t` (the caller's own `table`, or another)
  hipError_t reserve(const size_t n, RunTable<Key>& t) {
    hipError_t e = t.scalars.reserve(8);
    for (DevBuf<Key>* b : {&keys, &sorted_keys, &t.keys}) e = e != hipSuccess ? e : b->reserve(n);
    for (DevBuf<uint32_t>* b : {&vals, &sorted_vals}) e = e != hipSuccess ? e : b->reserve(n);
    for (DevBuf<int>* b : {&run_counts, &run_offsets}) e = e != hipSuccess ? e : b->reserve(n);
    return e;
  }
  void release() { keys.release(); sorted_keys.release(); vals.release(); sorted_vals.release(); run_counts.release(); run_offsets.release(); table.release(); }
};

// dgs_cloud_assign_batch (voxel_batch.hip): the staged inputs, one record per cloud, the keys, values and runs of all clouds back to
// back; everything above is left untouched.
struct VbSeg;     // voxel_batch.hip
struct VbScratch {
  DevBuf<float4> in;                   // host inputs, all clouds back to back
  DevBuf<VbSeg> segs;
  DevBuf<float> mm;                    // per cloud 64 partial boxes, then the boxes
  KeyRuns<unsigned long long> runs;    // keys: (cloud number << 32) | cell index
  DevBuf<int> bounds;                  // first run and end of the emitted runs per cloud
  int64_t counts8[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // of the last call: launches, host waits, clouds
};

// interpolate / buildPointCloud / getCloud over many lines (building_cloud.hip): the table of sample positions, kept across calls, and
// scratch of its own; everything above is left untouched.
struct BcScratch {
  bc::StepTable steps;                 // the table on the host: the master copy, grown on demand
  int64_t table_on_device = 0;         // entries of it that `table` holds
  DevBuf<float> table;
  DevBuf<unsigned char> in;            // one upload: header {error line, total}, first line per item, matrix per line, matrices, end points
  DevBuf<float4> rec;                  // per line: a.x, a.y, dn.x, dn.y
  DevBuf<int> cnt;                     // per line: points, scanned in place to the line's first point
  DevBuf<int> item_off;                // first point per item, n_items + 1 entries
  DevBuf<float4> out;                  // the last result
  int64_t n_out = 0, n_items = -1;     // n_items < 0: no result to read
  int64_t counts8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// Batched k-NN covariances of resident clouds (cov_batch.hip): the device tables of a pass's chunks, the pinned block they travel from
// (its own, marked: the handle's pinned block is rewritten by the batch that follows while this upload may still be in flight),
// and the counts of the last pass.
struct CbScratch {
  DevBuf<unsigned char> tables;        // per chunk: entries | first search workgroup per cloud | first covariance workgroup per cloud
  PinnedBlock stage;                   // the tables' upload: marked, nobody waits for it
  int64_t points_budget = 0;           // DGS_COV_BATCH_POINTS (0: covplan::kCovBatchPoints)
  int64_t counts8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// The buffers of the segmented stable compaction over the scans of a stage (compact.h seg_flags / seg_upload / seg_compact)
struct SegCompact {
  DevBuf<unsigned char> flags;         // keep flags, every scan padded to whole workgroups
  DevBuf<int> blk;                     // per-workgroup kept counts of all scans (+ 1), scanned in place
  DevBuf<int> cnt;                     // [0] kept points of all scans
  DevBuf<int> totals;                  // kept points per scan of the stage
  DevBuf<unsigned char> tables;        // the stage's table: entries | heads | first workgroups | first search workgroups
  PinnedBlock stage;                   // the table's upload and the totals' download
  void release() { flags.release(); blk.release(); cnt.release(); totals.release(); tables.release(); stage.release(); }
};

// The prefilter chain over many scans (prefilter_batch.hip): a pool of stage clouds per scan of a chunk, the shared flag / count /
// neighbour arrays of all scans back to back, the stage tables and the pinned block they travel through.  Separate from PfScratch: the
// single call's buffers and hooks are not touched, except that its hooks report n = 0 afterwards.
struct PfbScratch {
  std::vector<CloudState> a, b, c, d, e;   // per scan: distance / down-sampling / outlier / height / flatten outputs (a, b, d carry the indices)
  DevBuf<float4> in;                   // staged host inputs, all scans of a chunk back to back
  SegCompact seg;                      // every stage ends with its compaction's host wait
  DevBuf<int> nbr;                     // k-NN lists of all scans of a stage: [(points before the scan + position in index order) * 32 + slot]
  DevBuf<float> mean_d;                // statistical pass: per point, all scans back to back
  DevBuf<double> stats;                // statistical pass: mean, stddev, threshold, variance per scan
  DevBuf<float4> normals;              // normal pass (the body writes them)
  DevBuf<float> cov9;
  std::vector<double> stats_host;      // of the last call: {mean, stddev, threshold, points} per scan
  int64_t points_budget = 0;           // DGS_PREFILTER_BATCH_POINTS (0: pfbplan::kBatchPoints)
  int64_t counts8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// dgs_floor_detection_batch (floor_detection_batch.hip): detect() over many scans in one chain.  Per scan the clipped cloud with its
// index, its normals and its filtered cloud stay on the device until the next batch; the getters read them by scan number.  The normal
// stage runs in a PfbScratch of the batch's own (prefilter_batch_normal_stage).  Separate from FdScratch: the single call's buffers and
// getters are not touched.
struct FdbScratch {
  std::vector<CloudState> clip;        // per scan: the clipped cloud and (normal filter) its index
  std::vector<DevBuf<float4>> normals, filtered;   // per scan
  std::vector<FdScan> scans;           // of the last batch
  PfbScratch nrm;                      // the normal stage's index build, lists, tables and pinned block
  DevBuf<float4> in, tilted, kept;     // staged host inputs; after the tilt; after the normal filter: all scans of a chunk back to back
  SegCompact seg;                      // the filter stages' flags, counts, tables and pinned block
  DevBuf<unsigned char> sac_tables;    // the RANSAC's table: entries | first tiles
  PinnedBlock sac_stage;               // its upload, the draw lists behind it, and where meta, counts and hypotheses come down
  DevBuf<int> draws, counts, meta;     // per live scan: its draw list; max_hyp counts; 4 ints of meta
  DevBuf<FdHyp> hyps;                  // per live scan max_hyp records
  SacScratch sac;                      // mt19937 values and the identity permutation; the device buffers of a scan finished alone
  DevBuf<FdHyp> hyps_single;           // that scan's hypotheses
  dgs_floor_detection_params params{}; // of the last batch: the getters' inlier rule
  int64_t points_budget = 0;           // DGS_FLOOR_BATCH_POINTS (0: fdplan::kBatchPoints)
  int64_t counts8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

}  // namespace dgs

struct dgs_handle;
struct dgs_cloud {
  dgs::CloudState st;
  int device = 0;
  std::vector<dgs_handle*> users;  // handles whose tgt/src point at st: detached again when the cloud is destroyed first
};

struct dgs_handle {
  dgs_params prm;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipEvent_t ev_poll[2] = {nullptr, nullptr};  // chunk-boundary events of the optimiser loops (created on first use)
  // side stream: small builds that the main stream does not need yet (the target's NN index while the batch iterates)
  hipStream_t side_stream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // third stream: the double-precision computeHessian launches of the upstream order run beside the main stream's launches (ndt_strict.h)
  hipStream_t hd_stream = nullptr;
  static constexpr int kHdEvents = 32;
  hipEvent_t ev_hd_a[kHdEvents] = {}, ev_hd_b[kHdEvents] = {};
  int strict_kernel = 3;              // DGS_NDT_STRICT_KERNEL: upstream-order kernels: 3 item-compacted (one launch per round), 2 lane-per-point (two launches per round)
  bool hd_overlap = true;             // DGS_NDT_HD_OVERLAP=0: the computeHessian launch of a round in line with the round's first launch
  bool ndt_speculate = true;          // DGS_NDT_SPECULATE=0: upstream order, item-compacted kernel: the Newton step's Jacobi SVD in the closing workgroup instead of speculated
  bool ndt_fixed_slices = false;     // DGS_NDT_FIXED_SLICES=1: upstream order, item-compacted kernel: a pair's slices are a function of its own size (ndt_strict.h strict_slices_of)
                                      // from the Gauss-Jordan direction and verified beside the next launch (NdtPair::spec_s)
  bool ndt_fixed_slices_initial = false;   // ndt_fixed_slices as dgs_create left it
  bool batch_independent = false;     // dgs_set_batch_independent: FAST_GICP / FAST_VGICP sum a pair over slices that follow its own size (gicp.hip, the FIXED round kernels), NDT order 1
                                      // takes ndt_fixed_slices with it, and every fitness goes through the edge scorer (fitness_batch.hip): a pair's record does not depend on its batch
  bool ndt_deal_by_cost = true;       // DGS_NDT_DEAL_BY_COST=0: upstream order, item-compacted kernel: a launch's workgroups dealt to the pairs in index order (deal_workgroup)
  bool ndt_reuse_trials = true;       // DGS_NDT_REUSE_TRIALS=0: upstream orders: a repeated More-Thuente trial pose is evaluated again and its result replaced by the cached one
                                      // instead of heaviest evaluation kind first (deal_workgroup_by_cost); the same (pair, slice) set and the same bits either way
#ifdef DGS_DEAL_STAMPS
  unsigned long long* deal_stamps = nullptr;   // stamp build (make stamps): the workgroup stamps of the recorded launches
  long long deal_stamp_seq = 0;                // item-kernel launches issued by this handle
#endif
  int solve_min_active = 0;           // DGS_NDT_SOLVE_MIN_ACTIVE (default 0 = the Newton step stays in the closing workgroup): item-compacted upstream-order kernel:
                                      // with at least this many pairs in a launch the Newton steps go to ndt_strict_solve_kernel on the third stream.  Measured on the
                                      // bench step: 6.58-6.65 ms with 2 / 4 / 8 / 16 against 6.24 ms in line -- a pair sits out a round per iteration, and the closings'
                                      // ~45 us chains were already hidden behind the other pairs' derivative work
  bool side_pending = false;
  bool side_build_deferred = false;   // forked, launches still to be enqueued (side_build_now)
  std::string err;

  // clouds (pcl::PointXYZ layout): the handle's own copies, or borrowed dgs_cloud objects
  dgs::CloudState own_target, own_source;
  dgs::CloudState* tgt = &own_target;
  dgs::CloudState* src = &own_source;
  dgs_cloud* tgt_cloud = nullptr;  // non-null while tgt / src borrow a dgs_cloud
  dgs_cloud* src_cloud = nullptr;
  int64_t nt = 0, ns = 0;
  bool have_target = false, have_source = false;

  // ---- NDT target model
  dgs::VoxelGrid grid{};
  dgs::DevBuf<int> cell2vox;
  dgs::DevBuf<dgs::VoxelRec> vox;
  dgs::DevBuf<float4> vox_centroid;
  dgs::DevBuf<double> vox_dbg;       // per occupied voxel: mean[3], icov[9]  (test hook; double-precision computeHessian pass)
  dgs::DevBuf<dgs::VoxelStrictRec> vox_strict;   // per occupied voxel: mean, float(icov) 3 x 3 (upstream evaluation orders)
  dgs::DevBuf<int> vox_count;        // points per occupied voxel
  dgs::DevBuf<int> vox_valid;
  dgs::KeyRuns<uint32_t> runs;       // runs.table: the model's run keys and scalars, [0]=num_runs, [1]=n_valid
  dgs::RunTable<uint32_t> vg_table;  // dgs_voxel_grid_filter's own runs / scalars: the NDT model's (above) stay what setInputTarget made them
  dgs::DevBuf<float> minmax_partial; // block partials + final 6 floats
  dgs::DevBuf<unsigned char> cub_temp;
  int64_t grid_cells = 0;
  int64_t n_occupied = 0, n_valid = 0;  // filled lazily by counts query
  int64_t n_occupied_bound = 0;         // target points of the voxel model = an upper bound of its occupied voxels (known without a device round trip)
  bool counts_stale = true;

  // ---- NDT optimiser
  dgs::DevBuf<dgs::NdtPair> pairs;
  dgs::DevBuf<dgs::NdtInit> inits;
  dgs::DevBuf<double> partials;       // [pair][block][kAccumPad]
  dgs::DevBuf<int> done_counter;      // [0] = finished pairs
  int* done_flags = nullptr;          // pinned host memory, device-visible: one "finished" flag per pair of the running fused NDT batch
  int done_flags_cap = 0;
  dgs::DevBuf<int> ndt_queue;         // queue kernel: 16 control ints, then one 64-byte line per pair (its queue word)
  dgs::DevBuf<unsigned char> ndt_ring;   // queue kernel: one 384-byte record slot per pair and round (ndt_align.hip, kQueueSlotBytes)
  int ndt_ring_rounds = 0;
  int ndt_queue_mode = 0;             // DGS_NDT_QUEUE=1 (experiments build): the persistent queue kernel instead of one launch per evaluation (measured slower)
  bool ndt_schedule = false;          // DGS_NDT_SCHEDULE=1 (tests): the launch-per-evaluation path cuts every round like the queue kernel would
  int ndt_queue_min_pairs = 2;        // DGS_NDT_QUEUE_MIN_PAIRS: batches smaller than this keep the launch-per-evaluation path
  dgs::DevBuf<int> pair_blocks;       // slices the last derivative launch gave each pair
  dgs::DevBuf<double> strict_rows;    // ndt_strict_order 2: per-point totals, [pair][43][max_n] (column-major per pair)
  dgs::DevBuf<double> strict_totals;  // ndt_strict_order 1/2: [pair][kStrictPad] sums of one evaluation
  dgs::DevBuf<const float4*> src_ptrs;
  dgs::DevBuf<int> src_sizes;
  dgs::NdtConsts consts{};
  int64_t last_evaluations = 0;
  int64_t last_reused = 0;            // NDT, upstream orders: trial poses of the last align / batch found in the line search's cache (dgs_get_counts slot 6)
  dgs::DevBuf<int> knn_nbr;           // k-NN sets of the cloud whose covariances are being made: [position in Hilbert order * stride + slot], stride 32 (k <= 32) or 64
  dgs::DevBuf<int> knn_stats;         // debug build (-DDGS_KNN_STATS): waves, waves on the cooperative path, candidate leaves
  bool nn_kd = true;                  // DGS_NN_KD=0: Hilbert order also for the loop batch's target index
  int64_t nn_kd_min_queries = 6 * 65536;   // DGS_NN_KD_MIN_QUERIES: source points of a batch from which its target index is built k-d ordered
  bool nn_kd_all = false;             // DGS_NN_KD_ALL=1: every target index is k-d ordered (tests of the k-d build through the single-query hooks)
  bool batch_kd = false;              // set by dgs_align_batch* around its work: the target index it builds is k-d ordered
  int knn_parts = 0;                  // DGS_KNN_PARTS: waves per leaf in gicp_knn_leaf_kernel (0 = by cloud size)
  bool knn_leaf = true;               // DGS_KNN_LEAF=0: the per-query k-NN walk (gicp_knn_kernel) instead of the wave-per-leaf search
  bool knn_leaf_wide = true;          // DGS_KNN_LEAF_WIDE=0: the per-query walk (gicp_knn_wide_kernel) for 32 < k <= 64 instead of the wave-per-leaf search
  int knn_min_waves = 4096;           // DGS_KNN_MIN_WAVES: ... but never fewer waves than this (4 per SIMD)
  int knn_rounds = 8;                 // DGS_KNN_ROUNDS: rounds of 8 adjacent queries per wave in gicp_knn_kernel (1 = no warm bounds)
  bool gicp_fused = true;             // DGS_GICP_FUSED=0: the optimiser step of FAST_GICP / FAST_VGICP as its own launch (gicp_solve_kernel)
  bool ndt_pack2 = false;             // DGS_NDT_PACK2=1: DIRECT7 derivatives with two points per lane on packed FP32 (A/B measurements)
  bool ndt_fused = true;              // DGS_NDT_FUSED=0 at dgs_create: (derivatives, solve) launch pairs instead of fused launches

  // pinned host staging
  void* pinned = nullptr;
  size_t pinned_bytes = 0;

  // last result (single-pair API)
  float final_T[16];
  bool have_result = false;

  dgs::DevBuf<double> nn_partials;
  int nn_bpp = 0;                   // rows (workgroups) per pair of the fitness batch being prepared / walked
  double* fit_host = nullptr;       // pinned: the totals of the last fitness batch ({sum, count, inliers, 0} per pair)
  int fit_host_cap = 0;
  // dgs_align_batch -> ndt_align_pairs: walk the fitness of the candidates that have finished on the side stream while the rest iterate
  struct EarlyFitness {
    bool on = false;        // wanted for the batch being aligned
    bool enqueued = false;  // ndt_align_pairs has enqueued every pair's walk, the totals and their copy: read fit_host after its sync
    double max_range = 0.0;
    int max_n = 0;
    int lds_kb = 0;         // DGS_EARLY_FITNESS_LDS_KB: occupancy cap of the side-stream walks (workgroups per CU = 160 / this; 0 = none)
    int max_active = 1 << 30;   // DGS_EARLY_FITNESS_MAX_ACTIVE: side-stream walks start once at most this many pairs still iterate
    int min_pairs = 8;      // DGS_EARLY_FITNESS_MIN_PAIRS: a side-stream launch waits until this many finished pairs are ready
  } early_fit;
  // DGS_EARLY_FITNESS=1.  Off by default: measured on the bench workload (scripts/ab_early_fitness.sh, profiles/r03/early_fitness_ab.txt)
  // it never beat the plain order -- 2.19-2.22 ms per step against 2.15 at best (8+ pairs per launch, no occupancy cap), 2.4-3.3 ms with
  // the cap, 4.3 ms with a launch per finished pair.  A walk's workgroup lives ~100 us whatever the launch holds, so (i) a launch per
  // few pairs leaves the chip as empty as the tail it was meant to fill, (ii) a large launch floods every slot and the iteration
  // launch that arrives next waits one workgroup lifetime (35 -> 90-120 us in the trace), (iii) capped to 1-2 workgroups per CU the
  // walk is several times slower and the end of the batch waits for it.
  bool early_fitness_enabled = false;
  const double* nn_out = nullptr;   // device: {sum, count, inliers, 0} per pair of the last fitness batch (inside nn_partials; read by dgs_group's record kernel)
  dgs::DevBuf<float4> scratch_cloud;
  dgs::NnGrid tgt_grid, aux_grid;   // fitness-pass index over the current target / over cloud1 of dgs_calc_fitness_score
  int grid_mode = 0;                // DGS_NN_GRID at dgs_create: 0 (default) tree walk only, >= 1 grid pass in front of it, -1 grid pass for big batches.
                                    // Measured on the 32 x 65,536 bench step: the grid pass cuts the fitness kernels from 0.83 to 0.69 ms, but
                                    // its build and queue traffic give the gain back (2.99 vs 3.00 ms per step), so it stays opt-in.
  bool use_grid = false;            // decision for the current target (grid_wanted)
  int grid_levels = 1;              // DGS_NN_GRID=2: also the coarse-block pass between the fine-block pass and the tree
  float grid_spacing_factor = 6.f;  // DGS_NN_GRID_FACTOR: fine cell = factor x 2^floor(log2(median spacing))

  // ---- calc_fitness_score between two arbitrary clouds (InformationMatrixCalculator): own buffers, the registration's
  // target / source / result are left untouched
  dgs::DevBuf<float4> aux_cloud1, aux_cloud2, aux_out;
  // dgs_find_loop_candidates: staging kept across calls ([accum n | xy 2n], indices, count) -- the call is made every graph update
  dgs::DevBuf<double> fc_in;
  dgs::DevBuf<int> fc_out;
  dgs::DevBuf<long long> fc_cnt;
  dgs::Bvh aux_bvh;
  int64_t bvh_builds = 0;           // bvh_build calls that built something, since dgs_create (dgs_fitness_batch_get_counts: who built an index is observable)

  // ---- GICP (fast_gicp::FastGICP): k-NN covariances of both clouds, correspondences, Mahalanobis matrices
  dgs::DevBuf<int> corr;
  dgs::DevBuf<float> corr_sq;
  dgs::DevBuf<double> mahal;                   // 6 doubles per source point
  dgs::DevBuf<dgs::GicpPair> gpairs;
  dgs::DevBuf<dgs::GicpItem> gitems;
  dgs::DevBuf<dgs::GicpTarget> gtargets;       // gicp_align_pairs: one entry per distinct target cloud of the call
  // FAST_VGICP target model
  dgs::VgicpMap vmap{};
  dgs::DevBuf<dgs::VgicpVoxel> vvox;
  dgs::DevBuf<int> vcell2vox;
  bool vmap_valid = false;
  int64_t vmap_voxels = 0;
  dgs::DevBuf<float4> batch_slab;              // host sources of dgs_align_batch staged as one slab (kept across calls)
  std::vector<dgs::CloudState> batch_clouds;   // index + covariances of sources handed to dgs_align_batch as raw arrays
  dgs::GicpConsts gconsts{};

  // ---- fixed slices of ICP_HIP / GICP_HIP round launches (batch_rounds.h SliceTable, slice_rows.h): one set, a handle has one method for life
  dgs::DevBuf<int> slice_blk_pair;             // workgroup -> pair of the round launch
  dgs::DevBuf<double> slice_rows;              // one partial row per (pair, slice): kIcpPad / kPgPad doubles

  // ---- ICP (pcl::IterativeClosestPoint, icp.hip): the target's exact-NN index only -- no covariances, for the target or any source
  dgs_icp_options icp_opt{};                   // dgs_set_icp_options; read at every align
  dgs::DevBuf<dgs::IcpPair> ipairs;
  dgs::DevBuf<dgs::IcpItem> iitems;
  dgs::DevBuf<float4> icp_w;                   // working copies (input_transformed) of every source of the batch
  dgs::DevBuf<int> icp_origin;                 // index of the target's first finite point (the origin of the moment sums)
  dgs::DevBuf<float> icp_traj_T;               // per pair and iteration: T_k (column-major 16 floats)
  dgs::DevBuf<double> icp_traj_mse;
  dgs::DevBuf<int> icp_traj_n;
  std::vector<dgs::Bvh> icp_w_bvh;             // reciprocal mode: index over each working copy, rebuilt every round
  std::vector<int> icp_last_iters;             // iterations per pair of the last align / batch (dgs_icp_get_trajectory)
  int icp_traj_cap = 0;

  // ---- GICP_HIP (pcl::GeneralizedIterativeClosestPoint, pcl_gicp.hip): PCL-style covariances of target and sources (CloudState::pcov)
  dgs_pcl_gicp_options pg_opt{};               // dgs_set_pcl_gicp_options; read at every align
  dgs::DevBuf<dgs::PgPair> pgpairs;
  dgs::DevBuf<dgs::PgItem> pgitems;
  dgs::DevBuf<dgs::PgInit> pginits;
  dgs::DevBuf<dgs::PgTarget> pgtargets;        // pcl_gicp_align_pairs: one entry per distinct target cloud of the call
  dgs::DevBuf<float4> pg_w;                    // per source slot (walk order): output = guess * source, w = original index
  dgs::DevBuf<float4> pg_q;                    // per source slot: the target point of this outer iteration's pair, w = 1 kept / 0 not
  dgs::DevBuf<double> pg_m;                    // per source slot: M_i, 9 planes of doubles (structure of arrays)
  dgs::DevBuf<float> pg_traj_T;                // per pair and outer iteration: transformation_ (column-major 16 floats)
  dgs::DevBuf<int> pg_traj_i;                  // per pair and outer iteration: kept pairs, inner iterations, evaluation passes
  dgs::DevBuf<double> pg_traj_f;
  std::vector<int> pg_last_iters;              // outer iterations per pair of the last align / batch (dgs_pcl_gicp_get_trajectory)
  int pg_traj_cap = 0;
  float pg_probe_T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};       // dgs_pcl_gicp_set_probe: transformation_, column-major
  float pg_probe_guess[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};   // and the guess

  // ---- prefilter (prefilter.hip): own buffers and index; the registration's target / source / model / results are left untouched
  dgs::PfScratch pf;

  // ---- map cloud (map_cloud.hip): own buffers; registration and prefilter state are left untouched
  dgs::McScratch mc;

  // ---- line extraction (line_extraction.hip): own buffers; registration, prefilter and map cloud state are left untouched
  dgs::LnScratch ln;
  dgs::LaScratch la;
  dgs::LalScratch lal;
  dgs::LeScratch le;
  dgs::BoScratch bo;

  // ---- floor detection (floor_detection.hip): own buffers; everything above is left untouched
  dgs::FdScratch fd;

  // ---- batched calc_fitness_score between resident clouds (fitness_batch.hip): own buffers; everything above is left untouched
  dgs::FbScratch fb;

  // ---- building clouds (building_cloud.hip): own buffers and the table of sample positions; everything above is left untouched
  dgs::BcScratch bcl;

  // ---- batched down-sampling into resident clouds (voxel_batch.hip): own buffers; everything above is left untouched
  dgs::VbScratch vb;

  // ---- batched k-NN covariances (cov_batch.hip): the chunk tables and their staging; the neighbour table is knn_nbr
  dgs::CbScratch cb;

  // ---- the prefilter over many scans (prefilter_batch.hip): own buffers and indices; PfScratch and everything above is left untouched
  dgs::PfbScratch pfb;
  dgs::FdbScratch fdb;

  dgs::Profiler prof;
};

namespace dgs {

// profiling wrappers (dgs_api.hip)
int prof_begin(dgs_handle* h, int kernel_id, hipStream_t st = nullptr);   // st: default the handle's stream
void prof_end(dgs_handle* h, int kernel_id, int slot, hipStream_t st = nullptr);
void prof_end_counted(dgs_handle* h, int kernel_id, int slot, int count);   // one bracket that stands for `count` passes: its time once, the count advanced by `count`
int ensure_pinned(dgs_handle* h, size_t bytes);
// dgs_api.hip: n host inputs (float4 points) into `slab` back to back, on the handle's stream, in order; d_in[i]: where input i stands.
// Pageable memory: each copy has left the caller's array when it returns.
int stage_host_inputs(dgs_handle* h, DevBuf<float4>& slab, int n, const float* const* inputs, const int64_t* sizes, const float4** d_in);
int ensure_poll_events(dgs_handle* h);
int side_fork(dgs_handle* h);   // side_stream continues from what the main stream has enqueued so far
int side_join(dgs_handle* h);   // the main stream waits for what side_fork()'s work (no-op when nothing is pending)
int side_build_now(dgs_handle* h);   // enqueues the deferred build of the target's NN index on the side stream

// ndt_voxel.hip
int ndt_build_target(dgs_handle* h);
int voxel_grid_filter(dgs_handle* h, const float4* in, int64_t n, float leaf, float4* out, int64_t out_capacity, int64_t* n_out);
int approx_voxel_grid_filter(dgs_handle* h, const float4* in, int64_t n, float leaf, float4* out, int64_t out_capacity, int64_t* n_out);   // pcl::ApproximateVoxelGrid
int cloud_minmax(dgs_handle* h, const float4* pts, int64_t n, float out6[6]);
int cloud_minmax_device(dgs_handle* h, const float4* pts, int64_t n, float** d_out6, hipStream_t st = nullptr);
// ndt_align.hip
int ndt_align_pairs(dgs_handle* h, int n_pairs, const float4* const* d_src_ptrs_host, const int* sizes_host,
                    const float* guesses16, dgs_result* results);
int ndt_trajectory(dgs_handle* h, int pair, double* out, int* len);
int ndt_probe(dgs_handle* h, const double* p6, const float* T16, double* score, double* g6, double* H36, int kind = 1);   // kind 2: the double-precision computeHessian pass
int strict_row_probe(dgs_handle* h, const double* totals, int ncol, double* rows2);   // dgs_strict_row_probe
// pcl_ndt.hip (DGS_METHOD_PCL_NDT): the evaluation kernel of pcl::NormalDistributionsTransform, launched by ndt_align.hip's driver in place of its own
inline bool is_pcl_ndt(const dgs_handle* h) { return h->prm.method == DGS_METHOD_PCL_NDT; }
inline bool is_ndt_family(const dgs_handle* h) { return h->prm.method == DGS_METHOD_NDT || h->prm.method == DGS_METHOD_PCL_NDT; }   // voxel model, NDT driver, NDT hooks
void pcl_ndt_launch(dgs_handle* h, int n_pairs, int cap_blocks, int total_blocks, int launch, hipStream_t st);   // launch >= 0: fused round; < 0: rows only
void pcl_ndt_init_tables(dgs_handle* h, int n_pairs, hipStream_t st);
int pcl_ndt_neighbours(dgs_handle* h, const float* queries_xyz16, int64_t m, int on_device, int32_t* counts, int32_t* voxel_ids);
// nn_bvh.hip
int bvh_build(dgs_handle* h, Bvh& bvh, const float4* pts, int64_t n, hipStream_t st = nullptr, bool kd_order = false);  // st: default the handle's stream; kd_order: median-split order (slower build, faster queries)
int nn_fitness(dgs_handle* h, const float4* src, int64_t n, const float* T16, double max_range, double inlier_sq,
               double* sum, int64_t* count, int64_t* inliers);
// batched: device arrays of source pointers / sizes, device transforms (column-major 16 floats every T_stride_bytes)
int nn_fitness_batch(dgs_handle* h, int n_pairs, const float4* const* d_src_ptrs, const int* d_sizes, int max_size, const float* d_T,
                     size_t T_stride_bytes, double max_range, double inlier_sq, double* sums, int64_t* counts, int64_t* inliers);
int nn_fitness_batch_on(dgs_handle* h, const Bvh& index, NnGrid* grid, int n_pairs, const float4* const* d_src_ptrs, const int* d_sizes, int max_size,
                        const float* d_T, size_t T_stride_bytes, double max_range, double inlier_sq, double* sums, int64_t* counts, int64_t* inliers);
int nn_fitness_prepare(dgs_handle* h, int n_pairs, int max_size, bool grid);
// ids: `count` pair indices (< 65,536) to walk, or nullptr for pairs 0 .. count - 1
void nn_fitness_enqueue(dgs_handle* h, hipStream_t st, const Bvh& index, const int* ids, int count, const float4* const* d_src_ptrs, const int* d_sizes,
                        const float* d_T, size_t T_stride_bytes, double max_range, double inlier_sq, int background_lds_kb);
int nn_fitness_totals_enqueue(dgs_handle* h, int n_pairs);
void nn_fitness_read(const dgs_handle* h, int n_pairs, double* sums, int64_t* counts, int64_t* inliers);
int nn_search(dgs_handle* h, const float4* queries, int64_t m, int32_t* d_idx, float* d_sq);
int ensure_target_index(dgs_handle* h, hipStream_t st = nullptr);   // tree (+ grid when h->use_grid) over the current target
// the grid pass pays for its build (one more sort of the target) from ~4 x 65,536 queries on: fitness of a candidate batch
inline bool grid_wanted(const dgs_handle* h, int64_t queries) { return h->grid_mode > 0 || (h->grid_mode < 0 && queries >= 262144); }
// nn_grid.hip -- the one-lane-per-query voxel-hierarchy fitness index: measured slower than the 8-lane tree walk, so it
// is part of the EXPERIMENTS build only (`make experiments` -> libdgs_reg_exp.so, -DDGS_EXPERIMENTS); the product library does not
// carry its kernels and ignores DGS_NN_GRID.
#ifdef DGS_EXPERIMENTS
constexpr bool kExperiments = true;
int nn_grid_build(dgs_handle* h, NnGrid& G, const Bvh& bvh, const float4* pts, int64_t n, hipStream_t st = nullptr);
int nn_grid_launch_fitness(dgs_handle* h, NnGrid& G, const Bvh& index, int n_pairs, const float4* const* d_src_ptrs, const int* d_sizes, int max_n, const float* d_T,
                           size_t T_stride_bytes, float max_range, float inlier_sq, double* partial, int bpp);
int nn_grid_search(dgs_handle* h, NnGrid& G, const Bvh& index, const float4* queries, int64_t m, float* d_sq);
#else
constexpr bool kExperiments = false;
inline int nn_grid_build(dgs_handle*, NnGrid&, const Bvh&, const float4*, int64_t, hipStream_t = nullptr) { return DGS_ERR_UNSUPPORTED; }
inline int nn_grid_launch_fitness(dgs_handle*, NnGrid&, const Bvh&, int, const float4* const*, const int*, int, const float*, size_t, float, float, double*, int) { return DGS_ERR_UNSUPPORTED; }
inline int nn_grid_search(dgs_handle*, NnGrid&, const Bvh&, const float4*, int64_t, float*) { return DGS_ERR_UNSUPPORTED; }
#endif
// gicp.hip
int vgicp_build_map(dgs_handle* h);  // vgicp_voxel.hip: needs the target covariances
int vgicp_voxels(dgs_handle* h, int64_t capacity, int32_t* coord3, int32_t* counts, double* mean3, double* cov9, int64_t* n_voxels);
int gicp_align(dgs_handle* h, const float* guess16, dgs_result* out);
int gicp_align_batch(dgs_handle* h, int n, CloudState* const* srcs, const float* guesses16, dgs_result* out);
int gicp_align_pairs(dgs_handle* h, int n, dgs_cloud* const* tgts, dgs_cloud* const* srcs, const float* guesses16, dgs_result* out);   // pair i against tgts[i]
const float* gicp_final_transforms(dgs_handle* h, size_t* stride_bytes);
int gicp_probe(dgs_handle* h, const double* T16_rowmajor, int error_only, double* err, double* H36, double* b6);
// gicp_cov.hip: FAST_GICP / FAST_VGICP covariances of a cloud under the handle's (k, regularisation), cached on the cloud
int ensure_covariance(dgs_handle* h, CloudState& c);
int gicp_covariances(dgs_handle* h, int which, double* host_out6, int64_t n);
// cov_batch.hip: the covariances of many clouds (indices built) under the handle's key, in one search and one covariance launch per chunk.
// kind: covplan::kFast (CloudState::cov, what ensure_covariance makes) or covplan::kPcl (CloudState::pcov, what ensure_pcov makes) -- the same bits.
int ensure_covariances(dgs_handle* h, int n, CloudState* const* clouds, int kind);
int cloud_build_covariances(dgs_handle* h, int n, dgs_cloud* const* clouds);   // dgs_cloud_build_covariances behind its argument checks
void cov_batch_release(dgs_handle* h);
// gicp_cov_ordered.hip: covariances in upstream's operation order (dgs_params.gicp_cov_jacobi_svd = DGS_GICP_COV_UPSTREAM_ORDER) from knn_lists' sets
struct BvhView;
int gicp_cov_upstream_order(dgs_handle* h, const BvhView& v, CloudState& c, int k, int regularization, const int* nbr, int stride);
// icp.hip
int icp_align(dgs_handle* h, const float* guess16, dgs_result* out);
int icp_align_batch(dgs_handle* h, int n, CloudState* const* srcs, const float* guesses16, dgs_result* out);
const float* icp_final_transforms(dgs_handle* h, size_t* stride_bytes);
int icp_trajectory(dgs_handle* h, int pair, float* T16s, double* mse, int32_t* n_corr, int capacity, int* len);
void icp_release(dgs_handle* h);
// knn_lists.hip: exact k-NN lists of a cloud in itself -> h->knn_nbr
// out: default h->knn_nbr; stride: where the table's stride goes (kKnnMax or, k > 32, kKnnMaxWide) -- without it k <= 32 and the stride is kKnnMax
int knn_lists(dgs_handle* h, CloudState& c, int k, DevBuf<int>* out = nullptr, int* stride = nullptr);
bool knn_uses_leaf_search(const dgs_handle* h, int k);   // whether knn_lists serves k with the wave-per-leaf search (the DGS_KNN_STATS printout asks)
// the two widths of the k-NN lists (nn_group.h): slots per lane of the 8-lane group; the table's stride, which is the largest k of that width
constexpr int kKnnSlots = 4, kKnnMax = kKnnSlots * 8;               // k <= 32: every consumer of the lists
constexpr int kKnnSlotsWide = 8, kKnnMaxWide = kKnnSlotsWide * 8;   // 32 < k <= 64: the GICP family's covariances
constexpr const char* kKnnTooWide = "reg_correspondence_randomness > 64 is not supported by the HIP k-NN";
static_assert(kKnnMaxWide == 64, "kKnnTooWide names the limit");
// prefilter.hip
void prefilter_release(dgs_handle* h);
// map_cloud.hip
void map_cloud_release(dgs_handle* h);
// line_extraction.hip
void line_extraction_release(dgs_handle* h);
void line_align_release(dgs_handle* h);
// line_align_local.hip
void line_align_local_release(dgs_handle* h);
// line_edges.hip: edge_extraction of n_seg segments of the packed lines at d_lines (device, 6 doubles per line) -> h->le.edges and
// h->le.eoff_host (n_seg + 1).  `emit` false stops after the counts.  The caller has checked the limits (line_edges_bad_segments).
int line_edges_run(dgs_handle* h, const double* d_lines, const std::vector<LeSeg>& segs, bool emit);
void line_edges_release(dgs_handle* h);
// dgs_api.hip: the message dgs_last_error(NULL) returns, for an entry point that refuses its arguments before it looks at the handle
void set_handleless_error(const char* why);
// building_overlap.hip
void building_overlap_release(dgs_handle* h);
// floor_detection.hip
void floor_detection_release(dgs_handle* h);
const char* fd_bad_params(const dgs_floor_detection_params* p);   // why the parameters are refused, or nullptr
// floor_detection_batch.hip
void floor_detection_batch_release(dgs_handle* h);
// What a batched stage that runs inside another call did: the stage adds to the sink its caller hands it, the caller folds the sink
// into the counts8 of its own call.
struct StageCounts {
  int64_t launches = 0, waits = 0, built = 0;   // kernel launches, host waits, indices built
};
// floor_detection.hip, for the single call and the batch alike
namespace fdplan { struct ScanWalk; }
// a closed walk's end state -> tr; -> false: it ran past its draw list.  Else its winner, if it has one (hyps: the host's copy of the
// scan's hypotheses), -> tr and `coeffs`.
bool fd_walk_to_trace(const fdplan::ScanWalk& w, const FdHyp* hyps, dgs_floor_detection_trace& tr, float* coeffs);
// steps 5-8 of detect() over `pts` (n >= 3 points on the device) in the buffers handed in (the single call's FdScratch, or the batch's
// for a scan it finishes alone), with the draw list of `plan` and, while the walk runs past it, a longer one: the walk's end state in
// sc.trace, the winner's coefficients in `coeffs`, the cloud in sc.host_filtered.  *exhausted: the stream (rng_raw, or nullptr:
// mt19937(12345)) holds no further draw.  Launches and host waits are added to `did`.
int fd_ransac_lists(dgs_handle* h, const dgs_floor_detection_params& p, const float4* pts, int64_t n, const uint32_t* rng_raw, SacDrawPlan& plan,
                    SacScratch& sac, DevBuf<FdHyp>& hyps, FdScan& sc, float* coeffs, bool* exhausted, StageCounts* did);
// selectWithinDistance of the plane `c` over sc.host_filtered, in index order -> sc.inliers
void fd_select_inliers(FdScan& sc, const dgs_floor_detection_params& p, const float* c);
// step 9, the checks behind the RANSAC (fdplan::verdict): `coeffs` the winner's when sc.trace names one, `inliers` its inlier count
// -> sc.status, sc.coeffs, sc.trace.raw_coeffs and sc.trace.dot
void fd_verdict(FdScan& sc, const dgs_floor_detection_params& p, const float* tilt_inv16, const float* coeffs, int64_t inliers);
// the getters of both calls over a scan's record (nullptr: no such scan) and the device arrays of that scan
int fd_get_filtered(dgs_handle* h, const FdScan* sc, const float4* d_filtered, float* out_xyz16, int64_t capacity, int32_t out_on_device, int64_t* n);
int fd_get_inliers(const FdScan* sc, int32_t* indices, float* points_xyz16, int64_t capacity, int64_t* n);
int fd_get_trace(const FdScan* sc, dgs_floor_detection_trace* trace);
int fd_get_clipped(dgs_handle* h, const FdScan* sc, const float4* d_clipped, const float4* d_normals, float* clipped_xyz16, float* normals4, int64_t capacity,
                   int64_t* n);
// fitness_batch.hip
// the batched index build as a call of its own: FbScratch::counts8 reports it (and nothing else); `did` (nullable) receives the same
int fitness_batch_build_indices(dgs_handle* h, int n, dgs_cloud* const* clouds, StageCounts* did = nullptr);
int fitness_batch_build_state_indices(dgs_handle* h, int n, CloudState* const* clouds, StageCounts* sink);   // the build over cloud states, inside another call
int fitness_batch_clouds(dgs_handle* h, int n_edges, dgs_cloud* const* cloud1s, dgs_cloud* const* cloud2s, const float* relposes16, double max_range,
                         double* scores, int64_t* used);
// one edge of the scorer over plain device arrays: index over cloud1, cloud2's points, the relative pose (column-major, host)
struct FbEdgeIn {
  const Bvh* index;
  const float4* src;
  int64_t n1, n2;
  const float* T16;
};
int fitness_batch_edges(dgs_handle* h, int n_edges, const FbEdgeIn* in, double max_range, double* scores, int64_t* used);
// the same scorer for sources of the handle's current target (batch-independent fitness): builds the target's index when it has none
// dgs_calc_inlier_fraction_batch_clouds: per edge the points of relpose * cloud2 whose exact 1-NN squared distance in cloud1 is < max_sq_dist
int inlier_batch_clouds(dgs_handle* h, int n_edges, dgs_cloud* const* cloud1s, dgs_cloud* const* cloud2s, const float* relposes16, double max_sq_dist,
                        double* fractions, int64_t* inliers);
int fitness_target_edges(dgs_handle* h, int n, const float4* const* srcs, const int64_t* sizes, const float* T16s, size_t T_stride_floats, double max_range, double* scores);
void fitness_batch_release(dgs_handle* h);
// building_cloud.hip
void building_cloud_release(dgs_handle* h);
// voxel_batch.hip: inputs filtered (0 NONE, 1 VOXELGRID, 2 APPROX_VOXELGRID) into resident clouds; the caller has checked the arguments
int cloud_assign_batch(dgs_handle* h, int n, const float* const* inputs, const int64_t* sizes, int on_device, int filter, float leaf, dgs_cloud* const* clouds,
                       int64_t* out_sizes);
// VOXELGRID of n device inputs into n cloud states by one chain, two host waits (added to `sink`); `owners` (nullable):
// the dgs_cloud objects the states belong to, whose users are detached.  On DGS_ERR_GRID_TOO_LARGE no state has been touched.
int voxelgrid_batch(dgs_handle* h, int n, const float4* const* d_in, const int64_t* sizes, float leaf, CloudState* const* states, dgs_cloud* const* owners,
                    int64_t* out_sizes, StageCounts* sink);
void voxel_batch_release(dgs_handle* h);
// prefilter_batch.hip
void prefilter_batch_release(dgs_handle* h);
void prefilter_batch_release(PfbScratch& S);
// The normal stage of the batched chain for another call (floor_detection_batch.hip), in the scratch S it hands in: the batched index
// build over pool[s] for every scan s < n with sizes[s] > 0, the k = min(10, size) lists and pf_normal_body with one view point,
// normals of scan s -> normals[s].  Launches only: nobody waits.  Launches, waits and builds are added to S.counts8; *fell_back: the
// lists came from the per-query walk scan by scan (DGS_KNN_LEAF=0).
int prefilter_batch_normal_stage(dgs_handle* h, PfbScratch& S, int n, CloudState* pool, const int64_t* sizes, float vx, float vy, float vz,
                                 float4* const* normals, bool* fell_back);
// dgs_api.hip: the handles that borrow `c` as target or source fall back to "no input set" (what dgs_cloud_destroy does first)
void cloud_detach_users(dgs_cloud* c);
// pcl_gicp.hip
int ensure_pcov(dgs_handle* h, CloudState& c);   // the PCL-style covariances of a cloud, cached under (k, epsilon)
int pcl_gicp_align(dgs_handle* h, const float* guess16, dgs_result* out);
int pcl_gicp_align_batch(dgs_handle* h, int n, CloudState* const* srcs, const float* guesses16, dgs_result* out);
int pcl_gicp_align_pairs(dgs_handle* h, int n, dgs_cloud* const* tgts, dgs_cloud* const* srcs, const float* guesses16, dgs_result* out);   // pair i against tgts[i]
const float* pcl_gicp_final_transforms(dgs_handle* h, size_t* stride_bytes);
int pcl_gicp_covariances(dgs_handle* h, int which, double* host_out9, int64_t n);
int pcl_gicp_evaluate(dgs_handle* h, const double* x6, int32_t* m, double* f, double* g6);
int pcl_gicp_trajectory(dgs_handle* h, int pair, float* T16s, int32_t* n_corr, int32_t* inner, int32_t* passes, double* f, int capacity, int* len);
void pcl_gicp_release(dgs_handle* h);
// transform
int transform_cloud(dgs_handle* h, const float4* in, float4* out, int64_t n, const float* T16_colmajor_host);
// dgs_api.hip: a copy of `src` (points only) on dst_h's device, device to device (peer copy over xGMI when the devices differ)
int cloud_clone_to(dgs_handle* dst_h, const dgs_cloud* src, dgs_cloud** out);

}  // namespace dgs
