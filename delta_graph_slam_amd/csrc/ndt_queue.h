// The persistent queue kernel and its launcher: EXPERIMENTS build only (measured slower than one launch per evaluation, see the
// status note).  Included by ndt_align.hip inside namespace dgs when DGS_EXPERIMENTS is defined, in the host part: it needs
// ndt_point_loop / ndt_block_row (ndt_fast.h), ndt_close_evaluation (ndt_optimiser.h), the queue layout helpers that the init
// kernel shares (queue_word, queue_ctl, queue_slot, ndt_queue_slices) and the host driver's NdtLaunch and with_search.

// ================================================================================================ the queue kernel
// STATUS (round 3): correct -- bit for bit equal to the launch-per-evaluation path under the same slice schedule
// (tests/test_queue_gpu.py) -- and SLOWER: 3.9-4.9 ms per 32-candidate step against 1.5 ms (DESIGN.md has the phase breakdown).  Off by
// default and compiled into the experiments build only.
// ONE persistent launch per align instead of one launch per evaluation.  A launch per evaluation pays, at every kernel boundary, the
// whole serial tail of the slowest pair -- row hand-off, Newton step, More-Thuente state machine, trig of the next transform, the
// dependent loads of the next prologue: t = 10.6 us + 1.49 us x (pairs still iterating) per launch on the 32-candidate bench step,
// 38 launches, i.e. 0.4 ms of 1.44 ms spent with the chip waiting for 32 single waves (profiles/r03/tail_table_lockstep.json).  Here the pairs
// advance independently: a work item is (pair, round, slice); the workgroup that closes round r of a pair opens its round r + 1, and
// every other workgroup meanwhile works on the other pairs' slices -- the serial tail of one pair hides behind the derivative work of
// the rest.  Workgroups are workers that CLAIM items (no worker ever waits for a particular other worker, so the kernel cannot
// deadlock on workgroups that are not resident), pairs that finish stop offering items, the stragglers' rounds are cut into more
// slices and get the whole chip, and a worker leaves when no pair is iterating any more.
//   queue word of a pair (64 bits, own 64-byte line): [63:44] round | [43:32] slices of this round | [31:0] slices claimed.
//   claim = one agent-scope atomic add of 1; the returned word tells round, slice count and the claimed slice at once.
//   The slice count of a round is a fixed function of (batch shape, round number) -- never of timing -- so the partition of the
//   sums, and with it every result bit, is reproducible run to run (ndt_queue_slices; the launch-per-evaluation path can be run with
//   the same schedule for bit-for-bit comparison: DGS_NDT_QUEUE=0 DGS_NDT_SCHEDULE=1).
//   Coherence inside the launch is per access, as for the rows (common.h): the closing workgroup writes the pair's record through
//   (agent-scope stores), drains, and only then publishes the next round's queue word; workers read queue words, the record and the
//   rows with agent-scope loads.  A worker whose poll guard runs out raises `abort` and everybody leaves (the align reports an error)
//   instead of hanging the device.

constexpr unsigned long long kQueueClosed = 0xFFFFFull << 44;   // round = all ones, no slices: the pair has finished
constexpr unsigned long long kQueueAbort = 1ull << 32;
template <int SEARCH>
__global__ __launch_bounds__(kBlock, 4) void ndt_queue_kernel(const float4* const* __restrict__ src_ptrs, const int* __restrict__ src_sizes, NdtPair* pairs,
                                                              const VoxelGrid g, const double gd1, const float gd2, const int leaf_pow2,
                                                              double* partials, const int n_pairs, const int cap_blocks, const int slices_base,
                                                              const NdtConsts consts, int* queue, int* __restrict__ done_counter, char* ring,
                                                              const int ring_rounds) {
  __shared__ unsigned long long s_item;
  __shared__ int s_pair;
  __shared__ int s_last;
  const int lane = threadIdx.x & 63;
  unsigned polls = 0;
#ifdef DGS_QUEUE_STATS
  unsigned acc_polls = 0, acc_failed = 0, acc_claims = 0, acc_closings = 0;
  unsigned long long acc_look = 0, acc_item = 0, acc_rec = 0, acc_loop = 0, acc_row = 0, acc_ticket = 0, acc_close = 0;
#define QSTAMP(var) const unsigned long long var = wall_clock64();
#else
#define QSTAMP(var)
#endif
  for (;;) {
    // ---- claim an item (wave 0; every lane holds the same values, lane 0 does the atomics)
    if (threadIdx.x < kWave) {
      int pair = -1;
      unsigned long long item = 0;
#ifdef DGS_QUEUE_STATS
      const unsigned long long t_claim0 = wall_clock64();
      unsigned st_polls = 0, st_failed = 0;
#endif
      unsigned idle = 0;
      for (;;) {
#ifdef DGS_QUEUE_STATS
        st_polls++;
#endif
        int left = 0, abort = 0;
        for (int c0 = 0; c0 <= n_pairs && pair < 0; c0 += 64) {
          const int idx = c0 + lane;   // queue word index: 0 = control, 1 + p = pair p
          unsigned long long w = 0;
          if (idx <= n_pairs) w = __hip_atomic_load(queue_ctl(queue) + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (c0 == 0) {
            left = __builtin_amdgcn_readfirstlane((int)(unsigned)w);
            abort = __builtin_amdgcn_readfirstlane((int)(unsigned)(w >> 32)) & 1;
          }
          unsigned long long m = __ballot(idx >= 1 && idx <= n_pairs && (unsigned)w < (unsigned)((w >> 32) & 0xFFFull));   // pairs with unclaimed slices
          if (m == 0ull) continue;
          // ONE attempt per look, at a pair that depends on the worker (so that the workers spread over the pairs); a worker that loses
          // the race looks again instead of walking down a stale list (which is what turns a few late workers into a herd)
          const int rot = (int)((blockIdx.x * 11u + polls + idle) & 63u);
          m = (m >> rot) | (rot ? (m << (64 - rot)) : 0ull);
          const int cand = c0 + ((__ffsll((long long)m) - 1 + rot) & 63) - 1;
          unsigned lo = 0, hi = 0;
          if (lane == 0) {
            const unsigned long long old = __hip_atomic_fetch_add(queue_word(queue, cand), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            lo = (unsigned)old; hi = (unsigned)(old >> 32);
          }
          lo = __builtin_amdgcn_readfirstlane(lo); hi = __builtin_amdgcn_readfirstlane(hi);
          if (lo < (hi & 0xFFFu)) { pair = cand; item = ((unsigned long long)hi << 32) | lo; }
#ifdef DGS_QUEUE_STATS
          else st_failed++;
#endif
          c0 = n_pairs + 1;   // leave the scan: claimed, or look again
          idle = 0;
        }
        if (pair >= 0) break;
        if (left <= 0 || abort != 0) break;
        // a worker that can never be needed again leaves: at most cap_blocks slices per pair still iterating can ever be on offer
        if ((long long)blockIdx.x >= (long long)left * cap_blocks) break;
        if (++polls > (1u << 22)) {   // seconds of polling without finding work: something is wrong -- leave, all of us
          if (lane == 0) __hip_atomic_fetch_or(queue_ctl(queue), kQueueAbort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          break;
        }
        // back off: the longer nothing was on offer, the longer the nap (0.5 us ... 8 us); whoever just lost a race looks again at once
        idle = min(idle + 1u, 5u);
        for (unsigned k = 0; k < (1u << (idle - 1u)); k++) __builtin_amdgcn_s_sleep(16);
      }
      if (lane == 0) { s_pair = pair; s_item = item; }
#ifdef DGS_QUEUE_STATS
      acc_polls += st_polls; acc_failed += st_failed; acc_claims += pair >= 0 ? 1 : 0; acc_look += wall_clock64() - t_claim0;
#endif
    }
    __syncthreads();
    const int pair = s_pair;
    if (pair < 0) {
#ifdef DGS_QUEUE_STATS
      if (threadIdx.x == 0) {   // diagnostic build: this worker's counters (100 MHz ticks), flushed once
        int* stat = queue + 2 * (n_pairs + 2);
        atomicAdd(&stat[2], (int)acc_polls); atomicAdd(&stat[3], (int)acc_failed); atomicAdd(&stat[4], (int)acc_claims); atomicAdd(&stat[7], (int)acc_closings);
        atomicAdd(&stat[5], (int)acc_look); atomicAdd(&stat[6], (int)acc_item);
        atomicAdd(&stat[8], (int)acc_rec); atomicAdd(&stat[9], (int)acc_loop); atomicAdd(&stat[10], (int)acc_row); atomicAdd(&stat[11], (int)acc_ticket); atomicAdd(&stat[12], (int)acc_close);
      }
#endif
      return;
    }
    QSTAMP(t_item0)
    const unsigned long long item = s_item;
    const int slice = (int)(unsigned)item, n_slices = (int)((item >> 32) & 0xFFFull), round = (int)(item >> 44);
    // ---- the round's record slot: scalar loads (see kQueueSlotBytes)
    const NdtPair& rec = *queue_slot(ring, ring_rounds, pair, round);
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; k++) T[k] = rec.T[k];
    const int need_h_word = rec.need_hessian;
    const bool need_h = need_h_word != 0;
    const float4* __restrict__ src = src_ptrs[pair];
    const int n = src_sizes[pair];
    double acc[kAccum];
#pragma unroll
    for (int k = 0; k < kAccum; k++) acc[k] = 0.0;
#ifdef DGS_QUEUE_STATS
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
    QSTAMP(t_rec)
    ndt_point_loop<SEARCH>(T, NdtHdrGlobal{rec}, need_h, src, n, slice * kBlock + (int)threadIdx.x, n_slices * kBlock, g, gd1, gd2, leaf_pow2, acc);
    QSTAMP(t_loop)
    ndt_block_row<true>(acc, partials + ((size_t)pair * cap_blocks + slice) * kAccumPad);
    // ---- publish the row, take a ticket; the workgroup that takes the round's last ticket closes it and opens the pair's next round
    if (threadIdx.x < kAccumPad) handoff_drain_stores();
    __syncthreads();
    QSTAMP(t_row)
    if (threadIdx.x == 0) s_last = handoff_take_ticket(&pairs[pair].ticket, n_slices) ? 1 : 0;
    __syncthreads();
    QSTAMP(t_ticket)
    if (s_last) {
      // the next round's slot starts as a copy of this round's transform (an evaluation that only adds the Hessian at the accepted point
      // keeps it); the optimiser then writes what changes.  Both through to memory, in this order.
      // The closing wave is ONE wave on a SIMD that it shares with the derivative loops of other workers: at equal priority its serial
      // chain (row sums, Newton step, line-search state machine, trig) runs at a third of its speed (measured 33 us against 8 us at the end
      // of a lockstep launch, where the SIMD is idle) -- and the pair's next round cannot open before it is through.  Raise it.
      __builtin_amdgcn_s_setprio(3);
      NdtPair* next = queue_slot(ring, ring_rounds, pair, min(round + 1, ring_rounds - 1));
      if (threadIdx.x < 12) {
        __hip_atomic_store(&next->T[threadIdx.x], T[threadIdx.x < 12 ? threadIdx.x : 0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      bool done = ndt_close_evaluation<true>(pairs + pair, partials + (size_t)pair * cap_blocks * kAccumPad, n_slices, consts, done_counter, 0x7FFFFFF0, next, need_h_word);
      if (round + 2 >= ring_rounds) done = true;   // cannot happen: the optimiser ends a registration long before its slots run out
      if (threadIdx.x < kWave) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the closing wave's write-through stores of the record have landed
        if (threadIdx.x == 0) {
          if (done) {
            __hip_atomic_store(queue_word(queue, pair), kQueueClosed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(queue_ctl(queue), ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // one pair fewer (the count is > 0: no borrow into the abort bit)
          } else {
            const unsigned long long next = ((unsigned long long)(round + 1) << 44) | ((unsigned long long)ndt_queue_slices(round + 1, slices_base, cap_blocks) << 32);
            __hip_atomic_store(queue_word(queue, pair), next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
      }
      __builtin_amdgcn_s_setprio(0);
    }
#ifdef DGS_QUEUE_STATS
    {
      const unsigned long long t_end = wall_clock64();
      acc_item += t_end - t_item0; acc_rec += t_rec - t_item0; acc_loop += t_loop - t_rec; acc_row += t_row - t_loop; acc_ticket += t_ticket - t_row;
      if (s_last) { acc_close += t_end - t_ticket; acc_closings++; }
    }
#endif
    __syncthreads();   // LDS (item, record, reduction buffers) is re-used by the next item
  }
}

static void launch_queue(dgs_handle* h, const NdtLaunch& L) {
  const dim3 grid(L.queue_workers), block(kBlock);
  const double gd1 = h->consts.gauss_d1;
  const float gd2 = (float)h->consts.gauss_d2;
  int fe = 0;
  const int leaf_pow2 = (std::frexp(h->grid.leaf, &fe) == 0.5f) ? 1 : 0;
  int slot = prof_begin(h, DGS_K_NDT_DERIVATIVES);
  with_search(h->consts.search_method, [&](auto S) {
    hipLaunchKernelGGL((ndt_queue_kernel<decltype(S)::value>), grid, block, 0, h->stream, h->src_ptrs.ptr, h->src_sizes.ptr, h->pairs.ptr, h->grid, gd1, gd2, leaf_pow2,
                       h->partials.ptr, L.n_pairs, L.cap_blocks, L.queue_base, h->consts, h->ndt_queue.ptr, h->done_counter.ptr,
                       reinterpret_cast<char*>(h->ndt_ring.ptr), h->ndt_ring_rounds);
  });
  prof_end(h, DGS_K_NDT_DERIVATIVES, slot);
}
