// The launch clock: a kernel's duration from stamps its own workgroups write, instead of two HIP events around the launch (a marker packet
// on either side of a kernel keeps dependent kernels 3-6 us further apart than a plain boundary: DESIGN.md 6).
//
// A timed kernel takes a pointer to one LcSlot per workgroup (null = not timed: one uniform branch).  One lane of every workgroup stores the
// constant-rate wall clock at entry (t0) and behind the workgroup's last store (t1): plain vector stores, one slot per workgroup, no atomics, no
// reset.  The host reads the slots behind a completed stream or copy and reduces a launch to (max t1 - min t0) / rate: first workgroup in to
// last workgroup out, without the dispatch on either side.
//
// The slots live in a ring of equal blocks in one device buffer; a launch takes the next block, the reader drains what is pending.  The
// bookkeeping and the reduction below make no HIP call and need no context (tests reach them through mind_debug_launch_clock); the buffer, the
// copies and the sums are predict.hip's.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

struct LcSlot { unsigned long long t0, t1; };      // wall-clock ticks at the workgroup's entry / behind its last store

enum { LC_PAIR = 0, LC_ACTOR = 1, LC_ILQR = 2, LC_KINDS = 3 };

// a timed launch: its block of the ring, its workgroups (= slots written), what it was, and whether a copy of the block to the host was queued
struct LcRecord { int block, grid, kind, copied; };

struct LcRing {
  int n_blocks = 0, block_slots = 0;               // geometry of the device buffer: n_blocks blocks of block_slots slots
  int head = 0;                                    // the next block handed out
  long long dropped = 0;                           // launches that got no block (take() < 0) since reset()
  std::vector<LcRecord> pending;                   // handed out and not drained, oldest first: blocks head - pending.size() .. head - 1 (mod n_blocks)

  void reset(int blocks, int slots) { n_blocks = blocks; block_slots = slots; head = 0; dropped = 0; pending.clear(); }
  // `records` more launches of at most `grid` workgroups fit beside what is pending
  bool fits(int records, int grid) const { return grid <= block_slots && (long long)pending.size() + records <= n_blocks; }
  // the geometry to grow to so that they do (never smaller than the present one): blocks double, slots round up to a multiple of 64
  void grown(int records, int grid, int &blocks, int &slots) const {
    blocks = n_blocks > 0 ? n_blocks : 32;
    slots = block_slots > 0 ? block_slots : 64;
    while (blocks < records) blocks *= 2;          // (the caller drains before it re-allocates: only the new records must fit)
    if (grid > slots) slots = (grid + 63) / 64 * 64;
  }
  // the next block for a launch of `grid` workgroups; -1 when the grid outgrows a block or every block is pending (the launch then runs
  // untimed and is counted in `dropped`: a pending block is never overwritten)
  int take(int grid, int kind) {
    if (grid <= 0 || grid > block_slots || (int)pending.size() >= n_blocks) { ++dropped; return -1; }
    const int b = head;
    head = head + 1 == n_blocks ? 0 : head + 1;
    pending.push_back(LcRecord{b, grid, kind, 0});
    return b;
  }
  size_t slot_of(int block) const { return (size_t)block * (size_t)block_slots; }
  // the blocks of the pending records i0 .. i0 + n - 1 as at most two runs [first, first + count) of consecutive blocks (two when they wrap);
  // returns the number of runs
  int pending_runs(int i0, int n, int (&first)[2], int (&count)[2]) const {
    if (n <= 0 || i0 < 0 || i0 + n > (int)pending.size()) return 0;
    const int b0 = pending[i0].block;
    if (b0 + n <= n_blocks) { first[0] = b0; count[0] = n; return 1; }
    first[0] = b0; count[0] = n_blocks - b0;
    first[1] = 0; count[1] = n - count[0];
    return 2;
  }
  // the oldest n records all have their copy queued
  bool copied(int n) const {
    if (n > (int)pending.size()) return false;
    for (int i = 0; i < n; ++i)
      if (!pending[i].copied) return false;
    return true;
  }
  void mark_copied(int i0, int n) {
    for (int i = i0; i < i0 + n && i < (int)pending.size(); ++i)
      if (i >= 0) pending[i].copied = 1;
  }
  // the oldest n records were read (head stays: the ring goes on where it was)
  void drained(int n) {
    if (n >= (int)pending.size()) pending.clear();
    else if (n > 0) pending.erase(pending.begin(), pending.begin() + n);
  }
};

// one launch from its slots: last stamp out minus first stamp in, in ticks (0 for an empty grid or stamps that run backwards)
static inline unsigned long long lc_reduce(const LcSlot *s, int grid) {
  if (grid <= 0) return 0;
  unsigned long long lo = s[0].t0, hi = s[0].t1;
  for (int i = 1; i < grid; ++i) {
    if (s[i].t0 < lo) lo = s[i].t0;
    if (s[i].t1 > hi) hi = s[i].t1;
  }
  return hi > lo ? hi - lo : 0;
}

// ticks of a clock of rate_khz (hipDeviceAttributeWallClockRate: kHz = ticks per millisecond) in milliseconds
static inline double lc_ticks_ms(unsigned long long ticks, int rate_khz) { return rate_khz > 0 ? (double)ticks / (double)rate_khz : 0.0; }

#if defined(__HIPCC__)
// The stamps, one text for every timed kernel.  lc_stamp_in: first statement of the kernel, in front of any early return.  lc_stamp_out: behind the
// workgroup's last store on a path every thread of the workgroup takes (the barrier and its wait for the waves' outstanding stores exist with a
// non-null pointer only).  lc_stamp_both: a workgroup that leaves at once.
__device__ __forceinline__ void lc_stamp_in(LcSlot *clk) {
  if (clk != nullptr && threadIdx.x == 0) clk[blockIdx.x].t0 = (unsigned long long)wall_clock64();
}
__device__ __forceinline__ void lc_stamp_out(LcSlot *clk) {
  if (clk != nullptr) {
    __syncthreads();
    if (threadIdx.x == 0) clk[blockIdx.x].t1 = (unsigned long long)wall_clock64();
  }
}
__device__ __forceinline__ void lc_stamp_both(LcSlot *clk) {
  if (clk != nullptr && threadIdx.x == 0) {
    const unsigned long long t = (unsigned long long)wall_clock64();
    clk[blockIdx.x].t0 = t;
    clk[blockIdx.x].t1 = t;
  }
}
#endif
