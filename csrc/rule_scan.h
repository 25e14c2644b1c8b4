// mxstream — what the keyed rules' device code shares: the host helpers of csrc/mxs_hip_util.h
// for their six units (csrc/timeout_hip.hip, sustain_hip.hip, burst_hip.hip, reorder_hip.hip,
// fsm_hip.hip, rate_hip.hip), and for the rules that scan a batch sorted by key
// (sustain_scan_kernel, burst_scan_kernel, fsm_scan_kernel, rate_scan_kernel) the scan frame: who
// owns a key's run, the append of a transition, and when a wave walks on. The counter rates
// (rate_scan_kernel) use the frame without the append: about one row leaves per element, placed
// by arrival index and compacted in order (csrc/mxs_rate.h).
// Included from .hip files only.
//
// The frame. The batch arrives stably sorted by key (`skeys`, with `perm` = the arrival index of
// every sorted row). A wave owns the key runs that BEGIN in its 64 sorted rows, its chunk: their
// elements there are one segmented inclusive scan (a run head starts a segment, every lane loads
// its key's row as the carry), so short runs share a wave. A run that leaves the chunk is walked
// on by the same wave, 64 rows at a time, with the carry in registers; the rows before a chunk's
// first head belong to such a walk and are skipped by the chunk's own wave. A key's state
// therefore has one reading and one writing wave: the lane that ends a run stores it, no atomics
// touch it. Transitions are appended with one reservation per wave and chunk that has any
// (ballot / popcount), each tagged ``arrival index << 1 | code``; sustain_gather_kernel
// (csrc/sustain_hip.hip), the family's gather, turns the rows sorted by tag into the five
// output columns. The state machines' rows carry 8 bits of code: rule_row_append and a gather of
// their own (csrc/fsm_hip.hip).
//
// A kernel's loops around the frame:
//   for (base = the wave's first row; base < n; base += the grid's rows)   // the wave's chunks
//     for (b0 = base;; b0 += 64)                                           // a chunk, then a walk
//       fr = rule_heads(skeys, n, b0, lane, cont);
//       if (fr.leave) break;
//       rule_owned(skeys, perm, n, cap, lane, cont, ck, fr);
//       ..
// The frame is two calls with the leave between them, in the kernel: as one function the early
// exit merges with the full path at the function's end, which cost the walk onto a hot key's run
// 2.8 % (profiles/rule_scan_refactor.md).
//       if (!rule_run_goes_on(fr.act, tm)) break;
//       cont = true, ck = __shfl(fr.k, 63), the carry = lane 63's state;
// `base` and `b0` are the same for a wave's 64 lanes, `leave` and rule_run_goes_on's result
// come from ballots, and `cont` and `ck` are set from them and from shuffles of one lane: every
// loop condition is wave-uniform, the 64 lanes leave together and every ballot and shuffle below
// runs with all of them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mxs_hip_util.h"

namespace mxs {

// A lane's place in the frame: sorted row i = b0 + lane, its key and arrival index.
struct RuleFrame {
  int64_t i, k, src;
  bool in;    // i < n
  bool head;  // the row begins a run (never while walking on)
  bool act;   // the row belongs to a run this wave owns
  bool tail;  // act, and the row ends its run
  bool ok;    // act, and key and arrival index are in range: the lane may touch memory
  unsigned long long hm;  // the head ballot (0 while walking on)
  bool leave;  // wave-uniform: no run begins in this chunk
};

// The frame's first piece, for the 64 rows from b0 on: i, in, k, and unless the wave is walking
// on (`cont`) the run heads and their ballot. `leave` (the same in every lane): the whole chunk
// continues an earlier run, that run's wave walks it and this one goes to its next chunk.
__device__ __forceinline__ RuleFrame rule_heads(const int64_t* skeys, int64_t n, int64_t b0,
                                                int lane, bool cont) {
  RuleFrame fr = {};
  fr.i = b0 + lane;
  fr.in = fr.i < n;
  fr.k = fr.in ? skeys[fr.i] : 0;
  if (!cont) {
    // the neighbour reads stay inside the batch: row i - 1 is read for i >= 1 only
    fr.head = fr.in && (fr.i == 0 || skeys[fr.i - 1] != fr.k);
    fr.hm = __ballot(fr.head);
  }
  fr.leave = !cont && !fr.hm;
  return fr;
}

// The second piece, in a wave that stays: act, tail, src and ok. `ck` is the key of the run the
// wave is walking on.
__device__ __forceinline__ void rule_owned(const int64_t* skeys, const int64_t* perm, int64_t n,
                                           int64_t cap, int lane, bool cont, int64_t ck,
                                           RuleFrame& fr) {
  if (!cont) fr.act = fr.in && lane >= __ffsll((long long)fr.hm) - 1;
  else fr.act = fr.in && fr.k == ck;  // sorted: a prefix of the chunk, lane 0 included
  // and row i + 1 for i + 1 < n only
  fr.tail = fr.act && (fr.i + 1 == n || skeys[fr.i + 1] != fr.k);
  fr.src = fr.act ? perm[fr.i] : 0;
  // Out-of-range ids never reach memory (the callers check both before the launch).
  fr.ok = fr.act && (uint64_t)fr.k < (uint64_t)cap && (uint64_t)fr.src < (uint64_t)n;
}

// The value before a lane's element: the previous lane's `after`, or the carry at a run's head
// and in lane 0 (a walked run's carry is lane 63's `after` of the chunk before).
template <typename T>
__device__ __forceinline__ T rule_before(T after, T carry, bool head, int lane) {
  const T prev = __shfl_up(after, 1);
  return (head || lane == 0) ? carry : prev;
}

// Append the wave's transitions: one reservation for all of them, then per emitting lane the tag
// ``arrival << 1 | code`` (code 1: fired) and `since`, a fired row's from the state after the
// element (s1), a resolved row's from the state before it (s0). `fire` and `resolve` are the
// rule's own; both false in a lane that is not `ok`. All 64 lanes call it.
__device__ __forceinline__ void rule_edge_append(bool fire, bool resolve, int64_t src, int64_t s1,
                                                 int64_t s0, int64_t n,
                                                 int64_t* __restrict__ out_tag,
                                                 int64_t* __restrict__ out_since,
                                                 uint32_t* __restrict__ out_n, int lane) {
  const bool emit = fire || resolve;
  const unsigned long long m = __ballot(emit);
  uint32_t wb = 0;
  if (lane == 0 && m) wb = atomicAdd(out_n, (uint32_t)__popcll(m));
  wb = __shfl(wb, 0);
  if (emit) {
    const int64_t q = (int64_t)wb + __popcll(m & ((1ull << lane) - 1ull));
    if (q < n) {  // at most one row per element: always true
      out_tag[q] = (src << 1) | (fire ? 1 : 0);
      out_since[q] = fire ? s1 : s0;
    }
  }
}

// The same append for a rule whose rows carry a wider code (fsm_scan_kernel: 8 bits): the lane's
// own `tag` = ``arrival << bits | code`` and `since`. `emit` is false in a lane that is not `ok`.
// All 64 lanes call it.
__device__ __forceinline__ void rule_row_append(bool emit, int64_t tag, int64_t since, int64_t n,
                                                int64_t* __restrict__ out_tag,
                                                int64_t* __restrict__ out_since,
                                                uint32_t* __restrict__ out_n, int lane) {
  const unsigned long long m = __ballot(emit);
  uint32_t wb = 0;
  if (lane == 0 && m) wb = atomicAdd(out_n, (uint32_t)__popcll(m));
  wb = __shfl(wb, 0);
  if (emit) {
    const int64_t q = (int64_t)wb + __popcll(m & ((1ull << lane) - 1ull));
    if (q < n) {  // at most one row per element: always true
      out_tag[q] = tag;
      out_since[q] = since;
    }
  }
}

// The run of lane 63 goes on in the next chunk: the wave walks it. `tm` is the tail ballot.
__device__ __forceinline__ bool rule_run_goes_on(bool act, unsigned long long tm) {
  const unsigned long long am = __ballot(act);
  return ((am >> 63) & 1ull) && !((tm >> 63) & 1ull);
}

}  // namespace mxs
