// mxstream — keyed window joins (JoinedStreams.apply over one fired window): the two sides'
// gathered firings are matched by key and every matched key's nL x nR pairs are expanded into
// three output columns (key, left value, right value).
//
// A side is a gathered firing of the list-window pane arena (csrc/mxs_listwin.h): `keys[nseg]`
// ascending key ids, `heads[nseg]` the segment starts in `ord[total]` (segment i ends at
// heads[i + 1], the last one at `total`), `ord` the values as f64 order bits.
//
// Kernels (csrc/join_hip.hip) and their C++ twins (csrc/join_cpu.cpp):
//   join_match   per left segment: the right segment of the same key (binary search, or -1) and
//                the pair count nL * nR (64-bit, saturated at kJoinMaxPairs)
//   join_scan    exclusive scan of the counts -> pair_off[kL + 1] (pair_off[kL] = P), and the
//                matched segments compacted in order: plan rows (first pair, key, left start,
//                right start, nR), so that the offsets the expand searches strictly increase
//   join_expand  output positions [p0, p1) of [0, P): position p of matched segment j is
//                q = p - first[j], a = q / nR, b = q % nR, row (key, left[ls + a], right[rs + b])
//                -- left-major, the nested loop's order -- written at p - p0
//
// The plan is one int64 array of kJoinPlanCols columns of `kL + 1` words each (column c starts
// at c * (kL + 1)); column kJoinFirst holds m + 1 words (first[m] = P), the others m.
// meta (int64[kJoinMeta]): [kJoinP] = P, saturated at kJoinMaxPairs; [kJoinM] = m matched
// segments; [kJoinErr] != 0 when P reached kJoinMaxPairs (nothing may be expanded then).
#pragma once
#include <cstdint>

#include "mxs_common.h"

namespace mxs {

constexpr int64_t kJoinMaxPairs = 1ll << 62;
constexpr int kJoinScanTile = 4096;    // left segments per scan tile
constexpr int kJoinBlock = 256;        // threads of an expand workgroup
constexpr int kJoinTile = 4096;        // output positions per expand tile
constexpr int kJoinPlanCols = 5;
constexpr int kJoinFirst = 0, kJoinKey = 1, kJoinLs = 2, kJoinRs = 3, kJoinNr = 4;
constexpr int kJoinMeta = 4, kJoinP = 0, kJoinM = 1, kJoinErr = 2;

struct JoinSide {
  const int64_t* keys;
  const int64_t* heads;
  int64_t nseg, total;
};

// a + b of two values <= kJoinMaxPairs, saturated there (associative: the scan's operator).
MXS_HD uint64_t join_sat_add(uint64_t a, uint64_t b) {
  const uint64_t s = a + b;
  return s > (uint64_t)kJoinMaxPairs ? (uint64_t)kJoinMaxPairs : s;
}
// nl * nr saturated at kJoinMaxPairs (nl, nr >= 0).
MXS_HD uint64_t join_sat_mul(uint64_t nl, uint64_t nr) {
  if (nl == 0 || nr == 0) return 0;
  if (nl > (uint64_t)kJoinMaxPairs / nr) return (uint64_t)kJoinMaxPairs;
  return nl * nr;
}

namespace gpu {
void join_match(const JoinSide& l, const JoinSide& r, int64_t* match, uint64_t* cnt,
                intptr_t stream);
int64_t join_scan_scratch_bytes(int64_t kl);
void join_scan(const JoinSide& l, const JoinSide& r, const int64_t* match, const uint64_t* cnt,
               void* scratch, int64_t* pair_off, int64_t* plan, int64_t* meta, intptr_t stream);
void join_expand(const int64_t* plan, int64_t kl, int64_t m, int64_t P, const uint64_t* lord,
                 const uint64_t* rord, int64_t p0, int64_t p1, int64_t* out_key, int64_t* out_l,
                 int64_t* out_r, intptr_t stream);
}  // namespace gpu

namespace cpu {
void join_match(const JoinSide& l, const JoinSide& r, int64_t* match, uint64_t* cnt);
void join_scan(const JoinSide& l, const JoinSide& r, const int64_t* match, const uint64_t* cnt,
               int64_t* pair_off, int64_t* plan, int64_t* meta);
// The nested loop itself, from the unscanned description (match + pair_off, not the plan).
void join_expand(const JoinSide& l, const JoinSide& r, const int64_t* match,
                 const int64_t* pair_off, const uint64_t* lord, const uint64_t* rord, int64_t p0,
                 int64_t p1, int64_t* out_key, int64_t* out_l, int64_t* out_r);
}  // namespace cpu

}  // namespace mxs
