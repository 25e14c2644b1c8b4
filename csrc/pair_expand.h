// mxstream — the tile frame of an output-centric pair expansion, shared by join_expand_kernel
// (csrc/join_hip.hip) and ijoin_expand_kernel (csrc/ijoin_hip.hip). Device code only: include
// from a .hip file.
//
// A plan lists the m rows that have pairs; its first-pair column `first` (m + 1 words, strictly
// increasing, first[m] = P) says where each row's pairs start among all P. A workgroup of
// kJoinBlock threads owns kJoinTile consecutive output positions: pair_tile_begin finds the rows
// that overlap them and leaves their tile-relative starts in LDS, and in every store round a
// lane that has left its row finds its next one there with pair_lane_row. A kernel's loops
// around the frame:
//   for (tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
//     t = pair_tile_begin(first, m, p0, p1, tile, rel);
//     for (r = 0; r < kPairRounds; ++r)
//       pr = r * kPairStep + 2 * threadIdx.x;          // the lane's two positions: pr, pr + 1
//       if (pr >= t.len) break;
//       if (pr >= nxt) k = pair_lane_row(rel, k, t.ns, pr), nxt = rel[k + 1], the row's data
//       else           the same row, kPairStep positions on
//       ..
//     __syncthreads();                                 // rel is refilled for the next tile
// The break and the branch stay in the kernels; the helpers have no early return (a helper whose
// exit merges with its full path at its end has cost a hot loop 2.8 %:
// profiles/rule_scan_refactor.md).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mxs_join.h"

namespace mxs {

constexpr int kPairStep = 2 * kJoinBlock;  // positions a workgroup covers per store round
constexpr int kPairRounds = kJoinTile / kPairStep;

struct PairTile {
  int64_t tb;     // the tile's first position among all pairs
  int32_t len;    // its positions (kJoinTile, less in the range's last tile)
  int64_t s0;     // the plan row that owns the tile's first position
  int32_t ns;     // plan rows that overlap the tile, 1 <= ns <= len: offsets strictly increase
  int64_t qbase;  // pairs of row s0 before the tile
};

// The frame of tile `tile` of the range [p0, p1). Fills rel[0 .. ns]: rel[k] = the tile-relative
// first position of the tile's k-th row (rel[0] = 0: the row that owns the tile's first position
// started at or before it), rel[ns] = the tile's length. All threads call it; it ends with the
// barrier after the fill.
__device__ __forceinline__ PairTile pair_tile_begin(const int64_t* __restrict__ first, int64_t m,
                                                    int64_t p0, int64_t p1, int64_t tile,
                                                    int32_t* rel) {
  PairTile t;
  t.tb = p0 + tile * kJoinTile;
  t.len = (int32_t)(p1 - t.tb < kJoinTile ? p1 - t.tb : kJoinTile);
  const int64_t tb = t.tb, te = tb + t.len;
  // s0 = the last row with first <= tb; the tile's rows end before the first row after s0 with
  // first >= te (first[m] = P >= te). Both searches are uniform over the workgroup.
  int64_t lo = 0, hi = m;    // first[lo] <= tb < first[hi]
  int64_t lo2 = 0, hi2 = m;  // first[lo2] < te <= first[hi2]
  while (hi - lo > 1 || hi2 - lo2 > 1) {
    if (hi - lo > 1) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (first[mid] <= tb) lo = mid; else hi = mid;
    }
    if (hi2 - lo2 > 1) {
      const int64_t mid = lo2 + ((hi2 - lo2) >> 1);
      if (first[mid] < te) lo2 = mid; else hi2 = mid;
    }
  }
  t.s0 = lo;
  t.ns = (int32_t)(hi2 - lo);
  t.qbase = tb - first[lo];
  for (int32_t k = threadIdx.x; k <= t.ns; k += kJoinBlock)
    rel[k] = k == 0 ? 0 : (k == t.ns ? t.len : (int32_t)(first[lo + k] - tb));
  __syncthreads();
  return t;
}

// Another row for a lane at position pr that was in row k (-1: none yet): the last k' > k with
// rel[k'] <= pr (rel[k + 1] <= pr < rel[ns]).
__device__ __forceinline__ int32_t pair_lane_row(const int32_t* rel, int32_t k, int32_t ns,
                                                 int32_t pr) {
  int32_t l2 = k + 1, h2 = ns;
  while (h2 - l2 > 1) {
    const int32_t mid = (l2 + h2) >> 1;
    if (rel[mid] <= pr) l2 = mid; else h2 = mid;
  }
  return l2;
}

}  // namespace mxs
