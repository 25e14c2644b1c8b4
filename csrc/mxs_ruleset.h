// mxstream — broadcast rule set (``samples.key_by(..).connect(rules.broadcast(..)).process(
// RuleSetAlert(..))``): up to 64 rules hold for every key, every sample is tested against all of
// them and leaves once per rule that it breaks. The lookup's compaction becomes an expansion.
//
// State: one table int64[kRuleSetMax, 2]; row r = (threshold bits, comparison code) of rule id r.
// The code is a LookupWhen (kLookupGt .. kLookupNe, csrc/mxs_lookup.h); 0 means no rule r.
//
// The frame is the lookup's: a tile is kLookupTile samples, 64 groups of 64. Kernels
// (csrc/ruleset_hip.hip) and their C++ twins (csrc/ruleset_cpu.cpp):
//   ruleset_count  per sample v: m = the 64-bit mask of the rules it breaks, bit r set iff rule r
//                  exists and ``v <code r> threshold r`` on the two doubles (Java's rules: NaN is
//                  false but for !=, -0.0 == 0.0). gsum[tile * 64 + j] = the rows (set bits) of the
//                  samples [64 j, 64 j + 64) of the tile, counts[tile] = the tile's rows (at most
//                  4096 * 64 = 2**18). Samples >= n count 0. Reads 8 bytes per sample, no keys.
//   lookup_scan    (as it is) offsets = the exclusive scan of counts, meta[0] = the total
//   ruleset_emit   one row per sample and set bit, in sample order, then ascending rule id, as
//                  five columns (key, value bits, rule id, threshold bits, ts): a sample's first
//                  row is offsets[tile] + the rows of the tile's earlier groups + the rows of the
//                  group's earlier samples. The mask is recomputed, not stored.
#pragma once
#include <cstdint>

#include "mxs_lookup.h"

namespace mxs {

constexpr int kRuleSetMax = 64;                  // rule ids [0, 64): one mask bit each
constexpr int kRuleSetGroups = kLookupTile / 64;  // group sums of a tile

// A table row's code is a rule when it is one of the six comparisons.
MXS_HD bool ruleset_active(int64_t code) { return code >= kLookupGt && code <= kLookupNe; }

namespace gpu {
void ruleset_count(const int64_t* vals, int64_t n, const int64_t* rules, uint32_t* gsum,
                   uint32_t* counts, intptr_t stream);
void ruleset_emit(const int64_t* keys, const int64_t* vals, const int64_t* ts, int64_t n,
                  const int64_t* rules, const uint32_t* gsum, const uint32_t* counts,
                  const int64_t* offsets, int64_t total, int64_t* out_key, int64_t* out_val,
                  int64_t* out_rule, int64_t* out_thr, int64_t* out_ts, intptr_t stream);
}  // namespace gpu

namespace cpu {
void ruleset_count(const int64_t* vals, int64_t n, const int64_t* rules, uint32_t* gsum,
                   uint32_t* counts);
void ruleset_emit(const int64_t* keys, const int64_t* vals, const int64_t* ts, int64_t n,
                  const int64_t* rules, int64_t total, int64_t* out_key, int64_t* out_val,
                  int64_t* out_rule, int64_t* out_thr, int64_t* out_ts);
}  // namespace cpu

}  // namespace mxs
