// mxstream — keyed interval joins (Flink 1.8 KeyedStream.intervalJoin(other).between(lo, hi)): an
// arriving batch of one side is joined at once with the other side's buffered elements of the
// same key whose timestamps lie in the batch element's range, then merged into its own buffer.
//
// A buffer is three int64 columns (key id, ts, value bits) of n rows, ascending by (key, ts),
// equal (key, ts) in arrival order. A batch is laid out the same way (sorted by the caller).
//
// Kernels (csrc/ijoin_hip.hip) and their C++ twins (csrc/ijoin_cpu.cpp):
//   ijoin_probe   per batch element (k, t): lb = the first other row >= (k, max(t + rlo,
//                 cutoff + 1)), ub = the first other row > (k, t + rhi), cnt = ub - lb (0 when the
//                 range is empty). (rlo, rhi) = (lo, hi) for a left batch, (-hi, -lo) for a right
//                 one; rows with ts <= cutoff are expired and never matched. Sums saturate.
//   ijoin_scan    exclusive 64-bit saturating scan of the counts with the non-empty elements
//                 compacted in order: plan rows (first pair, element index, lb), first[m] = P
//   ijoin_expand  output positions [p0, p1) of [0, P): position p of plan row j is b = p -
//                 first[j], batch element i = idx[j], other row o = lb[j] + b; four columns (key,
//                 left value, right value, max of the two timestamps) written at p - p0
//   ijoin_merge   rank merge of a sorted batch into a sorted buffer (old rows first on ties)
//   ijoin_keep    cnt = 1 for a row with ts > cutoff, else 0: scanned by ijoin_scan, whose idx
//   ijoin_gather  column then lists the survivors in order (the purge)
//
// The plan is one int64 array of kIJoinPlanCols columns of n + 1 words each; column kIJoinFirst
// holds m + 1 words, the others m. meta (int64[kIJoinMeta]) = [P saturated at kJoinMaxPairs, m,
// error != 0 when P reached kJoinMaxPairs, unused].
#pragma once
#include <cstdint>

#include "mxs_common.h"
#include "mxs_join.h"

namespace mxs {

constexpr int kIJoinPlanCols = 3;
constexpr int kIJoinFirst = 0, kIJoinIdx = 1, kIJoinLb = 2;
constexpr int kIJoinMeta = 4;
constexpr int64_t kI64Min = INT64_MIN, kI64Max = INT64_MAX;

struct IJoinCols {  // a buffer or a batch
  const int64_t* key;
  const int64_t* ts;
  const int64_t* val;
  int64_t n;
};

// a + b saturated at the int64 limits.
MXS_HD int64_t ijoin_sat_add(int64_t a, int64_t b) {
  if (b > 0 && a > kI64Max - b) return kI64Max;
  if (b < 0 && a < kI64Min - b) return kI64Min;
  return a + b;
}

// (ka, ta) < (kb, tb) in the buffers' order.
MXS_HD bool ijoin_less(int64_t ka, int64_t ta, int64_t kb, int64_t tb) {
  return ka < kb || (ka == kb && ta < tb);
}

// The first row of (key, ts)[0, n) that is >= (k, t) / > (k, t).
MXS_HD int64_t ijoin_lower(const int64_t* key, const int64_t* ts, int64_t n, int64_t k,
                           int64_t t) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (ijoin_less(key[mid], ts[mid], k, t)) lo = mid + 1; else hi = mid;
  }
  return lo;
}
MXS_HD int64_t ijoin_upper(const int64_t* key, const int64_t* ts, int64_t n, int64_t k,
                           int64_t t) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (!ijoin_less(k, t, key[mid], ts[mid])) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One batch element's range [lb, lb + cnt) in the other buffer.
MXS_HD void ijoin_range(const int64_t* okey, const int64_t* ots, int64_t no, int64_t k, int64_t t,
                        int64_t rlo, int64_t rhi, int64_t cutoff, int64_t* lb, uint64_t* cnt) {
  int64_t tl = ijoin_sat_add(t, rlo);
  const int64_t th = ijoin_sat_add(t, rhi);
  const bool none = cutoff == kI64Max;  // every row is expired
  if (!none && tl < cutoff + 1) tl = cutoff + 1;
  const int64_t l = ijoin_lower(okey, ots, no, k, tl);
  *lb = l;
  if (none || tl > th) {
    *cnt = 0;
    return;
  }
  const int64_t u = ijoin_upper(okey, ots, no, k, th);
  *cnt = u > l ? (uint64_t)(u - l) : 0ull;
}

namespace gpu {
void ijoin_probe(const IJoinCols& batch, const IJoinCols& other, int64_t rlo, int64_t rhi,
                 int64_t cutoff, int64_t* lb, uint64_t* cnt, intptr_t stream);
int64_t ijoin_scan_scratch_bytes(int64_t n);
void ijoin_scan(const uint64_t* cnt, const int64_t* lb, int64_t n, void* scratch, int64_t* plan,
                int64_t* meta, intptr_t stream);
void ijoin_expand(const int64_t* plan, int64_t n, int64_t m, int64_t P, const IJoinCols& batch,
                  const IJoinCols& other, int side, int64_t p0, int64_t p1, int64_t* out_key,
                  int64_t* out_l, int64_t* out_r, int64_t* out_ts, intptr_t stream);
void ijoin_merge(const IJoinCols& old, const IJoinCols& batch, int64_t* out_key, int64_t* out_ts,
                 int64_t* out_val, intptr_t stream);
void ijoin_keep(const int64_t* ts, int64_t n, int64_t cutoff, uint64_t* cnt, intptr_t stream);
void ijoin_gather(const int64_t* plan, int64_t n, int64_t m, const IJoinCols& src,
                  int64_t* out_key, int64_t* out_ts, int64_t* out_val, intptr_t stream);
}  // namespace gpu

namespace cpu {
void ijoin_probe(const IJoinCols& batch, const IJoinCols& other, int64_t rlo, int64_t rhi,
                 int64_t cutoff, int64_t* lb, uint64_t* cnt);
void ijoin_scan(const uint64_t* cnt, const int64_t* lb, int64_t n, int64_t* plan, int64_t* meta);
// The per-element loop itself, from the unscanned counts (cnt, lb), not from the plan.
void ijoin_expand(const uint64_t* cnt, const int64_t* lb, const IJoinCols& batch,
                  const IJoinCols& other, int side, int64_t p0, int64_t p1, int64_t* out_key,
                  int64_t* out_l, int64_t* out_r, int64_t* out_ts);
void ijoin_merge(const IJoinCols& old, const IJoinCols& batch, int64_t* out_key, int64_t* out_ts,
                 int64_t* out_val);
// Order-preserving compaction of the rows with ts > cutoff; returns their number.
int64_t ijoin_purge(const IJoinCols& src, int64_t cutoff, int64_t* out_key, int64_t* out_ts,
                    int64_t* out_val);
}  // namespace cpu

}  // namespace mxs
