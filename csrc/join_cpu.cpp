// mxstream — C++ twins of the window-join kernels (csrc/join_hip.hip; design: csrc/mxs_join.h).
// Plain loops: they define the result the kernels are compared against array for array.
#include <stdexcept>

#include "mxs_join.h"

namespace mxs {
namespace cpu {

namespace {
int64_t seg_len(const JoinSide& s, int64_t i) {
  return (i + 1 < s.nseg ? s.heads[i + 1] : s.total) - s.heads[i];
}
}  // namespace

void join_match(const JoinSide& l, const JoinSide& r, int64_t* match, uint64_t* cnt) {
  for (int64_t i = 0; i < l.nseg; ++i) {
    const int64_t key = l.keys[i];
    int64_t lo = 0, hi = r.nseg;  // first right segment whose key is >= key
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (r.keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    if (lo < r.nseg && r.keys[lo] == key) {
      match[i] = lo;
      cnt[i] = join_sat_mul((uint64_t)seg_len(l, i), (uint64_t)seg_len(r, lo));
    } else {
      match[i] = -1;
      cnt[i] = 0;
    }
  }
}

void join_scan(const JoinSide& l, const JoinSide& r, const int64_t* match, const uint64_t* cnt,
               int64_t* pair_off, int64_t* plan, int64_t* meta) {
  const int64_t stride = l.nseg + 1;
  uint64_t run = 0;
  int64_t m = 0;
  for (int64_t i = 0; i < l.nseg; ++i) {
    pair_off[i] = (int64_t)run;
    if (cnt[i]) {
      const int64_t j = match[i];
      plan[kJoinFirst * stride + m] = (int64_t)run;
      plan[kJoinKey * stride + m] = l.keys[i];
      plan[kJoinLs * stride + m] = l.heads[i];
      plan[kJoinRs * stride + m] = r.heads[j];
      plan[kJoinNr * stride + m] = seg_len(r, j);
      ++m;
    }
    run = join_sat_add(run, cnt[i]);
  }
  pair_off[l.nseg] = (int64_t)run;
  plan[kJoinFirst * stride + m] = (int64_t)run;
  meta[kJoinP] = (int64_t)run;
  meta[kJoinM] = m;
  meta[kJoinErr] = run >= (uint64_t)kJoinMaxPairs ? 1 : 0;
}

void join_expand(const JoinSide& l, const JoinSide& r, const int64_t* match,
                 const int64_t* pair_off, const uint64_t* lord, const uint64_t* rord, int64_t p0,
                 int64_t p1, int64_t* out_key, int64_t* out_l, int64_t* out_r) {
  if (p0 < 0 || p1 < p0 || p1 > pair_off[l.nseg])
    throw std::invalid_argument("join_expand: pair range outside [0, P)");
  if (p0 == p1) return;
  // The segment that owns p0: the last one whose offset is <= p0 (an unmatched segment shares
  // its offset with its successor and is never the last).
  int64_t lo = 0, hi = l.nseg;  // pair_off[lo] <= p0 < pair_off[hi]
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (pair_off[mid] <= p0) lo = mid; else hi = mid;
  }
  int64_t p = p0;
  for (int64_t i = lo; i < l.nseg && p < p1; ++i) {
    const int64_t j = match[i];
    if (j < 0) continue;
    const int64_t nl = seg_len(l, i), nr = seg_len(r, j);
    const int64_t q = p - pair_off[i];  // > 0 only in the first segment
    int64_t a = q / nr, b = q % nr;
    for (; a < nl && p < p1; ++a, b = 0) {
      const int64_t lv = (int64_t)f64_from_order_bits(lord[l.heads[i] + a]);
      for (; b < nr && p < p1; ++b, ++p) {
        out_key[p - p0] = l.keys[i];
        out_l[p - p0] = lv;
        out_r[p - p0] = (int64_t)f64_from_order_bits(rord[r.heads[j] + b]);
      }
    }
  }
}

}  // namespace cpu
}  // namespace mxs
