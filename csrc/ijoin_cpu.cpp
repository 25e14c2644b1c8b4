// mxstream — C++ twins of the interval-join kernels (csrc/ijoin_hip.hip; design:
// csrc/mxs_ijoin.h). Plain loops: they define the result the kernels are compared against array
// for array.
#include <stdexcept>

#include "mxs_ijoin.h"

namespace mxs {
namespace cpu {

void ijoin_probe(const IJoinCols& batch, const IJoinCols& other, int64_t rlo, int64_t rhi,
                 int64_t cutoff, int64_t* lb, uint64_t* cnt) {
  // Linear scans, not the kernels' binary searches: the first row >= (k, tl), then the rows up
  // to (k, th). A sorted batch's bounds never decrease, so both scans go on where the previous
  // element's ended; a bound that does decrease restarts them.
  const bool none = cutoff == kI64Max;
  int64_t l = 0, u = 0, pk = kI64Min, ptl = kI64Min, pth = kI64Min;
  for (int64_t i = 0; i < batch.n; ++i) {
    const int64_t k = batch.key[i], t = batch.ts[i];
    int64_t tl = ijoin_sat_add(t, rlo);
    const int64_t th = ijoin_sat_add(t, rhi);
    if (!none && tl < cutoff + 1) tl = cutoff + 1;
    if (ijoin_less(k, tl, pk, ptl)) l = 0;
    if (ijoin_less(k, th, pk, pth)) u = 0;
    while (l < other.n && ijoin_less(other.key[l], other.ts[l], k, tl)) ++l;
    while (u < other.n && !ijoin_less(k, th, other.key[u], other.ts[u])) ++u;
    lb[i] = l;
    cnt[i] = !none && u > l ? (uint64_t)(u - l) : 0ull;
    pk = k, ptl = tl, pth = th;
  }
}

void ijoin_scan(const uint64_t* cnt, const int64_t* lb, int64_t n, int64_t* plan, int64_t* meta) {
  const int64_t stride = n + 1;
  uint64_t run = 0;
  int64_t m = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (cnt[i]) {
      plan[kIJoinFirst * stride + m] = (int64_t)run;
      plan[kIJoinIdx * stride + m] = i;
      plan[kIJoinLb * stride + m] = lb[i];
      ++m;
    }
    run = join_sat_add(run, cnt[i] > (uint64_t)kJoinMaxPairs ? (uint64_t)kJoinMaxPairs : cnt[i]);
  }
  plan[kIJoinFirst * stride + m] = (int64_t)run;
  meta[0] = (int64_t)run;
  meta[1] = m;
  meta[2] = run >= (uint64_t)kJoinMaxPairs ? 1 : 0;
  meta[3] = 0;
}

void ijoin_expand(const uint64_t* cnt, const int64_t* lb, const IJoinCols& batch,
                  const IJoinCols& other, int side, int64_t p0, int64_t p1, int64_t* out_key,
                  int64_t* out_l, int64_t* out_r, int64_t* out_ts) {
  if (p0 < 0 || p1 < p0) throw std::invalid_argument("ijoin_expand: bad pair range");
  uint64_t first = 0;  // the first pair of element i
  int64_t p = p0;
  for (int64_t i = 0; i < batch.n && p < p1; ++i) {
    const uint64_t c = cnt[i];
    if (first + c > (uint64_t)p) {
      for (uint64_t b = (uint64_t)p - first; b < c && p < p1; ++b, ++p) {
        const int64_t o = lb[i] + (int64_t)b;
        const int64_t bt = batch.ts[i], ot = other.ts[o];
        out_key[p - p0] = batch.key[i];
        out_l[p - p0] = side == 0 ? batch.val[i] : other.val[o];
        out_r[p - p0] = side == 0 ? other.val[o] : batch.val[i];
        out_ts[p - p0] = bt > ot ? bt : ot;
      }
    }
    first += c;
  }
  if (p != p1) throw std::invalid_argument("ijoin_expand: pair range outside [0, P)");
}

void ijoin_merge(const IJoinCols& old, const IJoinCols& batch, int64_t* out_key, int64_t* out_ts,
                 int64_t* out_val) {
  int64_t i = 0, j = 0, o = 0;
  while (i < old.n || j < batch.n) {
    // An old row goes first unless the batch row is strictly smaller.
    const bool take_old =
        j == batch.n ||
        (i < old.n && !ijoin_less(batch.key[j], batch.ts[j], old.key[i], old.ts[i]));
    const IJoinCols& s = take_old ? old : batch;
    const int64_t r = take_old ? i++ : j++;
    out_key[o] = s.key[r];
    out_ts[o] = s.ts[r];
    out_val[o] = s.val[r];
    ++o;
  }
}

int64_t ijoin_purge(const IJoinCols& src, int64_t cutoff, int64_t* out_key, int64_t* out_ts,
                    int64_t* out_val) {
  int64_t m = 0;
  for (int64_t i = 0; i < src.n; ++i) {
    if (src.ts[i] <= cutoff) continue;
    out_key[m] = src.key[i];
    out_ts[m] = src.ts[i];
    out_val[m] = src.val[i];
    ++m;
  }
  return m;
}

}  // namespace cpu
}  // namespace mxs
