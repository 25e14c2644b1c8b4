// mxstream — stand-alone sanitizer harness of the interval-join twins (csrc/ijoin_cpu.cpp):
// built with -fsanitize=address,undefined by mxstream.build.build_sanitize_ijoin and run
// directly. Drives probe / scan / expand / merge / purge over the edge cases (empty sides,
// neighbouring keys, duplicates, saturating bounds, expired rows) against a nested loop.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mxs_ijoin.h"

using namespace mxs;

namespace {

struct Rows {
  std::vector<int64_t> key, ts, val;
  IJoinCols cols() const { return IJoinCols{key.data(), ts.data(), val.data(), (int64_t)key.size()}; }
  void add(int64_t k, int64_t t, int64_t v) {
    key.push_back(k), ts.push_back(t), val.push_back(v);
  }
};

#define REQUIRE(c)                                                  \
  do {                                                              \
    if (!(c)) {                                                     \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

// Probe + scan + expand of `batch` (side 0 = left) against `other`, checked against the nested
// loop over the rule l.ts + lo <= r.ts <= l.ts + hi seen from the batch element.
int64_t check_join(const Rows& batch, const Rows& other, int side, int64_t lo, int64_t hi,
                   int64_t cutoff) {
  const int64_t rlo = side == 0 ? lo : (hi == kI64Min ? kI64Max : -hi);
  const int64_t rhi = side == 0 ? hi : (lo == kI64Min ? kI64Max : -lo);
  const int64_t n = (int64_t)batch.key.size();
  std::vector<int64_t> lb(n + 1);
  std::vector<uint64_t> cnt(n + 1);
  cpu::ijoin_probe(batch.cols(), other.cols(), rlo, rhi, cutoff, lb.data(), cnt.data());
  std::vector<int64_t> plan(kIJoinPlanCols * (n + 1)), meta(kIJoinMeta);
  cpu::ijoin_scan(cnt.data(), lb.data(), n, plan.data(), meta.data());
  const int64_t P = meta[0];
  REQUIRE(meta[2] == 0);
  std::vector<int64_t> ek, el, er, et;
  for (int64_t i = 0; i < n; ++i)
    for (size_t o = 0; o < other.key.size(); ++o) {
      const int64_t t = batch.ts[i], u = other.ts[o];
      if (other.key[o] != batch.key[i] || u <= cutoff) continue;
      if (u < ijoin_sat_add(t, rlo) || u > ijoin_sat_add(t, rhi)) continue;
      ek.push_back(batch.key[i]);
      el.push_back(side == 0 ? batch.val[i] : other.val[o]);
      er.push_back(side == 0 ? other.val[o] : batch.val[i]);
      et.push_back(t > u ? t : u);
    }
  REQUIRE(P == (int64_t)ek.size());
  // The whole range and every split of it in two.
  for (int64_t cut = 0; cut <= P; ++cut) {
    std::vector<int64_t> k(P + 1), l(P + 1), r(P + 1), t(P + 1);
    cpu::ijoin_expand(cnt.data(), lb.data(), batch.cols(), other.cols(), side, 0, cut, k.data(),
                      l.data(), r.data(), t.data());
    cpu::ijoin_expand(cnt.data(), lb.data(), batch.cols(), other.cols(), side, cut, P,
                      k.data() + cut, l.data() + cut, r.data() + cut, t.data() + cut);
    for (int64_t p = 0; p < P; ++p)
      REQUIRE(k[p] == ek[p] && l[p] == el[p] && r[p] == er[p] && t[p] == et[p]);
  }
  return P;
}

Rows merged(const Rows& old, const Rows& batch) {
  Rows out;
  const size_t n = old.key.size() + batch.key.size();
  out.key.resize(n), out.ts.resize(n), out.val.resize(n);
  cpu::ijoin_merge(old.cols(), batch.cols(), out.key.data(), out.ts.data(), out.val.data());
  for (size_t i = 1; i < n; ++i)
    REQUIRE(!ijoin_less(out.key[i], out.ts[i], out.key[i - 1], out.ts[i - 1]));
  return out;
}

}  // namespace

int main() {
  Rows empty;
  Rows other;  // keys 1, 2, 3; key 2 with duplicates
  other.add(1, 10, 100), other.add(1, 12, 101);
  other.add(2, 5, 200), other.add(2, 10, 201), other.add(2, 10, 202), other.add(2, 15, 203);
  other.add(3, 10, 300);
  Rows batch;
  batch.add(1, 30, 1);   // no match, between two that match
  batch.add(2, 10, 2), batch.add(2, 10, 3), batch.add(2, 12, 4);
  batch.add(4, 10, 5);   // no such key
  const int64_t bounds[][2] = {{-3, 5}, {0, 0}, {2, 7}, {-7, -2}, {-2, 4}, {1, -1 + 2}};
  for (const auto& b : bounds)
    for (int side = 0; side < 2; ++side) {
      check_join(batch, other, side, b[0], b[1], kI64Min);
      check_join(batch, other, side, b[0], b[1], 9);   // rows at ts <= 9 are expired
      check_join(batch, other, side, b[0], b[1], kI64Max);
      REQUIRE(check_join(batch, empty, side, b[0], b[1], kI64Min) == 0);
      REQUIRE(check_join(empty, other, side, b[0], b[1], kI64Min) == 0);
    }
  REQUIRE(check_join(batch, other, 0, 0, 0, kI64Min) == 4);

  // Saturation: ts + hi beyond I64_MAX and ts + lo below I64_MIN.
  Rows far, fb;
  far.add(7, kI64Min + 1, 1), far.add(7, -5, 2), far.add(7, kI64Max - 1, 3), far.add(7, kI64Max, 4);
  fb.add(7, kI64Min + 2, 9), fb.add(7, kI64Max - 2, 10);
  for (int side = 0; side < 2; ++side) {
    check_join(fb, far, side, -10, 10, kI64Min);
    check_join(fb, far, side, kI64Min, kI64Max, kI64Min);
    check_join(fb, far, side, kI64Min + 1, kI64Max, -6);
  }

  // Merge: ties keep the old rows first; a batch before, after and inside the old rows.
  Rows m1 = merged(other, batch);
  REQUIRE(m1.key.size() == 12);
  REQUIRE(m1.val[4] == 201 && m1.val[5] == 202 && m1.val[6] == 2 && m1.val[7] == 3);
  Rows before, after;
  before.add(0, 99, 1), after.add(9, 0, 2);
  REQUIRE(merged(other, before).val[0] == 1);
  REQUIRE(merged(other, after).val[7] == 2);
  REQUIRE(merged(empty, batch).key.size() == 5 && merged(other, empty).key.size() == 7);
  REQUIRE(merged(empty, empty).key.empty());

  // Purge keeps the order of the survivors.
  Rows kept;
  kept.key.resize(7), kept.ts.resize(7), kept.val.resize(7);
  const int64_t nk = cpu::ijoin_purge(other.cols(), 10, kept.key.data(), kept.ts.data(),
                                      kept.val.data());
  REQUIRE(nk == 2 && kept.val[0] == 101 && kept.val[1] == 203);
  REQUIRE(cpu::ijoin_purge(other.cols(), kI64Min, kept.key.data(), kept.ts.data(),
                           kept.val.data()) == 7);

  // The scan saturates at 2**62 and says so.
  std::vector<uint64_t> big = {1ull << 61, 0, 1ull << 61, 5};
  std::vector<int64_t> lb4(4, 0), plan(kIJoinPlanCols * 5), meta(kIJoinMeta);
  cpu::ijoin_scan(big.data(), lb4.data(), 4, plan.data(), meta.data());
  REQUIRE(meta[0] == kJoinMaxPairs && meta[1] == 3 && meta[2] == 1);
  std::puts("ijoin sanitize ok");
  return 0;
}
