// mxstream — stand-alone sanitizer harness of the rule-set twins (csrc/ruleset_cpu.cpp): built
// with -fsanitize=address,undefined by mxstream.build.build_sanitize_ruleset and run directly.
// Drives count / scan / emit over the group and tile edges (0, 1, 63, 64, 65, 4095, 4096, 4097,
// 2 * 4096 + 1 samples; nothing broken, everything broken, alternating), the rule sets (empty,
// one rule, ids {0, 5, 63}, all 64, every comparison, withdrawn and set again), NaN and signed
// zeros, against a per-sample loop over a std::map.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <utility>
#include <vector>

#include "mxs_ruleset.h"

using namespace mxs;

namespace {

#define REQUIRE(c)                                                  \
  do {                                                              \
    if (!(c)) {                                                     \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

int64_t bits(double d) {
  int64_t b;
  std::memcpy(&b, &d, sizeof b);
  return b;
}

bool model_cmp(int when, double a, double b) {
  switch (when) {
    case kLookupGt: return a > b;
    case kLookupGe: return a >= b;
    case kLookupLt: return a < b;
    case kLookupLe: return a <= b;
    case kLookupEq: return a == b;
    default: return a != b;
  }
}

struct Rules {
  std::vector<int64_t> rows;  // exactly 2 * 64 words: a read past the end is an ASan error
  std::map<int, std::pair<int, int64_t>> model;  // id -> (code, threshold bits)
  Rules() : rows(2 * kRuleSetMax, 0) {}
  void set(int id, int code, double thr) {
    rows[2 * id] = bits(thr), rows[2 * id + 1] = code;
    model[id] = {code, bits(thr)};
  }
  void withdraw(int id) {
    rows[2 * id] = 0, rows[2 * id + 1] = 0;
    model.erase(id);
  }
};

// count + scan + emit of one sample batch against the per-sample loop.
int64_t check_probe(const Rules& rs, const std::vector<int64_t>& vals) {
  const int64_t n = (int64_t)vals.size();
  std::vector<int64_t> keys(n), ts(n);
  for (int64_t i = 0; i < n; ++i) keys[i] = i % 7, ts[i] = 1000 + i;
  const int64_t ntiles = (n + kLookupTile - 1) / kLookupTile;
  std::vector<uint32_t> gsum(ntiles * kRuleSetGroups), counts(ntiles);
  cpu::ruleset_count(vals.data(), n, rs.rows.data(), gsum.data(), counts.data());
  int64_t total = 0;  // (the scan is the lookup's: csrc/tests/sanitize_lookup_main.cpp)
  for (int64_t tl = 0; tl < ntiles; ++tl) total += counts[tl];
  std::vector<int64_t> ek, ev, er, et, es;
  std::vector<uint32_t> eg(ntiles * kRuleSetGroups, 0);
  for (int64_t i = 0; i < n; ++i)
    for (const auto& r : rs.model) {
      if (!model_cmp(r.second.first, lookup_f64(vals[i]), lookup_f64(r.second.second))) continue;
      ek.push_back(keys[i]), ev.push_back(vals[i]), er.push_back(r.first);
      et.push_back(r.second.second), es.push_back(ts[i]);
      ++eg[i / 64];
    }
  REQUIRE(total == (int64_t)ek.size());
  REQUIRE(gsum == eg);
  for (int64_t tl = 0; tl < ntiles; ++tl) {
    uint32_t c = 0;
    for (int j = 0; j < kRuleSetGroups; ++j) c += gsum[tl * kRuleSetGroups + j];
    REQUIRE(counts[tl] == c);
  }
  std::vector<int64_t> ok(total), ov(total), orr(total), ot(total), os(total);
  cpu::ruleset_emit(keys.data(), vals.data(), ts.data(), n, rs.rows.data(), total, ok.data(),
                    ov.data(), orr.data(), ot.data(), os.data());
  REQUIRE(ok == ek && ov == ev && orr == er && ot == et && os == es);
  return total;
}

}  // namespace

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  Rules none, one, three, all;
  one.set(7, kLookupGt, 50.0);
  three.set(0, kLookupGt, 50.0), three.set(5, kLookupGe, 99.0), three.set(63, kLookupLt, 2.0);
  for (int r = 0; r < kRuleSetMax; ++r) all.set(r, kLookupGt, 10.0 + r / 100.0);

  // Sizes at the group and tile edges: everything broken, nothing broken, alternating.
  const int64_t sizes[] = {0, 1, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 1};
  for (const int64_t n : sizes) {
    std::vector<int64_t> hi(n), lo(n), alt(n);
    for (int64_t i = 0; i < n; ++i)
      hi[i] = bits(99.0), lo[i] = bits(5.0), alt[i] = i & 1 ? hi[i] : lo[i];
    REQUIRE(check_probe(none, hi) == 0);
    REQUIRE(check_probe(one, hi) == n && check_probe(one, lo) == 0);
    REQUIRE(check_probe(one, alt) == n / 2);
    REQUIRE(check_probe(three, hi) == 2 * n && check_probe(three, lo) == 0);
    REQUIRE(check_probe(all, hi) == 64 * n && check_probe(all, lo) == 0);
    REQUIRE(check_probe(all, alt) == 64 * (n / 2));
  }

  // Every comparison against NaN, signed zeros and the edges of the exact integers.
  const double pool[] = {51.0, 50.0, 52.0, nan, -0.0, 0.0, 9007199254740992.0,
                         -9007199254740992.0, std::numeric_limits<double>::infinity()};
  std::vector<int64_t> vals;
  for (int rep = 0; rep < 9; ++rep)
    for (const double s : pool) vals.push_back(bits(s));
  Rules every;
  int id = 0;
  for (int code = kLookupGt; code <= kLookupNe; ++code)
    for (const double t : pool) every.set(id++, code, t);
  REQUIRE(id == 54);
  check_probe(every, vals);
  // A rule withdrawn and set again; the last rule of an id wins; an unknown code is no rule.
  every.withdraw(3);
  check_probe(every, vals);
  every.set(3, kLookupNe, nan);
  every.set(3, kLookupEq, -0.0);
  check_probe(every, vals);
  every.rows[2 * 60 + 1] = 9;
  every.rows[2 * 61 + 1] = -1;
  check_probe(every, vals);
  // -0.0 == 0.0, and NaN only satisfies !=.
  Rules z;
  z.set(1, kLookupEq, 0.0);
  REQUIRE(check_probe(z, {bits(-0.0), bits(0.0), bits(nan)}) == 2);
  z.set(1, kLookupNe, nan);
  REQUIRE(check_probe(z, {bits(1.0), bits(nan)}) == 2);
  z.set(1, kLookupEq, nan);
  REQUIRE(check_probe(z, {bits(1.0), bits(nan)}) == 0);
  std::puts("ruleset sanitize ok");
  return 0;
}
