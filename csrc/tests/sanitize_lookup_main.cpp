// mxstream — stand-alone sanitizer harness of the latest-value lookup twins
// (csrc/lookup_cpu.cpp): built with -fsanitize=address,undefined by
// mxstream.build.build_sanitize_lookup and run directly. Drives upsert / mask / scan / emit /
// gather over the word and tile edges (1, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 1 rows; all
// kept, none kept, alternating), keys beyond the table, NaN and signed zeros, every comparison,
// against a per-row loop over a std::map.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <vector>

#include "mxs_lookup.h"

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
    case kLookupNe: return a != b;
    default: return true;
  }
}

struct Table {
  std::vector<int64_t> rows;  // exactly 2 * cap words: a read past the end is an ASan error
  int64_t cap;
  std::map<int64_t, int64_t> model;
  explicit Table(int64_t c) : rows(2 * c, 0), cap(c) {}
  void upsert(const std::vector<int64_t>& k, const std::vector<int64_t>& v) {
    cpu::lookup_upsert(k.data(), v.data(), (int64_t)k.size(), rows.data(), cap);
    for (size_t i = 0; i < k.size(); ++i) model[k[i]] = v[i];
  }
};

// mask + scan + emit (or gather) of one sample batch against the per-row loop.
int64_t check_probe(const Table& t, const std::vector<int64_t>& keys,
                    const std::vector<int64_t>& vals, int when, bool has_default,
                    int64_t default_bits) {
  const int64_t n = (int64_t)keys.size();
  std::vector<int64_t> ts(n);
  for (int64_t i = 0; i < n; ++i) ts[i] = 1000 + i;
  const int64_t ntiles = (n + kLookupTile - 1) / kLookupTile;
  std::vector<uint64_t> words(ntiles * kLookupWords);
  std::vector<uint32_t> counts(ntiles);
  std::vector<int64_t> offsets(ntiles), meta(kLookupMeta);
  cpu::lookup_mask(keys.data(), vals.data(), n, t.rows.data(), t.cap, when, has_default,
                   default_bits, words.data(), counts.data());
  cpu::lookup_scan(counts.data(), ntiles, offsets.data(), meta.data());
  std::vector<int64_t> ek, ev, et, es;
  for (int64_t i = 0; i < n; ++i) {
    const auto it = t.model.find(keys[i]);
    if (it == t.model.end() && !has_default) continue;
    const int64_t tb = it == t.model.end() ? default_bits : it->second;
    if (!model_cmp(when, lookup_f64(vals[i]), lookup_f64(tb))) continue;
    ek.push_back(keys[i]), ev.push_back(vals[i]), et.push_back(tb), es.push_back(ts[i]);
  }
  const int64_t kept = meta[0];
  REQUIRE(kept == (int64_t)ek.size());
  int64_t run = 0;
  for (int64_t tl = 0; tl < ntiles; ++tl) {
    REQUIRE(offsets[tl] == run);
    run += counts[tl];
  }
  std::vector<int64_t> ok(kept), ov(kept), ot(kept), os(kept);
  cpu::lookup_emit(keys.data(), vals.data(), ts.data(), n, t.rows.data(), t.cap, has_default,
                   default_bits, words.data(), kept, ok.data(), ov.data(), ot.data(), os.data());
  REQUIRE(ok == ek && ov == ev && ot == et && os == es);
  if (when == kLookupAll && has_default) {
    REQUIRE(kept == n);
    std::vector<int64_t> gk(n), gv(n), gt(n), gs(n);
    cpu::lookup_gather(keys.data(), vals.data(), ts.data(), n, t.rows.data(), t.cap, default_bits,
                       gk.data(), gv.data(), gt.data(), gs.data());
    REQUIRE(gk == ek && gv == ev && gt == et && gs == es);
  }
  return kept;
}

}  // namespace

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  // Last rule wins: 1000 rules of one key, then every key twice.
  Table one(1);
  std::vector<int64_t> k0(1000, 0), v0(1000);
  for (int i = 0; i < 1000; ++i) v0[i] = bits(i);
  one.upsert(k0, v0);
  REQUIRE(one.rows[0] == bits(999.0) && one.rows[1] == 1);
  Table t(64);
  std::vector<int64_t> rk, rv;
  for (int rep = 0; rep < 2; ++rep)
    for (int64_t k = 0; k < 64; k += 2) rk.push_back(k), rv.push_back(bits(50.0 + rep));
  t.upsert(rk, rv);
  REQUIRE(t.rows[0] == bits(51.0) && t.rows[3] == 0);
  t.upsert({}, {});

  // Sizes at the word and tile edges: all kept, none kept, alternating.
  const int64_t sizes[] = {0, 1, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 1};
  for (const int64_t n : sizes) {
    std::vector<int64_t> keys(n), hi(n), lo(n), alt(n);
    for (int64_t i = 0; i < n; ++i) {
      keys[i] = 2 * (i % 32);
      hi[i] = bits(99.0), lo[i] = bits(1.0), alt[i] = i & 1 ? hi[i] : lo[i];
    }
    REQUIRE(check_probe(t, keys, hi, kLookupGt, false, 0) == n);
    REQUIRE(check_probe(t, keys, lo, kLookupGt, false, 0) == 0);
    REQUIRE(check_probe(t, keys, alt, kLookupGt, false, 0) == n / 2);
    REQUIRE(check_probe(t, keys, alt, kLookupAll, true, bits(7.0)) == n);
    REQUIRE(check_probe(one, keys, hi, kLookupLt, false, 0) == (n + 31) / 32);  // key 0 only
  }

  // Keys without a rule, beyond the table, negative; every comparison with and without default.
  std::vector<int64_t> keys, vals;
  const double samples[] = {51.0, 50.0, 52.0, nan, -0.0, 0.0, 9007199254740992.0,
                            -9007199254740992.0};
  const int64_t ks[] = {0, 1, 2, 63, 64, 65, 1ll << 40, -1, INT64_MAX, INT64_MIN};
  for (const int64_t k : ks)
    for (const double s : samples) keys.push_back(k), vals.push_back(bits(s));
  Table z(8);
  z.upsert({0, 1, 2}, {bits(0.0), bits(-0.0), bits(nan)});
  const double defaults[] = {51.0, nan, 0.0};
  for (int when = 0; when < kLookupWhens; ++when) {
    check_probe(t, keys, vals, when, false, 0);
    check_probe(z, keys, vals, when, false, 0);
    for (const double d : defaults) {
      check_probe(t, keys, vals, when, true, bits(d));
      check_probe(z, keys, vals, when, true, bits(d));
    }
  }
  // -0.0 == 0.0, and NaN only satisfies !=.
  REQUIRE(check_probe(z, {0, 1}, {bits(-0.0), bits(0.0)}, kLookupEq, false, 0) == 2);
  REQUIRE(check_probe(z, {2, 2}, {bits(1.0), bits(nan)}, kLookupNe, false, 0) == 2);
  REQUIRE(check_probe(z, {2, 2}, {bits(1.0), bits(nan)}, kLookupEq, false, 0) == 0);
  std::puts("lookup sanitize ok");
  return 0;
}
