// mxstream — stand-alone sanitizer harness of the counter-rate twin (csrc/rate_cpu.cpp): built
// with -fsanitize=address,undefined by mxstream.build.build_sanitize_rate and run directly.
// Drives rate_update with exactly sized tables and output columns over key spaces of 1, 7, 64, 65
// and 4097 ids, long and double counters with resets, stragglers, equal timestamps, gaps beyond
// max_gap, every comparison, long values across the 64-bit wrap, NaN / infinite / -0.0 readings,
// timestamps at both ends of the allowed range and empty batches, against a model written as a
// map; and checks that every refused rule and batch leaves the table untouched.
#include <cmath>
#include <limits>
#include <map>
#include <utility>
#include <vector>

#include "mxs_rate.h"
#include "sanitize_util.h"

using namespace mxs;

namespace {

double f64_of(int64_t b) {
  double d;
  std::memcpy(&d, &b, sizeof d);
  return d;
}

// CounterRate record by record; a key without an entry was never seen. Row = (key, rate bits,
// inc bits, dt, ts).
struct Model {
  int kind, when;
  int64_t per_ms, max_gap;  // max_gap 0: none
  double thr;
  std::map<int64_t, std::pair<int64_t, int64_t>> state;
  int64_t ignored = 0, resets = 0, gaps = 0;
  void element(int64_t k, int64_t v, int64_t t, std::vector<Row>& out) {
    auto it = state.find(k);
    if (it == state.end()) {
      state.insert({k, {t, v}});
      return;
    }
    if (t <= it->second.first) {
      ++ignored;
      return;
    }
    const int64_t dt = t - it->second.first, last = it->second.second;
    int64_t inc;
    double x;
    if (kind == kSustainDouble) {
      const double a = f64_of(v), b = f64_of(last);
      if (!(a >= b)) ++resets;
      x = a >= b ? a - b : a;
      inc = bits_of(x);
    } else {
      if (v < last) ++resets;
      inc = v >= last ? (int64_t)((uint64_t)v - (uint64_t)last) : v;
      x = (double)inc;
    }
    it->second = {t, v};
    if (max_gap && dt > max_gap) {
      ++gaps;
      return;
    }
    const double prod = x * (double)per_ms;
    const double rate = prod / (double)dt;
    if (when == kLookupAll || compare(when, rate, thr)) out.emplace_back(k, bits_of(rate), inc, dt, t);
  }
  RateRule rule() const { return rate_rule(kind, when, bits_of(thr), per_ms, max_gap); }
};

// One batch through the twin with columns of exactly n words: a write past the end is an ASan
// error.
std::vector<Row> run(const RateRule& rule, const std::vector<int64_t>& keys,
                     const std::vector<int64_t>& vals, const std::vector<int64_t>& ts,
                     std::vector<int64_t>& state, int64_t* ignored) {
  const int64_t n = (int64_t)keys.size();
  std::vector<int64_t> c[5];
  for (auto& col : c) col.assign((size_t)n, -1);
  const int64_t rows = cpu::rate_update(keys.data(), vals.data(), ts.data(), n, rule, state.data(),
                                        (int64_t)state.size() / 2, c[0].data(), c[1].data(),
                                        c[2].data(), c[3].data(), c[4].data(), ignored);
  REQUIRE(rows >= 0 && rows <= n);
  std::vector<Row> out;
  for (int64_t i = 0; i < rows; ++i)
    out.emplace_back(c[0][i], c[1][i], c[2][i], c[3][i], c[4][i]);
  return out;
}

void check_table(const Model& m, const std::vector<int64_t>& state) {
  for (size_t k = 0; k < state.size() / 2; ++k) {
    auto it = m.state.find((int64_t)k);
    if (it == m.state.end()) {
      REQUIRE(state[2 * k] == kRateNone && state[2 * k + 1] == 0);
    } else {
      REQUIRE(state[2 * k] == it->second.first && state[2 * k + 1] == it->second.second);
    }
  }
}

std::vector<int64_t> fresh(int64_t cap) {
  std::vector<int64_t> st((size_t)cap * 2, 0);
  for (int64_t k = 0; k < cap; ++k) st[2 * k] = kRateNone;
  return st;
}

int64_t random_streams() {
  const double inf = std::numeric_limits<double>::infinity();
  const double specials[] = {std::nan(""), inf, -inf, 0.0, -0.0, 1e308};
  const int64_t ispecials[] = {INT64_MAX, INT64_MIN, INT64_MIN + 5, 0, -1, ((int64_t)1 << 53) + 1};
  int64_t total = 0, resets = 0, ignored = 0, gaps = 0;
  Rng rng{13579};
  for (int64_t cap : {1, 7, 64, 65, 4097})
    for (int kind : {kSustainLong, kSustainDouble})
      for (int when = kLookupAll; when < kLookupWhens; ++when)
        for (int64_t gap : {0, 40}) {
          const int64_t pers[] = {1, 7, 1000, 60000};
          Model m{kind, when, pers[rng.below(4)], gap, when == kLookupNe ? std::nan("") : 2000.0, {}};
          const RateRule rule = m.rule();
          auto state = fresh(cap);
          std::map<int64_t, int64_t> counter;
          int64_t now = 1000, got_ignored = 0;
          for (int step = 0; step < 6; ++step) {
            const int64_t n = step == 3 ? 0 : 1 + rng.below(200);
            std::vector<int64_t> keys, vals, ts;
            std::vector<Row> want;
            for (int64_t i = 0; i < n; ++i) {
              const int64_t k = rng.below(cap);
              int64_t t = now + rng.below(60) - 30;
              if (rng.below(10) == 0) t -= 500;
              if (rng.below(100) == 0) t = rng.below(2) ? kSustainTsLimit - 1 : -kSustainTsLimit + 1;
              int64_t& c = counter[k];
              c = rng.below(50) == 0 ? rng.below(10) : c + rng.below(1000);
              int64_t v;
              if (rng.below(25) == 0)
                v = kind == kSustainDouble ? bits_of(specials[rng.below(6)]) : ispecials[rng.below(6)];
              else
                v = kind == kSustainDouble ? bits_of((double)c / 8.0) : c;
              keys.push_back(k), vals.push_back(v), ts.push_back(t);
              m.element(k, v, t, want);
            }
            const auto got = run(rule, keys, vals, ts, state, &got_ignored);
            REQUIRE(got == want);
            REQUIRE(got_ignored == m.ignored);
            check_table(m, state);
            total += (int64_t)got.size();
            now += 5 + rng.below(55);
          }
          resets += m.resets, ignored += m.ignored, gaps += m.gaps;
        }
  REQUIRE(resets > 100 && ignored > 100 && gaps > 100);
  return total;
}

void edges() {
  int64_t ign = 0;
  // a long counter: first sample, increase, straggler, duplicate, reset
  Model m{kSustainLong, kLookupAll, 1000, 0, 0.0, {}};
  auto state = fresh(2);
  auto got = run(m.rule(), {0, 0, 0, 0, 0, 1}, {100, 350, 999, 360, 7, 1}, {10, 20, 15, 20, 24, 5},
                 state, &ign);
  REQUIRE(got == (std::vector<Row>{Row(0, bits_of(25000.0), 250, 10, 20),
                                   Row(0, bits_of(1750.0), 7, 4, 24)}));
  REQUIRE(ign == 2);
  REQUIRE(state == (std::vector<int64_t>{24, 7, 5, 1}));
  // across the wrap: INT64_MAX then INT64_MIN + 5 is a reset; back up wraps to -6
  auto ws = fresh(1);
  got = run(m.rule(), {0, 0, 0}, {INT64_MAX, INT64_MIN + 5, INT64_MAX}, {1, 2, 3}, ws, &ign);
  REQUIRE(got == (std::vector<Row>{
      Row(0, bits_of((double)(INT64_MIN + 5) * 1000.0 / 1.0), INT64_MIN + 5, 1, 2),
      Row(0, bits_of(-6000.0), -6, 1, 3)}));
  // doubles: NaN after a number is a reset to NaN; a number after NaN is a reset to itself;
  // -0.0 >= 0.0 holds; per = 7 makes the product inexact
  Model d{kSustainDouble, kLookupAll, 7, 0, 0.0, {}};
  auto ds = fresh(1);
  const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
  got = run(d.rule(), {0, 0, 0, 0, 0, 0, 0}, {bits_of(1.0), bits_of(nan), bits_of(0.1), bits_of(0.0),
            bits_of(-0.0), bits_of(inf), bits_of(inf)}, {1, 2, 5, 6, 7, 8, 9}, ds, &ign);
  REQUIRE(got.size() == 6);
  REQUIRE(std::get<2>(got[0]) == bits_of(nan) && std::isnan(f64_of(std::get<1>(got[0]))));
  REQUIRE(got[1] == Row(0, bits_of(0.1 * 7.0 / 3.0), bits_of(0.1), 3, 5));
  REQUIRE(got[2] == Row(0, bits_of(0.0), bits_of(0.0), 1, 6));          // 0.0 < 0.1: reset
  REQUIRE(got[3] == Row(0, bits_of(-0.0), bits_of(-0.0), 1, 7));        // -0.0 >= 0.0
  REQUIRE(got[4] == Row(0, bits_of(inf), bits_of(inf), 1, 8));
  REQUIRE(std::isnan(f64_of(std::get<2>(got[5]))));                     // inf - inf
  // the widest span the range allows, a subnormal rate, and max_gap re-basing silently
  Model w{kSustainDouble, kLookupAll, 1, 0, 0.0, {}};
  auto wst = fresh(1);
  got = run(w.rule(), {0, 0}, {bits_of(0.0), bits_of(1e-300)},
            {-kSustainTsLimit + 1, kSustainTsLimit - 1}, wst, &ign);
  REQUIRE(got.size() == 1 && std::get<3>(got[0]) == 2 * (kSustainTsLimit - 1));
  const double sub = f64_of(std::get<1>(got[0]));
  REQUIRE(sub > 0.0 && sub < std::numeric_limits<double>::min());
  Model g{kSustainLong, kLookupLt, 1000, 40, 100.0, {}};
  auto gs = fresh(1);
  got = run(g.rule(), {0, 0, 0, 0}, {0, 1, 2, 1000}, {0, 40, 81, 100}, gs, &ign);
  REQUIRE(got == (std::vector<Row>{Row(0, bits_of(25.0), 1, 40, 40)}));
  REQUIRE(gs == (std::vector<int64_t>{100, 1000}));
  REQUIRE(run(g.rule(), {}, {}, {}, gs, &ign).empty());
}

void refusals() {
  Model m{kSustainLong, kLookupAll, 1000, 0, 0.0, {}};
  const RateRule rule = m.rule();
  auto state = fresh(2);
  const auto before = state;
  int64_t o[5][2], ign = 0;
  auto call = [&](int64_t key, int64_t ts) {
    // a good first row: the refusal must come before anything is written
    const int64_t keys[2] = {0, key}, vals[2] = {1, 2}, tss[2] = {1, ts};
    cpu::rate_update(keys, vals, tss, 2, rule, state.data(), 2, o[0], o[1], o[2], o[3], o[4], &ign);
  };
  refused([&] { call(2, 1); });
  refused([&] { call(-1, 1); });
  refused([&] { call(1, kSustainTsLimit); });
  refused([&] { call(1, -kSustainTsLimit); });
  refused([&] { call(1, INT64_MIN); });
  REQUIRE(state == before && ign == 0);
  rate_rule(kSustainDouble, kLookupNe, bits_of(std::nan("")), 1, kSustainTsLimit - 1);
  refused([&] { rate_rule(2, kLookupAll, 0, 1, 0); });
  refused([&] { rate_rule(kSustainLong, -1, 0, 1, 0); });
  refused([&] { rate_rule(kSustainLong, kLookupWhens, 0, 1, 0); });
  refused([&] { rate_rule(kSustainLong, kLookupAll, 0, 0, 0); });
  refused([&] { rate_rule(kSustainLong, kLookupAll, 0, 1, -1); });
  refused([&] { rate_rule(kSustainLong, kLookupAll, 0, 1, kSustainTsLimit); });
}

}  // namespace

int main() {
  const int64_t total = random_streams();
  REQUIRE(total > 1000);
  edges();
  refusals();
  std::printf("rate sanitize ok\n");
  return 0;
}
