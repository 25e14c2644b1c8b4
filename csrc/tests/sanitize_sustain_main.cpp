// mxstream — stand-alone sanitizer harness of the sustained-alert twin (csrc/sustain_cpu.cpp):
// built with -fsanitize=address,undefined by mxstream.build.build_sanitize_sustain and run
// directly. Drives sustain_update with exactly sized tables and output columns over key spaces
// of 1, 7, 64, 65 and 4097 ids, all six comparisons, long and double values (NaN, infinities,
// INT64 extremes), for_ms 0 and large, timestamps at both ends of the allowed range, disorder,
// equal timestamps and empty batches, against a model written as a map of optional states; and
// checks that every refused batch leaves the table untouched.
#include <cmath>
#include <limits>
#include <map>
#include <utility>
#include <vector>

#include "mxs_sustain.h"
#include "sanitize_util.h"

using namespace mxs;

namespace {

// SustainedAlert record by record; a key without an entry has no open run.
struct Model {
  int kind, when;
  double thr;
  int64_t for_ms;
  std::map<int64_t, std::pair<int64_t, bool>> state;
  void element(int64_t k, int64_t vbits, int64_t ts, std::vector<Row>& out) {
    double v;
    if (kind == kSustainDouble) std::memcpy(&v, &vbits, sizeof v); else v = (double)vbits;
    auto it = state.find(k);
    if (compare(when, v, thr)) {
      if (it == state.end()) it = state.insert({k, {ts, false}}).first;
      if (!it->second.second && ts - it->second.first >= for_ms) {
        it->second.second = true;
        out.emplace_back(k, 1, it->second.first, vbits, ts);
      }
    } else if (it != state.end()) {
      if (it->second.second) out.emplace_back(k, 0, it->second.first, vbits, ts);
      state.erase(it);
    }
  }
};

// One batch through the twin with columns of exactly n words: a write past the end is an ASan
// error.
std::vector<Row> run(const Model& m, const std::vector<int64_t>& keys,
                     const std::vector<int64_t>& vals, const std::vector<int64_t>& ts,
                     std::vector<int64_t>& state) {
  const int64_t n = (int64_t)keys.size();
  std::vector<int64_t> c[5];
  for (auto& col : c) col.assign((size_t)n, -1);
  const int64_t rows = cpu::sustain_update(
      keys.data(), vals.data(), ts.data(), n, m.kind, m.when, bits_of(m.thr), m.for_ms,
      state.data(), (int64_t)state.size() / 2, c[0].data(), c[1].data(), c[2].data(), c[3].data(),
      c[4].data());
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
      REQUIRE(state[2 * k] == kSustainNone && state[2 * k + 1] == 0);
    } else {
      REQUIRE(state[2 * k] == it->second.first && state[2 * k + 1] == (it->second.second ? 1 : 0));
    }
  }
}

std::vector<int64_t> fresh(int64_t cap) {
  std::vector<int64_t> st((size_t)cap * 2, 0);
  for (int64_t k = 0; k < cap; ++k) st[2 * k] = kSustainNone;
  return st;
}

int64_t random_streams() {
  const double inf = std::numeric_limits<double>::infinity();
  const double specials[] = {std::nan(""), inf, -inf, 0.0, -0.0, 70.0};
  const int64_t ispecials[] = {INT64_MAX, INT64_MIN, 0, 70, 71, ((int64_t)1 << 53) + 1};
  int64_t total = 0;
  Rng rng{12345};
  for (int64_t cap : {1, 7, 64, 65, 4097})
    for (int when = kLookupGt; when < kLookupWhens; ++when)
      for (int kind : {kSustainLong, kSustainDouble})
        for (int64_t for_ms : {(int64_t)0, (int64_t)40, kSustainTsLimit}) {
          Model m{kind, when, 70.0, for_ms, {}};
          if (cap == 7 && kind == kSustainDouble && for_ms == 40) m.thr = std::nan("");
          auto state = fresh(cap);
          int64_t now = 1000;
          for (int step = 0; step < 6; ++step) {
            const int64_t n = step == 3 ? 0 : 1 + rng.below(200);
            std::vector<int64_t> keys, vals, ts;
            std::vector<Row> want;
            for (int64_t i = 0; i < n; ++i) {
              const int64_t k = rng.below(cap);
              int64_t t = now + rng.below(60) - 30;
              if (rng.below(50) == 0) t = rng.below(2) ? kSustainTsLimit - 1 : -kSustainTsLimit + 1;
              int64_t v;
              if (rng.below(20) == 0)
                v = kind == kSustainDouble ? bits_of(specials[rng.below(6)]) : ispecials[rng.below(6)];
              else
                v = kind == kSustainDouble ? bits_of(40.0 + (double)rng.below(600) / 10.0)
                                           : 40 + rng.below(60);
              keys.push_back(k), vals.push_back(v), ts.push_back(t);
              m.element(k, v, t, want);
            }
            const auto got = run(m, keys, vals, ts, state);
            REQUIRE(got == want);
            check_table(m, state);
            total += (int64_t)got.size();
            now += 5 + rng.below(55);
          }
        }
  return total;
}

void edges() {
  Model m{kSustainDouble, kLookupGt, 70.0, 50, {}};
  auto state = fresh(3);
  const int64_t b = bits_of(80.0), q = bits_of(10.0);
  // ts - since == for_ms exactly fires; one below does not
  auto got = run(m, {0, 0, 0, 1, 1, 1}, {b, b, b, b, b, q}, {0, 49, 50, 0, 49, 60}, state);
  REQUIRE(got == (std::vector<Row>{Row(0, 1, 0, b, 50)}));
  REQUIRE(state == (std::vector<int64_t>{0, 1, kSustainNone, 0, kSustainNone, 0}));
  // the resolve reports the run's since; a new run opens behind it
  got = run(m, {0, 0, 0}, {q, b, b}, {60, 70, 10}, state);
  REQUIRE(got == (std::vector<Row>{Row(0, 0, 0, q, 60)}));
  REQUIRE(state[0] == 70 && state[1] == 0);  // 10 - 70 is negative: not >= 50
  // the widest span the range allows
  got = run(m, {2, 2}, {b, b}, {-kSustainTsLimit + 1, kSustainTsLimit - 1}, state);
  REQUIRE(got == (std::vector<Row>{Row(2, 1, -kSustainTsLimit + 1, b, kSustainTsLimit - 1)}));
  REQUIRE(run(m, {}, {}, {}, state).empty());
}

void refusals() {
  auto state = fresh(2);
  const auto before = state;
  const int64_t b = bits_of(80.0);
  const int64_t thr = bits_of(70.0);
  int64_t o[5][2];
  auto call = [&](int64_t key, int64_t ts, int kind, int when, int64_t for_ms) {
    // a good first row: the refusal must come before anything is written
    const int64_t keys[2] = {0, key}, vals[2] = {b, b}, tss[2] = {1, ts};
    cpu::sustain_update(keys, vals, tss, 2, kind, when, thr, for_ms, state.data(), 2, o[0], o[1],
                        o[2], o[3], o[4]);
  };
  refused([&] { call(2, 1, kSustainDouble, kLookupGt, 0); });
  refused([&] { call(-1, 1, kSustainDouble, kLookupGt, 0); });
  refused([&] { call(1, kSustainTsLimit, kSustainDouble, kLookupGt, 0); });
  refused([&] { call(1, -kSustainTsLimit, kSustainDouble, kLookupGt, 0); });
  refused([&] { call(1, INT64_MIN, kSustainDouble, kLookupGt, 0); });
  refused([&] { call(1, 1, 2, kLookupGt, 0); });
  refused([&] { call(1, 1, kSustainDouble, kLookupAll, 0); });
  refused([&] { call(1, 1, kSustainDouble, kLookupWhens, 0); });
  refused([&] { call(1, 1, kSustainDouble, kLookupGt, -1); });
  REQUIRE(state == before);
}

}  // namespace

int main() {
  const int64_t total = random_streams();
  REQUIRE(total > 1000);
  edges();
  refusals();
  std::printf("sustain sanitize ok\n");
  return 0;
}
