// mxstream — stand-alone sanitizer harness of the burst-alert twin (csrc/burst_cpu.cpp): built
// with -fsanitize=address,undefined by mxstream.build.build_sanitize_burst and run directly.
// Drives burst_update with exactly sized rings, rows and output columns over key spaces of 1, 7,
// 64, 65 and 4097 ids, all six comparisons, long and double values (NaN, infinities, INT64
// extremes), times 2, 3, 5 and 16, within 0, 40 and the largest allowed, timestamps at both ends
// of the allowed range, disorder, equal timestamps and empty batches, against a model written
// as a map of deques; and checks that every refused batch leaves the state untouched.
#include <cmath>
#include <deque>
#include <limits>
#include <map>
#include <vector>

#include "mxs_burst.h"
#include "sanitize_util.h"

using namespace mxs;

namespace {

// BurstAlert record by record.
struct Key {
  std::deque<int64_t> recent;
  int64_t since = 0;
  bool firing = false;
};

struct Model {
  int kind, when;
  double thr;
  int times;
  int64_t within;
  std::map<int64_t, Key> state;
  void element(int64_t k, int64_t vbits, int64_t ts, std::vector<Row>& out) {
    double v;
    if (kind == kSustainDouble) std::memcpy(&v, &vbits, sizeof v); else v = (double)vbits;
    const bool breach = compare(when, v, thr);
    if (!breach && state.find(k) == state.end()) return;
    Key& s = state[k];
    if (breach) {
      s.recent.push_back(ts);
      if ((int)s.recent.size() > times) s.recent.pop_front();
    }
    const bool dense = (int)s.recent.size() == times && ts - s.recent.front() <= within;
    if (breach && dense && !s.firing) {
      s.firing = true, s.since = s.recent.front();
      out.emplace_back(k, 1, s.since, vbits, ts);
    } else if (!dense && s.firing) {
      out.emplace_back(k, 0, s.since, vbits, ts);
      s.firing = false, s.since = 0;
    }
  }
};

struct State {
  std::vector<int64_t> ring, row;
  State(int64_t cap, int times) : ring((size_t)(cap * times), 0), row((size_t)cap * 2, 0) {}
};

// One batch through the twin with columns of exactly n words: a write past the end is an ASan
// error.
std::vector<Row> run(const Model& m, const std::vector<int64_t>& keys,
                     const std::vector<int64_t>& vals, const std::vector<int64_t>& ts, State& st) {
  const int64_t n = (int64_t)keys.size();
  std::vector<int64_t> c[5];
  for (auto& col : c) col.assign((size_t)n, -1);
  const int64_t rows = cpu::burst_update(
      keys.data(), vals.data(), ts.data(), n, m.kind, m.when, bits_of(m.thr), m.times, m.within,
      st.ring.data(), st.row.data(), (int64_t)st.row.size() / 2, c[0].data(), c[1].data(),
      c[2].data(), c[3].data(), c[4].data());
  REQUIRE(rows >= 0 && rows <= n);
  std::vector<Row> out;
  for (int64_t i = 0; i < rows; ++i)
    out.emplace_back(c[0][i], c[1][i], c[2][i], c[3][i], c[4][i]);
  return out;
}

// The ring read oldest first against the model's deque.
void check_state(const Model& m, const State& st) {
  const int times = m.times;
  for (size_t k = 0; k < st.row.size() / 2; ++k) {
    const int64_t meta = st.row[2 * k + 1];
    const int firing = (int)(meta & 1), held = (int)((meta >> kBurstHeldShift) & 0x7f);
    const int pos = (int)(meta >> kBurstPosShift);
    auto it = m.state.find((int64_t)k);
    if (it == m.state.end()) {
      REQUIRE(meta == 0 && st.row[2 * k] == 0);
      continue;
    }
    const Key& s = it->second;
    REQUIRE(pos >= 0 && pos < times && held == (int)s.recent.size());
    REQUIRE(firing == (s.firing ? 1 : 0) && st.row[2 * k] == s.since);
    for (int j = 0; j < held; ++j)
      REQUIRE(st.ring[k * times + (size_t)((pos - held + j + times) % times)] == s.recent[(size_t)j]);
  }
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
        for (int times : {2, 3, 5, 16})
          for (int64_t within : {(int64_t)0, (int64_t)40, kSustainTsLimit - 1}) {
            Model m{kind, when, 70.0, times, within, {}};
            if (cap == 7 && kind == kSustainDouble && within == 40) m.thr = std::nan("");
            State st(cap, times);
            int64_t now = 1000;
            for (int step = 0; step < 6; ++step) {
              const int64_t n = step == 3 ? 0 : 1 + rng.below(200);
              std::vector<int64_t> keys, vals, ts;
              std::vector<Row> want;
              for (int64_t i = 0; i < n; ++i) {
                const int64_t k = rng.below(cap);
                int64_t t = now + rng.below(60) - 30;
                if (rng.below(50) == 0)
                  t = rng.below(2) ? kSustainTsLimit - 1 : -kSustainTsLimit + 1;
                int64_t v;
                if (rng.below(20) == 0)
                  v = kind == kSustainDouble ? bits_of(specials[rng.below(6)])
                                             : ispecials[rng.below(6)];
                else
                  v = kind == kSustainDouble ? bits_of(40.0 + (double)rng.below(600) / 10.0)
                                             : 40 + rng.below(60);
                keys.push_back(k), vals.push_back(v), ts.push_back(t);
                m.element(k, v, t, want);
              }
              const auto got = run(m, keys, vals, ts, st);
              REQUIRE(got == want);
              check_state(m, st);
              total += (int64_t)got.size();
              now += 5 + rng.below(55);
            }
          }
  return total;
}

void edges() {
  Model m{kSustainDouble, kLookupGt, 70.0, 3, 50, {}};
  State st(3, 3);
  const int64_t b = bits_of(80.0), q = bits_of(10.0);
  // ts - recent[0] == within exactly is dense; one above is not
  auto got = run(m, {0, 0, 0, 1, 1, 1}, {b, b, b, b, b, b}, {0, 49, 50, 0, 49, 51}, st);
  REQUIRE(got == (std::vector<Row>{Row(0, 1, 0, b, 50)}));
  REQUIRE(st.row[0] == 0 && st.row[1] == burst_meta(1, 3, 0));
  REQUIRE(st.row[2] == 0 && st.row[3] == burst_meta(0, 3, 0));
  // a quiet element inside the span keeps the burst; one beyond it resolves with the burst's since
  got = run(m, {0, 0, 0}, {q, q, b}, {50, 51, 52}, st);
  // and the breach behind it sees recent = (49, 50, 52): a new burst
  REQUIRE(got == (std::vector<Row>{Row(0, 0, 0, q, 51), Row(0, 1, 49, b, 52)}));
  REQUIRE(st.row[0] == 49 && st.row[1] == burst_meta(1, 3, 1));
  got = run(m, {0}, {b}, {53}, st);
  REQUIRE(got.empty() && st.row[0] == 49 && st.row[1] == burst_meta(1, 3, 2));
  // the widest span the range allows, and disorder
  Model w{kSustainLong, kLookupGe, 1.0, 2, kSustainTsLimit - 1, {}};
  State sw(1, 2);
  got = run(w, {0, 0, 0}, {1, 0, 1}, {kSustainTsLimit - 1, 5, -kSustainTsLimit + 1}, sw);
  REQUIRE(got == (std::vector<Row>{Row(0, 1, kSustainTsLimit - 1, 1, -kSustainTsLimit + 1)}));
  REQUIRE(run(w, {}, {}, {}, sw).empty());
}

void refusals() {
  State st(2, 2);
  const State before = st;
  const int64_t b = bits_of(80.0);
  const int64_t thr = bits_of(70.0);
  int64_t o[5][2];
  auto call = [&](int64_t key, int64_t ts, int kind, int when, int times, int64_t within) {
    // a good first row: the refusal must come before anything is written
    const int64_t keys[2] = {0, key}, vals[2] = {b, b}, tss[2] = {1, ts};
    cpu::burst_update(keys, vals, tss, 2, kind, when, thr, times, within, st.ring.data(),
                      st.row.data(), 2, o[0], o[1], o[2], o[3], o[4]);
  };
  refused([&] { call(2, 1, kSustainDouble, kLookupGt, 2, 0); });
  refused([&] { call(-1, 1, kSustainDouble, kLookupGt, 2, 0); });
  refused([&] { call(1, kSustainTsLimit, kSustainDouble, kLookupGt, 2, 0); });
  refused([&] { call(1, -kSustainTsLimit, kSustainDouble, kLookupGt, 2, 0); });
  refused([&] { call(1, INT64_MIN, kSustainDouble, kLookupGt, 2, 0); });
  refused([&] { call(1, 1, 2, kLookupGt, 2, 0); });
  refused([&] { call(1, 1, kSustainDouble, kLookupAll, 2, 0); });
  refused([&] { call(1, 1, kSustainDouble, kLookupWhens, 2, 0); });
  refused([&] { call(1, 1, kSustainDouble, kLookupGt, 1, 0); });
  refused([&] { call(1, 1, kSustainDouble, kLookupGt, kBurstMaxTimes + 1, 0); });
  refused([&] { call(1, 1, kSustainDouble, kLookupGt, 2, -1); });
  refused([&] { call(1, 1, kSustainDouble, kLookupGt, 2, kSustainTsLimit); });
  REQUIRE(st.ring == before.ring && st.row == before.row);
}

}  // namespace

int main() {
  const int64_t total = random_streams();
  REQUIRE(total > 1000);
  edges();
  refusals();
  std::printf("burst sanitize ok\n");
  return 0;
}
