// mxstream — stand-alone sanitizer harness of the keyed state-machine twin (csrc/fsm_cpu.cpp):
// built with -fsanitize=address,undefined by mxstream.build.build_sanitize_fsm and run directly.
// Drives fsm_update with exactly sized tables and output columns over key spaces of 1, 7, 64, 65
// and 4097 ids, machines of 1, 2, 3, 5 and 16 states and 2, 3 and 16 classes (state 15 and class
// 15, the top nibble and the last report bit), long and double values (NaN, infinities, -0.0,
// INT64 extremes), timestamps at both ends of the allowed range, disorder, equal timestamps and
// empty batches, against a model written as a map and a plain table; checks the packed
// composition against the sequential steps; and checks that every refused rule and batch
// leaves the table untouched.
#include <cmath>
#include <limits>
#include <map>
#include <utility>
#include <vector>

#include "mxs_fsm.h"
#include "sanitize_util.h"

using namespace mxs;

namespace {

// StateMachineAlert record by record; a key without an entry was never seen.
struct Model {
  int kind, initial;
  std::vector<double> bounds;
  std::vector<std::vector<int>> table;           // [state][class]
  std::vector<std::vector<bool>> report;         // [from][to]
  std::map<int64_t, std::pair<int64_t, int>> state;
  int cls(int64_t vbits) const {
    double v;
    if (kind == kSustainDouble) std::memcpy(&v, &vbits, sizeof v); else v = (double)vbits;
    int c = 0;
    for (double b : bounds) c += v >= b ? 1 : 0;
    return c;
  }
  void element(int64_t k, int64_t vbits, int64_t ts, std::vector<Row>& out) {
    auto it = state.find(k);
    if (it == state.end()) it = state.insert({k, {ts, initial}}).first;
    const int from = it->second.second, to = table[from][cls(vbits)];
    if (report[from][to]) out.emplace_back(k, from << 4 | to, it->second.first, vbits, ts);
    if (to != from) it->second.first = ts;
    it->second.second = to;
  }
  FsmRule rule() const {
    const int S = (int)table.size(), C = (int)bounds.size() + 1;
    std::vector<uint64_t> cols((size_t)C, 0);
    std::vector<uint32_t> masks((size_t)S, 0);
    for (int s = 0; s < S; ++s)
      for (int c = 0; c < C; ++c) cols[c] |= (uint64_t)table[s][c] << (4 * s);
    for (int a = 0; a < S; ++a)
      for (int b = 0; b < S; ++b)
        if (report[a][b]) masks[a] |= 1u << b;
    return fsm_rule(bounds.data(), cols.data(), masks.data(), S, C, initial, kind);
  }
};

// One batch through the twin with columns of exactly n words: a write past the end is an ASan
// error.
std::vector<Row> run(const FsmRule& rule, const std::vector<int64_t>& keys,
                     const std::vector<int64_t>& vals, const std::vector<int64_t>& ts,
                     std::vector<int64_t>& state) {
  const int64_t n = (int64_t)keys.size();
  std::vector<int64_t> c[5];
  for (auto& col : c) col.assign((size_t)n, -1);
  const int64_t rows = cpu::fsm_update(keys.data(), vals.data(), ts.data(), n, rule, state.data(),
                                       (int64_t)state.size() / 2, c[0].data(), c[1].data(),
                                       c[2].data(), c[3].data(), c[4].data());
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
      REQUIRE(state[2 * k] == kFsmNone && state[2 * k + 1] == 0);
    } else {
      REQUIRE(state[2 * k] == it->second.first && state[2 * k + 1] == it->second.second);
    }
  }
}

std::vector<int64_t> fresh(int64_t cap) {
  std::vector<int64_t> st((size_t)cap * 2, 0);
  for (int64_t k = 0; k < cap; ++k) st[2 * k] = kFsmNone;
  return st;
}

// A random machine of S states and C classes with bounds spread over the values' range.
Model machine(Rng& rng, int S, int C, int kind) {
  Model m{kind, (int)rng.below(S), {}, {}, {}, {}};
  for (int c = 1; c < C; ++c) m.bounds.push_back(40.0 + 60.0 * c / C);
  m.table.assign((size_t)S, std::vector<int>((size_t)C, 0));
  m.report.assign((size_t)S, std::vector<bool>((size_t)S, false));
  for (int s = 0; s < S; ++s)
    for (int c = 0; c < C; ++c) m.table[s][c] = (int)rng.below(S);
  for (int a = 0; a < S; ++a)
    for (int b = 0; b < S; ++b) m.report[a][b] = rng.below(3) != 0;
  m.table[S - 1][C - 1] = S - 1;  // the last state, class and report bit are used
  m.report[S - 1][S - 1] = true;
  return m;
}

int64_t random_streams() {
  const double inf = std::numeric_limits<double>::infinity();
  const double specials[] = {std::nan(""), inf, -inf, 0.0, -0.0, 70.0};
  const int64_t ispecials[] = {INT64_MAX, INT64_MIN, 0, 70, 71, ((int64_t)1 << 53) + 1};
  int64_t total = 0;
  Rng rng{24680};
  for (int64_t cap : {1, 7, 64, 65, 4097})
    for (int S : {1, 2, 3, 5, 16})
      for (int C : {2, 3, 16})
        for (int kind : {kSustainLong, kSustainDouble}) {
          Model m = machine(rng, S, C, kind);
          if (cap == 7 && C == 2) m.bounds[0] = kind == kSustainDouble ? 0.0 : 70.0;
          const FsmRule rule = m.rule();
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
            const auto got = run(rule, keys, vals, ts, state);
            REQUIRE(got == want);
            check_table(m, state);
            total += (int64_t)got.size();
            now += 5 + rng.below(55);
          }
        }
  return total;
}

// fsm_compose over a stretch equals stepping through it, from every state, for every S.
void composition() {
  Rng rng{97531};
  for (int S = 1; S <= kFsmMaxStates; ++S)
    for (int round = 0; round < 40; ++round) {
      uint64_t f[9];
      for (auto& x : f) {
        x = 0;
        for (int s = 0; s < S; ++s) x |= (uint64_t)rng.below(S) << (4 * s);
      }
      uint64_t left = f[0], right = f[8];   // both bracketings
      for (int i = 1; i < 9; ++i) left = fsm_compose(left, f[i], S);
      for (int i = 7; i >= 0; --i) right = fsm_compose(f[i], right, S);
      REQUIRE(left == right);
      for (int s = 0; s < S; ++s) {
        int st = s;
        for (uint64_t x : f) st = fsm_next(x, st);
        REQUIRE(fsm_next(left, s) == st);
      }
      if (S < kFsmMaxStates) REQUIRE((left >> (4 * S)) == 0);
    }
}

void edges() {
  // hysteresis: on at 90, off below 80; every change reported
  Model m{kSustainDouble, 0, {80.0, 90.0}, {{0, 0, 1}, {0, 1, 1}}, {{false, true}, {true, false}}, {}};
  const FsmRule rule = m.rule();
  auto state = fresh(3);
  const int64_t hi = bits_of(95.0), mid = bits_of(85.0), lo = bits_of(70.0), on = bits_of(90.0);
  // the first element ever changes the state: its since is its own timestamp
  auto got = run(rule, {0, 0, 0, 0, 1}, {hi, mid, lo, on, mid}, {10, 20, 30, 40, 50}, state);
  REQUIRE(got == (std::vector<Row>{Row(0, 0x01, 10, hi, 10), Row(0, 0x10, 10, lo, 30),
                                   Row(0, 0x01, 30, on, 40)}));
  REQUIRE(state == (std::vector<int64_t>{40, 1, 50, 0, kFsmNone, 0}));
  // since survives a batch; NaN is class 0; -0.0 meets a bound of 0.0
  got = run(rule, {1, 0}, {hi, bits_of(std::nan(""))}, {60, 5}, state);
  REQUIRE(got == (std::vector<Row>{Row(1, 0x01, 50, hi, 60), Row(0, 0x10, 40, bits_of(std::nan("")), 5)}));
  Model z{kSustainDouble, 0, {0.0}, {{0, 1}, {0, 1}}, {{false, true}, {true, false}}, {}};
  auto zs = fresh(1);
  got = run(z.rule(), {0, 0}, {bits_of(-0.0), bits_of(-1e-300)}, {1, 2}, zs);
  REQUIRE(got == (std::vector<Row>{Row(0, 0x01, 1, bits_of(-0.0), 1),
                                   Row(0, 0x10, 1, bits_of(-1e-300), 2)}));
  // the widest span the range allows
  got = run(rule, {2, 2}, {lo, hi}, {-kSustainTsLimit + 1, kSustainTsLimit - 1}, state);
  REQUIRE(got == (std::vector<Row>{Row(2, 0x01, -kSustainTsLimit + 1, hi, kSustainTsLimit - 1)}));
  REQUIRE(run(rule, {}, {}, {}, state).empty());
}

void refusals() {
  Model m{kSustainDouble, 0, {80.0, 90.0}, {{0, 0, 1}, {0, 1, 1}}, {{false, true}, {true, false}}, {}};
  const FsmRule rule = m.rule();
  auto state = fresh(2);
  const auto before = state;
  const int64_t b = bits_of(95.0);
  int64_t o[5][2];
  auto call = [&](int64_t key, int64_t ts) {
    // a good first row: the refusal must come before anything is written
    const int64_t keys[2] = {0, key}, vals[2] = {b, b}, tss[2] = {1, ts};
    cpu::fsm_update(keys, vals, tss, 2, rule, state.data(), 2, o[0], o[1], o[2], o[3], o[4]);
  };
  refused([&] { call(2, 1); });
  refused([&] { call(-1, 1); });
  refused([&] { call(1, kSustainTsLimit); });
  refused([&] { call(1, -kSustainTsLimit); });
  refused([&] { call(1, INT64_MIN); });
  REQUIRE(state == before);
  const double bounds[2] = {80.0, 90.0}, nan2[2] = {80.0, std::nan("")}, same[2] = {80.0, 80.0};
  const double inf2[2] = {80.0, std::numeric_limits<double>::infinity()};
  const uint64_t cols[3] = {0x00, 0x10, 0x11}, bad_to[3] = {0x00, 0x10, 0x21};
  const uint64_t above[3] = {0x100, 0x10, 0x11};
  const uint32_t rep[2] = {2, 1}, bad_rep[2] = {4, 1};
  fsm_rule(bounds, cols, rep, 2, 3, 1, kSustainLong);
  refused([&] { fsm_rule(bounds, cols, rep, 0, 3, 0, kSustainLong); });
  refused([&] { fsm_rule(bounds, cols, rep, 17, 3, 0, kSustainLong); });
  refused([&] { fsm_rule(bounds, cols, rep, 2, 0, 0, kSustainLong); });
  refused([&] { fsm_rule(bounds, cols, rep, 2, 17, 0, kSustainLong); });
  refused([&] { fsm_rule(bounds, cols, rep, 2, 3, 2, kSustainLong); });
  refused([&] { fsm_rule(bounds, cols, rep, 2, 3, -1, kSustainLong); });
  refused([&] { fsm_rule(bounds, cols, rep, 2, 3, 0, 2); });
  refused([&] { fsm_rule(nan2, cols, rep, 2, 3, 0, kSustainLong); });
  refused([&] { fsm_rule(inf2, cols, rep, 2, 3, 0, kSustainLong); });
  refused([&] { fsm_rule(same, cols, rep, 2, 3, 0, kSustainLong); });
  refused([&] { fsm_rule(bounds, bad_to, rep, 2, 3, 0, kSustainLong); });
  refused([&] { fsm_rule(bounds, above, rep, 2, 3, 0, kSustainLong); });
  refused([&] { fsm_rule(bounds, cols, bad_rep, 2, 3, 0, kSustainLong); });
}

}  // namespace

int main() {
  const int64_t total = random_streams();
  REQUIRE(total > 1000);
  composition();
  edges();
  refusals();
  std::printf("fsm sanitize ok\n");
  return 0;
}
