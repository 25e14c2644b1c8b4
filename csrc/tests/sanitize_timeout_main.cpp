// mxstream — stand-alone sanitizer harness of the keyed timer twins (csrc/timeout_cpu.cpp):
// built with -fsanitize=address,undefined by mxstream.build.build_sanitize_timeout and run
// directly. Drives update / mask / emit over key spaces at the word and tile edges (1, 7, 63, 64,
// 65, 4095, 4096, 4097, 2 * 4096 + 1 ids) with exactly sized tables, disorder, equal timestamps,
// late elements, keys that arm again, repeated and INT64_MAX watermarks, empty batches, growth
// and both settings of MXS_TIMEOUT_TILESKIP, against a per-record model with a timer heap.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <stdexcept>
#include <tuple>
#include <utility>
#include <vector>

#include "mxs_timeout.h"

using namespace mxs;

namespace {

#define REQUIRE(c)                                                  \
  do {                                                              \
    if (!(c)) {                                                     \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

typedef std::tuple<int64_t, int64_t, int64_t, int64_t> Row;  // key, count, last, deadline

struct Rng {
  uint64_t s;
  uint64_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s >> 33;
  }
  int64_t below(int64_t n) { return (int64_t)(next() % (uint64_t)n); }
};

// CountWithTimeout record by record: de-duplicated (ts, key) timers in a heap.
struct Model {
  int64_t timeout, wm = INT64_MIN;
  std::map<int64_t, std::pair<int64_t, int64_t>> state;
  std::set<std::pair<int64_t, int64_t>> timers;
  void element(int64_t k, int64_t ts) {
    auto& s = state[k];
    s.first += 1;
    s.second = ts;
    timers.insert({ts + timeout, k});
  }
  std::vector<Row> advance(int64_t w) {
    wm = std::max(wm, w);
    std::vector<Row> out;
    while (!timers.empty() && timers.begin()->first <= wm) {
      const auto t = *timers.begin();
      timers.erase(timers.begin());
      const auto& s = state[t.second];
      if (t.first == s.second + timeout) out.emplace_back(t.second, s.first, s.second, t.first);
    }
    std::sort(out.begin(), out.end());
    return out;
  }
};

// Tables of exactly cap entries: a read or write past the end is an ASan error.
struct Tables {
  int64_t cap, timeout, wm = INT64_MIN;
  std::vector<int64_t> state, deadline, tile_min;
  Tables(int64_t c, int64_t to)
      : cap(c), timeout(to), state(2 * c, 0), deadline(c, kTimeoutNone),
        tile_min(timeout_tiles(c), kTimeoutNone) {}
  void grow(int64_t c) {
    state.resize(2 * c, 0);
    deadline.resize(c, kTimeoutNone);
    tile_min.resize(timeout_tiles(c), kTimeoutNone);
    cap = c;
  }
  void update(const std::vector<int64_t>& k, const std::vector<int64_t>& ts) {
    cpu::timeout_update(k.data(), ts.data(), (int64_t)k.size(), timeout, state.data(),
                        deadline.data(), tile_min.data(), cap);
    check();
  }
  std::vector<Row> advance(int64_t w) {
    wm = std::max(wm, w);
    const int64_t ntiles = timeout_tiles(cap);
    std::vector<uint64_t> words(ntiles * kTimeoutWords);
    std::vector<uint32_t> counts(ntiles);
    cpu::timeout_mask(deadline.data(), cap, wm, tile_min.data(), words.data(), counts.data());
    int64_t total = 0;
    for (uint32_t c : counts) total += c;
    std::vector<int64_t> ok(total), oc(total), ol(total), od(total);
    cpu::timeout_emit(state.data(), deadline.data(), cap, words.data(), counts.data(), total,
                      ok.data(), oc.data(), ol.data(), od.data());
    check();
    std::vector<Row> out;
    for (int64_t i = 0; i < total; ++i) {
      REQUIRE(i == 0 || ok[i - 1] < ok[i]);  // key order
      REQUIRE(deadline[ok[i]] == kTimeoutNone);
      out.emplace_back(ok[i], oc[i], ol[i], od[i]);
    }
    std::sort(out.begin(), out.end());
    return out;
  }
  void check() const {  // tile_min is a lower bound of its tile's deadlines
    for (int64_t k = 0; k < cap; ++k) REQUIRE(tile_min[k / kTimeoutTile] <= deadline[k]);
  }
};

void run_stream(int64_t nkeys, bool grow, uint64_t seed) {
  const int64_t timeout = 90;
  Rng rng{seed};
  Tables tab(grow ? 1 : nkeys, timeout);
  Model model;
  model.timeout = timeout;
  int64_t now = 1000, wm = 0;
  for (int step = 0; step < 24; ++step) {
    const int64_t hi = std::max<int64_t>(1, std::min(nkeys, 1 + nkeys * (step + 2) / 12));
    const int64_t n = step % 7 == 3 ? 0 : 1 + rng.below(400);
    std::vector<int64_t> keys(n), ts(n);
    for (int64_t i = 0; i < n; ++i) {
      keys[i] = rng.below(hi);
      ts[i] = now + rng.below(60) - 30 - (rng.below(10) == 0 ? 500 : 0);  // some late
    }
    if (n > 2) keys[1] = keys[0], ts[1] = ts[0];
    while (tab.cap < hi) tab.grow(std::min(nkeys, tab.cap * 2));
    tab.update(keys, ts);
    for (int64_t i = 0; i < n; ++i) model.element(keys[i], ts[i]);
    if (rng.below(10) < 7) {
      wm = std::max(wm, now - rng.below(80));
      REQUIRE(tab.advance(wm) == model.advance(wm));
      if (rng.below(2)) REQUIRE(tab.advance(wm).empty() && model.advance(wm).empty());
      if (rng.below(4) == 0) REQUIRE(tab.advance(wm - 50) == model.advance(wm - 50));
    }
    now += 5 + rng.below(55);
  }
  const std::vector<Row> last = tab.advance(INT64_MAX);
  REQUIRE(last == model.advance(INT64_MAX));
  REQUIRE(tab.advance(INT64_MAX).empty());
  for (const auto& kv : model.state) {
    REQUIRE(tab.state[2 * kv.first] == kv.second.first);
    REQUIRE(tab.state[2 * kv.first + 1] == kv.second.second);
  }
  for (int64_t k = 0; k < tab.cap; ++k) REQUIRE(tab.deadline[k] == kTimeoutNone);
}

template <class F>
bool throws(F f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

void edges() {
  Tables t(2 * kTimeoutTile + 5, 100);
  t.update({7, kTimeoutTile + 1, 2 * kTimeoutTile + 4}, {200, 50, 10});
  t.update({7}, {400});  // tile 0: bound 300, true minimum 500
  REQUIRE(t.tile_min[0] == 300 && t.tile_min[1] == 150 && t.tile_min[2] == 110);
  const bool skip = timeout_tileskip();
  REQUIRE(t.advance(120) == std::vector<Row>({Row(2 * kTimeoutTile + 4, 1, 10, 110)}));
  REQUIRE(t.tile_min[0] == (skip ? 300 : 500) && t.tile_min[2] == kTimeoutNone);
  REQUIRE(t.advance(300) == std::vector<Row>({Row(kTimeoutTile + 1, 1, 50, 150)}));
  REQUIRE(t.tile_min[0] == 500);
  // the largest deadline below the sentinel fires at INT64_MAX only once
  t.update({0}, {INT64_MAX - 101});
  REQUIRE(t.advance(INT64_MAX - 2) == std::vector<Row>({Row(7, 2, 400, 500)}));
  REQUIRE(t.advance(INT64_MAX) == std::vector<Row>({Row(0, 1, INT64_MAX - 101, INT64_MAX - 1)}));
  REQUIRE(t.advance(INT64_MAX).empty());
  // refused batches leave the tables untouched
  const std::vector<int64_t> before = t.state;
  REQUIRE(throws([&] { t.update({1, t.cap}, {1, 1}); }));
  REQUIRE(throws([&] { t.update({1, -1}, {1, 1}); }));
  REQUIRE(throws([&] { t.update({1}, {INT64_MAX - 100}); }));
  REQUIRE(throws([&] { t.update({1}, {INT64_MAX}); }));
  REQUIRE(t.state == before);
  t.update({}, {});
}

}  // namespace

int main() {
  const int64_t spaces[] = {1, 7, 63, 64, 65, kTimeoutTile - 1, kTimeoutTile, kTimeoutTile + 1,
                            2 * kTimeoutTile + 1};
  for (const char* skip : {"1", "0"}) {
    setenv("MXS_TIMEOUT_TILESKIP", skip, 1);
    for (int64_t nkeys : spaces) {
      run_stream(nkeys, false, 11 + (uint64_t)nkeys);
      run_stream(nkeys, true, 23 + (uint64_t)nkeys);
    }
    edges();
  }
  std::printf("timeout sanitize ok\n");
  return 0;
}
