// mxstream — AddressSanitizer / UndefinedBehaviorSanitizer program over the reorder-buffer twins
// (csrc/reorder_cpu.cpp). A small chunked buffer built from the three twins and std::stable_sort
// -- the shape of runtime/reorder_operator.py -- runs random disordered streams against a
// brute-force list: every release equal row for row, ties in arrival order, the guards of the
// twins hit on purpose. Prints "reorder sanitize ok".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <stdexcept>
#include <tuple>
#include <vector>

#include "mxs_reorder.h"

using namespace mxs;

namespace {

#define REQUIRE(c)                                                     \
  do {                                                                 \
    if (!(c)) {                                                        \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                    \
    }                                                                  \
  } while (0)

using Col = std::vector<int64_t>;
struct Rows {
  Col key, ts, bits;
  bool operator==(const Rows& o) const { return key == o.key && ts == o.ts && bits == o.bits; }
};
struct Chunk {
  int64_t offset, head, n;
};

struct Buffer {
  Col key, ts, bits;  // the arena: exactly `tail` words each, so ASan sees every overrun
  std::vector<Chunk> chunks;
  int64_t wm = INT64_MIN, late = 0;
  size_t max_chunks;
  explicit Buffer(size_t mc) : max_chunks(mc) {}

  // indices of the given ranges in (ts, arrival) order
  Col sorted_src(const Col& begin, const Col& count, int64_t lo) const {
    Col dest(begin.size() + 1, 0);
    for (size_t c = 0; c < begin.size(); ++c) dest[c + 1] = dest[c] + count[c];
    const int64_t total = dest.back();
    Col k(total), src(total), b = begin;
    b.push_back(0);
    cpu::reorder_collect(ts.data(), (int64_t)ts.size(), b.data(), dest.data(),
                         (int64_t)begin.size(), total, lo, k.data(), src.data());
    Col order(total);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
      return (uint64_t)k[x] < (uint64_t)k[y];
    });
    Col out(total);
    for (int64_t i = 0; i < total; ++i) out[i] = src[order[i]];
    return out;
  }

  void consolidate() {
    Col begin, count;
    int64_t lo = INT64_MAX;
    for (const Chunk& c : chunks) {
      begin.push_back(c.offset + c.head);
      count.push_back(c.n - c.head);
      lo = std::min(lo, ts[c.offset + c.head]);
    }
    const Col src = sorted_src(begin, count, chunks.empty() ? 0 : lo);
    Rows fresh{Col(src.size()), Col(src.size()), Col(src.size())};
    cpu::reorder_gather(src.data(), (int64_t)src.size(), key.data(), ts.data(), bits.data(),
                        (int64_t)ts.size(), fresh.key.data(), fresh.ts.data(), fresh.bits.data());
    key = fresh.key, ts = fresh.ts, bits = fresh.bits;
    chunks.clear();
    if (!src.empty()) chunks.push_back({0, 0, (int64_t)src.size()});
  }

  void push(const Rows& b) {
    const int64_t n = (int64_t)b.ts.size();
    Col perm;
    for (int64_t i = 0; i < n; ++i) {
      if (b.ts[i] <= wm) ++late; else perm.push_back(i);
    }
    if (perm.empty()) return;
    std::stable_sort(perm.begin(), perm.end(),
                     [&](int64_t x, int64_t y) { return b.ts[x] < b.ts[y]; });
    const int64_t t = (int64_t)ts.size(), live = (int64_t)perm.size();
    key.resize(t + live), ts.resize(t + live), bits.resize(t + live);
    cpu::reorder_gather(perm.data(), live, b.key.data(), b.ts.data(), b.bits.data(), n,
                        key.data() + t, ts.data() + t, bits.data() + t);
    chunks.push_back({t, 0, live});
    if (chunks.size() > max_chunks) consolidate();
  }

  Rows release(int64_t w) {
    Rows out;
    if (w <= wm) return out;
    const int64_t prev = wm;
    wm = w;
    const int64_t k = (int64_t)chunks.size();
    if (k == 0) return out;
    Col begin(k), end(k), cut(k), count(k);
    for (int64_t c = 0; c < k; ++c)
      begin[c] = chunks[c].offset + chunks[c].head, end[c] = chunks[c].offset + chunks[c].n;
    cpu::reorder_cut(ts.data(), (int64_t)ts.size(), begin.data(), end.data(), k, w, cut.data());
    for (int64_t c = 0; c < k; ++c) {
      REQUIRE(cut[c] == reorder_upper_bound(ts.data(), begin[c], end[c], w));
      count[c] = cut[c] - begin[c];
    }
    // a chunk is ascending: the smallest live timestamp is some chunk's first, and it lies
    // above the previous watermark
    int64_t lo = INT64_MAX;
    for (int64_t c = 0; c < k; ++c) lo = std::min(lo, ts[begin[c]]);
    REQUIRE(lo > prev);
    const Col src = sorted_src(begin, count, lo);
    out = Rows{Col(src.size()), Col(src.size()), Col(src.size())};
    cpu::reorder_gather(src.data(), (int64_t)src.size(), key.data(), ts.data(), bits.data(),
                        (int64_t)ts.size(), out.key.data(), out.ts.data(), out.bits.data());
    std::vector<Chunk> rest;
    for (int64_t c = 0; c < k; ++c) {
      chunks[c].head += count[c];
      if (chunks[c].head < chunks[c].n) rest.push_back(chunks[c]);
    }
    chunks = rest;
    if (chunks.empty()) key.clear(), ts.clear(), bits.clear();
    return out;
  }
};

struct Model {
  std::vector<std::tuple<int64_t, int64_t, int64_t, int64_t>> rows;  // ts, seq, key, bits
  int64_t wm = INT64_MIN, seq = 0, late = 0;
  void push(const Rows& b) {
    for (size_t i = 0; i < b.ts.size(); ++i, ++seq) {
      if (b.ts[i] <= wm) ++late; else rows.emplace_back(b.ts[i], seq, b.key[i], b.bits[i]);
    }
  }
  Rows release(int64_t w) {
    Rows out;
    if (w <= wm) return out;
    wm = w;
    std::sort(rows.begin(), rows.end());
    size_t i = 0;
    for (; i < rows.size() && std::get<0>(rows[i]) <= w; ++i) {
      out.ts.push_back(std::get<0>(rows[i]));
      out.key.push_back(std::get<2>(rows[i]));
      out.bits.push_back(std::get<3>(rows[i]));
    }
    rows.erase(rows.begin(), rows.begin() + i);
    return out;
  }
};

void stream(uint32_t seed, size_t max_chunks, int64_t base) {
  std::mt19937_64 rng(seed);
  auto below = [&](int64_t n) { return (int64_t)(rng() % (uint64_t)n); };
  Buffer buf(max_chunks);
  Model model;
  int64_t now = base + 1000;
  for (int step = 0; step < 60; ++step) {
    const int64_t n = step % 7 == 3 ? 0 : 1 + below(step % 11 == 0 ? 9000 : 300);
    Rows b{Col(n), Col(n), Col(n)};
    for (int64_t i = 0; i < n; ++i) {
      b.key[i] = below(50);
      b.ts[i] = now + below(60) - 30 - (below(10) == 0 ? 500 : 0);
      b.bits[i] = (int64_t)rng();
    }
    if (n > 2) b.ts[1] = b.ts[0];
    buf.push(b);
    model.push(b);
    if (below(10) < 7) {
      const int64_t w = now - below(80);
      REQUIRE(buf.release(w) == model.release(w));
      if (below(3) == 0) REQUIRE(buf.release(w - 50).ts.empty());
    }
    REQUIRE(buf.late == model.late);
    now += 5 + below(55);
  }
  REQUIRE(buf.release(INT64_MAX) == model.release(INT64_MAX));
  REQUIRE(buf.chunks.empty() && buf.ts.empty() && model.rows.empty() && model.late > 0);
}

template <class F>
bool refuses(F f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

void guards() {
  const Col ts = {1, 2, 3, 4};
  Col cut(1), k(4), src(4), d0(2), d1(2), d2(2);
  const Col b_ok = {1}, e_bad = {5}, e_rev = {0}, neg = {-1}, e_ok = {4};
  REQUIRE(refuses([&] { cpu::reorder_cut(ts.data(), 4, b_ok.data(), e_bad.data(), 1, 9, cut.data()); }));
  REQUIRE(refuses([&] { cpu::reorder_cut(ts.data(), 4, b_ok.data(), e_rev.data(), 1, 9, cut.data()); }));
  REQUIRE(refuses([&] { cpu::reorder_cut(ts.data(), 4, neg.data(), e_ok.data(), 1, 9, cut.data()); }));
  cpu::reorder_cut(ts.data(), 4, b_ok.data(), e_ok.data(), 1, INT64_MAX, cut.data());
  REQUIRE(cut[0] == 4);
  cpu::reorder_cut(ts.data(), 4, b_ok.data(), e_ok.data(), 1, INT64_MIN, cut.data());
  REQUIRE(cut[0] == 1);
  const Col begin = {2, 0}, dest_over = {0, 3}, dest_gap = {1, 3}, dest_ok = {0, 2};
  REQUIRE(refuses([&] {
    cpu::reorder_collect(ts.data(), 4, begin.data(), dest_over.data(), 1, 3, 0, k.data(), src.data());
  }));
  REQUIRE(refuses([&] {
    cpu::reorder_collect(ts.data(), 4, begin.data(), dest_gap.data(), 1, 3, 0, k.data(), src.data());
  }));
  cpu::reorder_collect(ts.data(), 4, begin.data(), dest_ok.data(), 1, 2, 3, k.data(), src.data());
  REQUIRE(k[0] == 0 && k[1] == 1 && src[0] == 2 && src[1] == 3);
  const Col perm_bad = {0, 4}, perm_neg = {-1, 0};
  for (const Col* p : {&perm_bad, &perm_neg})
    REQUIRE(refuses([&] {
      cpu::reorder_gather(p->data(), 2, ts.data(), ts.data(), ts.data(), 4, d0.data(), d1.data(),
                          d2.data());
    }));
}

}  // namespace

int main() {
  guards();
  for (uint32_t seed = 0; seed < 6; ++seed) {
    stream(seed, 256, 0);
    stream(seed, 3, -(int64_t(1) << 61));  // consolidation at almost every push
    stream(seed, 1, (int64_t(1) << 62) - 100000);
  }
  // the widest span: rows at both ends of (-2**62, 2**62)
  {
    const int64_t lim = (int64_t(1) << 62) - 1;
    Buffer buf(4);
    Model model;
    const Rows a{{1, 2}, {lim, -lim}, {7, 8}}, b{{3, 4}, {-1, -lim}, {9, 10}};
    buf.push(a), model.push(a), buf.push(b), model.push(b);
    REQUIRE(buf.release(-1) == model.release(-1));
    REQUIRE(buf.release(INT64_MAX) == model.release(INT64_MAX));
  }
  std::puts("reorder sanitize ok");
  return 0;
}
