// mxstream — what the stand-alone sanitizer programs of the keyed alert rules share
// (sanitize_sustain_main.cpp, sanitize_burst_main.cpp): the check macro, the output row, the
// generator, and the comparison and the refusal test both models use. Each program is one
// translation unit, so everything here sits in an unnamed namespace.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <tuple>

#include "mxs_lookup.h"

#define REQUIRE(c)                                                  \
  do {                                                              \
    if (!(c)) {                                                     \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

namespace {

typedef std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t> Row;  // key, code, since, bits, ts

struct Rng {
  uint64_t s;
  uint64_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s >> 33;
  }
  int64_t below(int64_t n) { return (int64_t)(next() % (uint64_t)n); }
};

int64_t bits_of(double d) {
  int64_t b;
  std::memcpy(&b, &d, sizeof b);
  return b;
}

bool compare(int when, double a, double b) {
  switch (when) {
    case mxs::kLookupGt: return a > b;
    case mxs::kLookupGe: return a >= b;
    case mxs::kLookupLt: return a < b;
    case mxs::kLookupLe: return a <= b;
    case mxs::kLookupEq: return a == b;
    default: return a != b;
  }
}

// f() must throw std::invalid_argument.
template <class F>
void refused(F f) {
  bool threw = false;
  try {
    f();
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  REQUIRE(threw);
}

}  // namespace
