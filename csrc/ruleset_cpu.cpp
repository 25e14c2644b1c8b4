// mxstream — C++ twins of the rule-set kernels (csrc/ruleset_hip.hip; design:
// csrc/mxs_ruleset.h). Plain loops: they define the result the kernels are compared against array
// for array.
#include <stdexcept>

#include "mxs_ruleset.h"

namespace mxs {
namespace cpu {

namespace {

// The rules that sample `vbits` breaks, bit r = rule id r.
inline uint64_t broken(const int64_t* rules, int64_t vbits) {
  const double v = lookup_f64(vbits);
  uint64_t m = 0;
  for (int r = 0; r < kRuleSetMax; ++r) {
    const int64_t code = rules[2 * r + 1];
    if (ruleset_active(code) && lookup_cmp((int)code, v, lookup_f64(rules[2 * r]))) m |= 1ull << r;
  }
  return m;
}

}  // namespace

void ruleset_count(const int64_t* vals, int64_t n, const int64_t* rules, uint32_t* gsum,
                   uint32_t* counts) {
  const int64_t ntiles = (n + kLookupTile - 1) / kLookupTile;
  for (int64_t t = 0; t < ntiles; ++t) {
    uint32_t c = 0;
    for (int j = 0; j < kRuleSetGroups; ++j) {
      uint32_t g = 0;
      for (int b = 0; b < 64; ++b) {
        const int64_t i = t * kLookupTile + j * 64 + b;
        if (i >= n) break;
        g += (uint32_t)__builtin_popcountll(broken(rules, vals[i]));
      }
      gsum[t * kRuleSetGroups + j] = g;
      c += g;
    }
    counts[t] = c;
  }
}

void ruleset_emit(const int64_t* keys, const int64_t* vals, const int64_t* ts, int64_t n,
                  const int64_t* rules, int64_t total, int64_t* out_key, int64_t* out_val,
                  int64_t* out_rule, int64_t* out_thr, int64_t* out_ts) {
  int64_t o = 0;
  for (int64_t i = 0; i < n; ++i) {
    for (uint64_t m = broken(rules, vals[i]); m; m &= m - 1) {
      if (o >= total) throw std::invalid_argument("ruleset_emit: more rows than counted");
      const int r = __builtin_ctzll(m);
      out_key[o] = keys[i];
      out_val[o] = vals[i];
      out_rule[o] = r;
      out_thr[o] = rules[2 * r];
      out_ts[o] = ts[i];
      ++o;
    }
  }
  if (o != total) throw std::invalid_argument("ruleset_emit: fewer rows than counted");
}

}  // namespace cpu
}  // namespace mxs
