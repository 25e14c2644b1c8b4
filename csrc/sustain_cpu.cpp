// mxstream — C++ twin of the sustained-alert kernels (csrc/sustain_hip.hip; design:
// csrc/mxs_sustain.h). The plain loop in arrival order: it defines the result the kernels are
// compared against array for array.
#include <stdexcept>

#include "mxs_sustain.h"

namespace mxs {
namespace cpu {

int64_t sustain_update(const int64_t* keys, const int64_t* vals, const int64_t* ts, int64_t n,
                       int kind, int when, int64_t thr_bits, int64_t for_ms, int64_t* state,
                       int64_t cap, int64_t* out_key, int64_t* out_code, int64_t* out_since,
                       int64_t* out_val, int64_t* out_ts) {
  if (for_ms < 0) throw std::invalid_argument("sustain_update: for_ms must not be negative");
  if (when <= kLookupAll || when >= kLookupWhens)
    throw std::invalid_argument("sustain_update: unknown comparison");
  if (kind != kSustainLong && kind != kSustainDouble)
    throw std::invalid_argument("sustain_update: unknown value kind");
  for (int64_t i = 0; i < n; ++i) {
    if (keys[i] < 0 || keys[i] >= cap)
      throw std::invalid_argument("sustain_update: key outside the table");
    if (ts[i] <= -kSustainTsLimit || ts[i] >= kSustainTsLimit)
      throw std::invalid_argument("sustain_update: timestamp beyond 2**62");
  }
  const double thr = lookup_f64(thr_bits);
  int64_t m = 0;
  auto emit = [&](int64_t k, int64_t code, int64_t since, int64_t i) {
    out_key[m] = k, out_code[m] = code, out_since[m] = since, out_val[m] = vals[i];
    out_ts[m] = ts[i];
    ++m;
  };
  for (int64_t i = 0; i < n; ++i) {
    const int64_t k = keys[i];
    int64_t& since = state[2 * k];
    int64_t& firing = state[2 * k + 1];
    if (sustain_breach(kind, when, vals[i], thr)) {
      if (since == kSustainNone) since = ts[i], firing = 0;
      if (!firing && ts[i] - since >= for_ms) {
        firing = 1;
        emit(k, 1, since, i);
      }
    } else {
      if (since != kSustainNone && firing) emit(k, 0, since, i);
      since = kSustainNone, firing = 0;
    }
  }
  return m;
}

}  // namespace cpu
}  // namespace mxs
