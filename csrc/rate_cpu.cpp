// mxstream — C++ twin of the counter-rate kernels (csrc/rate_hip.hip; design: csrc/mxs_rate.h).
// The plain loop in arrival order: it defines the result the kernels are compared against array
// for array.
#include <stdexcept>

#include "mxs_rate.h"

namespace mxs {
namespace cpu {

int64_t rate_update(const int64_t* keys, const int64_t* vals, const int64_t* ts, int64_t n,
                    const RateRule& rule, int64_t* state, int64_t cap, int64_t* out_key,
                    int64_t* out_rate, int64_t* out_inc, int64_t* out_dt, int64_t* out_ts,
                    int64_t* out_of_order) {
  for (int64_t i = 0; i < n; ++i) {
    if (keys[i] < 0 || keys[i] >= cap)
      throw std::invalid_argument("rate_update: key outside the table");
    if (ts[i] <= -kSustainTsLimit || ts[i] >= kSustainTsLimit)
      throw std::invalid_argument("rate_update: timestamp beyond 2**62");
  }
  int64_t m = 0, ignored = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t k = keys[i], t = ts[i], v = vals[i];
    int64_t& last_ts = state[2 * k];
    int64_t& last = state[2 * k + 1];
    if (last_ts == kRateNone) {
      last_ts = t, last = v;
      continue;
    }
    if (t <= last_ts) {
      ++ignored;
      continue;
    }
    const int64_t dt = t - last_ts;
    const int64_t inc = rate_increase(rule.kind, v, last);
    last_ts = t, last = v;
    double rate;
    if (!rate_keep(rule, inc, dt, &rate)) continue;
    out_key[m] = k, out_rate[m] = rate_bits(rate), out_inc[m] = inc, out_dt[m] = dt;
    out_ts[m] = t;
    ++m;
  }
  *out_of_order += ignored;
  return m;
}

}  // namespace cpu
}  // namespace mxs
