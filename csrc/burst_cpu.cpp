// mxstream — C++ twin of the burst-alert kernel (csrc/burst_hip.hip; design: csrc/mxs_burst.h).
// The plain loop in arrival order: it defines the result the kernel is compared against array
// for array.
#include <stdexcept>

#include "mxs_burst.h"

namespace mxs {
namespace cpu {

int64_t burst_update(const int64_t* keys, const int64_t* vals, const int64_t* ts, int64_t n,
                     int kind, int when, int64_t thr_bits, int times, int64_t within,
                     int64_t* ring, int64_t* row, int64_t cap, int64_t* out_key,
                     int64_t* out_code, int64_t* out_since, int64_t* out_val, int64_t* out_ts) {
  if (times < 2 || times > kBurstMaxTimes)
    throw std::invalid_argument("burst_update: times must lie in [2, 16]");
  if (within < 0 || within >= kSustainTsLimit)
    throw std::invalid_argument("burst_update: within must lie in [0, 2**62)");
  if (when <= kLookupAll || when >= kLookupWhens)
    throw std::invalid_argument("burst_update: unknown comparison");
  if (kind != kSustainLong && kind != kSustainDouble)
    throw std::invalid_argument("burst_update: unknown value kind");
  for (int64_t i = 0; i < n; ++i) {
    if (keys[i] < 0 || keys[i] >= cap)
      throw std::invalid_argument("burst_update: key outside the table");
    if (ts[i] <= -kSustainTsLimit || ts[i] >= kSustainTsLimit)
      throw std::invalid_argument("burst_update: timestamp beyond 2**62");
  }
  const double thr = lookup_f64(thr_bits);
  int64_t m = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t k = keys[i];
    int64_t* r = ring + k * times;
    int64_t& since = row[2 * k];
    const int64_t meta = row[2 * k + 1];
    int firing = (int)(meta & 1);
    int held = (int)((meta >> kBurstHeldShift) & 0x7f), pos = (int)(meta >> kBurstPosShift);
    const bool breach = sustain_breach(kind, when, vals[i], thr);
    if (breach) {
      r[pos] = ts[i];
      pos = pos + 1 == times ? 0 : pos + 1;
      if (held < times) ++held;
    }
    // held == times: slot pos, the next to be overwritten, is the oldest
    const bool dense = held == times && ts[i] - r[pos] <= within;
    int64_t code = -1;
    if (breach && dense && !firing) {
      firing = 1, since = r[pos], code = 1;
    } else if (!dense && firing) {
      code = 0;
    }
    if (code >= 0) {
      out_key[m] = k, out_code[m] = code, out_since[m] = since, out_val[m] = vals[i];
      out_ts[m] = ts[i];
      ++m;
    }
    if (code == 0) firing = 0, since = 0;
    row[2 * k + 1] = burst_meta(firing, held, pos);
  }
  return m;
}

}  // namespace cpu
}  // namespace mxs
