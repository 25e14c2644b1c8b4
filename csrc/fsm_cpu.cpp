// mxstream — C++ twin of the keyed state-machine kernels (csrc/fsm_hip.hip; design:
// csrc/mxs_fsm.h). The plain loop in arrival order: it defines the result the kernels are
// compared against array for array.
#include <stdexcept>

#include "mxs_fsm.h"

namespace mxs {
namespace cpu {

int64_t fsm_update(const int64_t* keys, const int64_t* vals, const int64_t* ts, int64_t n,
                   const FsmRule& rule, int64_t* state, int64_t cap, int64_t* out_key,
                   int64_t* out_code, int64_t* out_since, int64_t* out_val, int64_t* out_ts) {
  for (int64_t i = 0; i < n; ++i) {
    if (keys[i] < 0 || keys[i] >= cap)
      throw std::invalid_argument("fsm_update: key outside the table");
    if (ts[i] <= -kSustainTsLimit || ts[i] >= kSustainTsLimit)
      throw std::invalid_argument("fsm_update: timestamp beyond 2**62");
  }
  int64_t m = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t k = keys[i];
    int64_t& since = state[2 * k];
    int64_t& st = state[2 * k + 1];
    if (since == kFsmNone) since = ts[i], st = rule.initial;
    const int from = (int)(st & 15);
    const int to = fsm_next(fsm_function(rule, vals[i]), from);
    if (fsm_reported(rule, from, to)) {
      out_key[m] = k, out_code[m] = from << 4 | to, out_since[m] = since, out_val[m] = vals[i];
      out_ts[m] = ts[i];
      ++m;
    }
    if (to != from) since = ts[i];
    st = to;
  }
  return m;
}

}  // namespace cpu
}  // namespace mxs
