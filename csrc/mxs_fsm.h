// mxstream — keyed state machines (``stream.key_by(k).process(StateMachineAlert(field, bounds,
// table, initial, report))``): one finite state machine per key, stepped by every sample, and a
// row for every reported transition.
//
// Per element (key k, value bits v, timestamp t), in arrival order:
//   class = the number of bounds b with ``value >= b`` on two doubles (Java's rules: a NaN is
//           class 0, -0.0 >= 0.0 holds); a long value is converted, a double is taken as it is
//           (`kind`, csrc/mxs_sustain.h). The bounds ascend, so the bounds met are a prefix.
//   the key's first element ever: the key enters `initial` with since = t.
//   to = table[from][class]; (from, to) reported -> emit (k, from << 4 | to, since, v, t), since
//   being the timestamp at which the key entered `from`; to != from -> since = t.
// Timestamps lie strictly inside (-2**62, 2**62) as for the other rules; the callers check it.
//
// State, for dense key ids k in [0, cap):
//   state int64[cap, 2]   row k = (since, state); since == kFsmNone: the key was never seen (then
//                         state is 0). 16-byte rows.
//
// The rule (FsmRule) holds at most 16 states and 16 classes:
//   bounds[C - 1]  the class bounds, finite, strictly ascending
//   cols[C]        the table by columns: nibble s of cols[c] is table[s][c]. A column is the
//                  function S -> S an element of class c applies, packed 4 bits per state
//   report[4]      bit ``from * 16 + to`` (word from / 4) is set for a reported pair
//
// fsm_update: a batch in arrival order updates the table and returns the reported transitions as
// five int64 columns in arrival order (key id, from << 4 | to, since, value bits, ts) and their
// number. An element emits at most one row: n rows of output cannot overflow.
//
// The C++ twin (csrc/fsm_cpu.cpp) is the plain loop and defines the result. The device
// (csrc/fsm_hip.hip) takes the batch stably sorted by key and scans the packed functions, which
// compose associatively: x then y is z[s] = y[x[s]], nibble by nibble (fsm_compose). The state
// after an element is nibble `carry` of the composition of its run so far, `carry` being the
// key's stored state (or `initial`). Nothing is reassociated but function composition over
// integers: the device's rows and table equal the twin's bit for bit.
#pragma once
#include <cmath>
#include <cstdint>
#include <stdexcept>

#include "mxs_common.h"
#include "mxs_sustain.h"

namespace mxs {

constexpr int64_t kFsmNone = INT64_MIN;  // `since` of a key that was never seen
constexpr int kFsmMaxStates = 16, kFsmMaxClasses = 16;
constexpr int kFsmTagBits = 8;           // a row's tag = arrival << 8 | from << 4 | to

struct FsmRule {
  double bounds[kFsmMaxClasses - 1];
  uint64_t cols[kFsmMaxClasses];
  uint64_t report[4];
  int32_t states, classes, initial, kind;
};

// The function of an element: the column of its class. A loop over the rule's own bounds with
// the same trip count in every lane; the last bound met wins, since they ascend.
MXS_HD uint64_t fsm_function(const FsmRule& r, int64_t vbits) {
  const double v = sustain_value(r.kind, vbits);
  uint64_t f = r.cols[0];
  for (int c = 1; c < r.classes; ++c)
    if (v >= r.bounds[c - 1]) f = r.cols[c];
  return f;
}

MXS_HD int fsm_next(uint64_t f, int state) { return (int)((f >> (4u * (unsigned)state)) & 15ull); }

// x, then y: z[s] = y[x[s]] for the rule's `states` states. Unsigned 64-bit throughout: state
// 15's nibble sits at bits 60-63.
MXS_HD uint64_t fsm_compose(uint64_t x, uint64_t y, int states) {
  uint64_t z = 0;
  for (int s = 0; s < states; ++s) {
    const unsigned sh = 4u * (unsigned)s;
    const unsigned via = (unsigned)(x >> sh) & 15u;
    z |= ((y >> (4u * via)) & 15ull) << sh;
  }
  return z;
}

MXS_HD bool fsm_reported(const FsmRule& r, int from, int to) {
  const unsigned w = (unsigned)from >> 2;
  // a select chain, not an indexed load: `from` differs from lane to lane on the device
  const uint64_t m = w == 0 ? r.report[0] : w == 1 ? r.report[1] : w == 2 ? r.report[2]
                                                                         : r.report[3];
  return (m >> (((unsigned)from & 3u) * 16u + (unsigned)to)) & 1ull;
}

// The checked rule of both sides: `bounds` classes - 1 doubles, `cols` classes words, `report`
// states masks (bit `to` of report[from]). Throws std::invalid_argument.
inline FsmRule fsm_rule(const double* bounds, const uint64_t* cols, const uint32_t* report,
                        int states, int classes, int initial, int kind) {
  if (states < 1 || states > kFsmMaxStates)
    throw std::invalid_argument("fsm: states must lie in [1, 16]");
  if (classes < 1 || classes > kFsmMaxClasses)
    throw std::invalid_argument("fsm: classes must lie in [1, 16]");
  if (initial < 0 || initial >= states)
    throw std::invalid_argument("fsm: the initial state is no state");
  if (kind != kSustainLong && kind != kSustainDouble)
    throw std::invalid_argument("fsm: unknown value kind");
  FsmRule r = {};
  r.states = states, r.classes = classes, r.initial = initial, r.kind = kind;
  for (int c = 0; c + 1 < classes; ++c) {
    if (!std::isfinite(bounds[c]) || (c && !(bounds[c - 1] < bounds[c])))
      throw std::invalid_argument("fsm: the bounds must be finite and strictly ascending");
    r.bounds[c] = bounds[c];
  }
  for (int c = 0; c < classes; ++c) {
    for (int s = 0; s < kFsmMaxStates; ++s) {
      const int to = fsm_next(cols[c], s);
      if (s < states ? to >= states : to != 0)
        throw std::invalid_argument("fsm: a table entry is no state");
    }
    r.cols[c] = cols[c];
  }
  for (int s = 0; s < states; ++s) {
    if (report[s] >> states) throw std::invalid_argument("fsm: a reported pair is no state");
    r.report[s >> 2] |= (uint64_t)report[s] << ((s & 3) * 16);
  }
  return r;
}

namespace gpu {
// out_tag / out_since: n words each, scratch for the unordered rows (tag = arrival << 8 |
// from << 4 | to); out_n: one uint32 the call zeroes and leaves at the number of rows.
void fsm_scan(const int64_t* skeys, const int64_t* perm, const int64_t* vals, const int64_t* ts,
              int64_t n, const FsmRule& rule, int64_t* state, int64_t cap, int64_t* out_tag,
              int64_t* out_since, uint32_t* out_n, intptr_t stream);
// The rows of fsm_scan sorted by tag -> the five columns; m rows.
void fsm_gather(const int64_t* tags, const int64_t* since, int64_t m, const int64_t* keys,
                const int64_t* vals, const int64_t* ts, int64_t n, int64_t* out_key,
                int64_t* out_code, int64_t* out_since, int64_t* out_val, int64_t* out_ts,
                intptr_t stream);
}  // namespace gpu

namespace cpu {
// Arrival order; the five columns hold n words each; returns the number of rows.
int64_t fsm_update(const int64_t* keys, const int64_t* vals, const int64_t* ts, int64_t n,
                   const FsmRule& rule, int64_t* state, int64_t cap, int64_t* out_key,
                   int64_t* out_code, int64_t* out_since, int64_t* out_val, int64_t* out_ts);
}  // namespace cpu

}  // namespace mxs
