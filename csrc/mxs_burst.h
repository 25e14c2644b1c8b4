// mxstream — burst alerts (``stream.key_by(k).process(BurstAlert(field, when, threshold, times,
// within))``): a key is reported once when its `times` most recent breaches of ``value <when>
// threshold`` lie within `within` ms of the current element, and once more at the first element
// for which they no longer do.
//
// Per element (key k, value bits v, timestamp t), in arrival order:
//   breach = ``value <when> threshold`` as in csrc/mxs_sustain.h (sustain_breach).
//   breach:  t is appended to the key's `recent` breaches; only the last `times` are kept.
//   dense  = `recent` holds `times` entries and t - recent[0] <= within (a negative difference,
//            disorder, is dense).
//   breach, dense, not firing -> firing, since = recent[0], emit (k, 1, since, v, t).
//   not dense, firing         -> emit (k, 0, since, v, t), not firing.
// Timestamps lie strictly inside (-2**62, 2**62), which the callers check, and within < 2**62,
// so t - recent[0] cannot overflow.
//
// State, for dense key ids k in [0, cap):
//   ring int64[cap, times]  a circular buffer of the key's last breaches' timestamps
//   row  int64[cap, 2]      (since, meta); meta = firing | held << 1 | pos << 8: held = the
//                           number of valid ring entries (<= times), pos = the slot the next
//                           breach is written to. held < times: the entries are slots
//                           pos - held .. pos - 1; held == times: slot pos is the oldest. since
//                           is 0 while the key is not firing. 16-byte rows.
//
// burst_update: a batch in arrival order updates ring and row and returns its transitions as
// five int64 columns in arrival order (key id, code 1 / 0, since, value bits, ts) and their
// number. An element emits at most one row: n rows of output cannot overflow.
//
// The C++ twin (csrc/burst_cpu.cpp) is the plain loop and defines the result. The device
// (csrc/burst_hip.hip) takes the batch stably sorted by key with `perm` = the arrival index of
// every sorted row. `dense` of an element depends only on the breaches at or before it -- a
// bounded look-back, not on the state -- and once it is known an element is one of four
// summaries over the state {off, on(since)}, which compose associatively:
//   ID      non-breach, dense:  the state stays
//   SET(t)  breach, dense:      off -> on(t); on(s) stays on(s)       (t = recent[0])
//   OFF     not dense:          -> off
//   ON(t)   arises only from composition: -> on(t)
//   x then y:  y is OFF or ON -> y;  y is ID -> x;  y is SET(t): x ID -> y, x SET -> x,
//              x OFF -> ON(t), x ON -> x.
#pragma once
#include <cstdint>

#include "mxs_common.h"
#include "mxs_lookup.h"
#include "mxs_sustain.h"

namespace mxs {

constexpr int kBurstMaxTimes = 16;     // the engine's largest `times`
constexpr int kBurstHeldShift = 1, kBurstPosShift = 8;

MXS_HD int64_t burst_meta(int firing, int held, int pos) {
  return (int64_t)firing | ((int64_t)held << kBurstHeldShift) | ((int64_t)pos << kBurstPosShift);
}

namespace gpu {
// out_tag / out_since: n words each, scratch for the unordered rows (tag = arrival << 1 | code);
// out_n: one uint32 the call zeroes and leaves at the number of transitions. The rows sorted by
// tag are gathered by sustain_gather.
void burst_scan(const int64_t* skeys, const int64_t* perm, const int64_t* vals, const int64_t* ts,
                int64_t n, int kind, int when, int64_t thr_bits, int times, int64_t within,
                int64_t* ring, int64_t* row, int64_t cap, int64_t* out_tag, int64_t* out_since,
                uint32_t* out_n, intptr_t stream);
}  // namespace gpu

namespace cpu {
// Arrival order; the five columns hold n words each; returns the number of transitions.
int64_t burst_update(const int64_t* keys, const int64_t* vals, const int64_t* ts, int64_t n,
                     int kind, int when, int64_t thr_bits, int times, int64_t within,
                     int64_t* ring, int64_t* row, int64_t cap, int64_t* out_key,
                     int64_t* out_code, int64_t* out_since, int64_t* out_val, int64_t* out_ts);
}  // namespace cpu

}  // namespace mxs
