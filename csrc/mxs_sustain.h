// mxstream — sustained-condition alerts (``stream.key_by(k).process(SustainedAlert(field, when,
// threshold, for_))``): a key is reported once when ``value <when> threshold`` has held without
// interruption for `for_ms`, and once more at the first element that ends such a run.
//
// Per element (key k, value bits v, timestamp t), in arrival order:
//   breach = ``value <when> threshold`` on two doubles (Java's rules, csrc/mxs_lookup.h
//            lookup_cmp); a long value is converted, a double is taken as it is (`kind`).
//   breach:     no open run -> since = t. Not firing and t - since >= for_ms -> firing, emit
//               (k, 1, since, v, t).
//   no breach:  firing -> emit (k, 0, since, v, t). The run is closed.
// A negative t - since (disorder) simply is not >= for_ms. Timestamps lie strictly inside
// (-2**62, 2**62), which the callers check, so t - since cannot overflow.
//
// State, for dense key ids k in [0, cap):
//   state int64[cap, 2]   row k = (since, firing 0 / 1); since == kSustainNone: no open run
//                         (then firing is 0). 16-byte rows.
//
// sustain_update: a batch in arrival order updates the table and returns its transitions as five
// int64 columns in arrival order (key id, code 1 / 0, since, value bits, ts) and their number. An
// element emits at most one row: n rows of output cannot overflow.
//
// The C++ twin (csrc/sustain_cpu.cpp) is the plain loop and defines the result. The device
// (csrc/sustain_hip.hip) takes the batch stably sorted by key with `perm` = the arrival index of
// every sorted row and scans the transition, which composes associatively:
//   a summary of a stretch of one key's elements is either
//     reset (it holds a non-breach):  the absolute state (since, firing) after the stretch, or
//     all-breach:                     (t_first, t_max) of the stretch.
//   all-breach applied to (s, f), s open:  (s, f || t_max - s >= for_ms)
//   all-breach applied to no open run:     (t_first, t_max - t_first >= for_ms)
//   x then y:  y reset -> y;  both all-breach -> (x.t_first, max(x.t_max, y.t_max));
//              x reset, y all-breach -> reset(y applied to x's state).
#pragma once
#include <cstdint>

#include "mxs_common.h"
#include "mxs_lookup.h"

namespace mxs {

constexpr int64_t kSustainNone = INT64_MIN;            // `since` of a key without an open run
constexpr int64_t kSustainTsLimit = (int64_t)1 << 62;  // |ts| must stay below it
constexpr int kSustainLong = 0, kSustainDouble = 1;    // `kind` of the value bits

MXS_HD double sustain_value(int kind, int64_t bits) {
  return kind == kSustainDouble ? lookup_f64(bits) : (double)bits;
}

// ``value <when> threshold``; `thr` is the threshold as a double.
MXS_HD bool sustain_breach(int kind, int when, int64_t vbits, double thr) {
  return lookup_cmp(when, sustain_value(kind, vbits), thr);
}

namespace gpu {
// out_tag / out_since: n words each, scratch for the unordered rows (tag = arrival << 1 | code);
// out_n: one uint32 the call zeroes and leaves at the number of transitions.
void sustain_scan(const int64_t* skeys, const int64_t* perm, const int64_t* vals,
                  const int64_t* ts, int64_t n, int kind, int when, int64_t thr_bits,
                  int64_t for_ms, int64_t* state, int64_t cap, int64_t* out_tag,
                  int64_t* out_since, uint32_t* out_n, intptr_t stream);
// The rows of sustain_scan sorted by tag -> the five columns; m rows.
void sustain_gather(const int64_t* tags, const int64_t* since, int64_t m, const int64_t* keys,
                    const int64_t* vals, const int64_t* ts, int64_t n, int64_t* out_key,
                    int64_t* out_code, int64_t* out_since, int64_t* out_val, int64_t* out_ts,
                    intptr_t stream);
}  // namespace gpu

namespace cpu {
// Arrival order; the five columns hold n words each; returns the number of transitions.
int64_t sustain_update(const int64_t* keys, const int64_t* vals, const int64_t* ts, int64_t n,
                       int kind, int when, int64_t thr_bits, int64_t for_ms, int64_t* state,
                       int64_t cap, int64_t* out_key, int64_t* out_code, int64_t* out_since,
                       int64_t* out_val, int64_t* out_ts);
}  // namespace cpu

}  // namespace mxs
