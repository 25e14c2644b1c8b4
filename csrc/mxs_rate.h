// mxstream — counter rates (``stream.key_by(k).process(CounterRate(field, per, when, threshold,
// max_gap))``): a cumulative counter per key, turned into the increase and the rate between two
// consecutive accepted samples (Prometheus' increase() / irate()).
//
// Per element (key k, value bits v, timestamp t), in arrival order, with the key's row
// (last_ts, last value bits):
//   never seen:    the row becomes (t, v); nothing leaves.
//   t <= last_ts:  a duplicate or a straggler. Ignored, the row is unchanged, `out_of_order` + 1.
//   otherwise:     dt  = t - last_ts (> 0)
//                  inc = v >= last ? v - last : v      (v < last: the counter restarted, the new
//                        reading is the increase). Longs subtract with 64-bit wrap-around, doubles
//                        with one IEEE subtraction; a NaN makes >= false, so inc = v.
//                  the row becomes (t, v).
//                  dt > max_gap: nothing leaves, the key has been re-based.
//                  rate = double(inc) * double(per_ms) / double(dt): the product, then the
//                        quotient, two IEEE operations (rate_of, the one place that computes it).
//                  no rule, or ``rate <when> threshold`` on two doubles (Java's rules,
//                  csrc/mxs_lookup.h lookup_cmp): the row (k, rate bits, inc bits, dt, t) leaves.
// Timestamps lie strictly inside (-2**62, 2**62) as for the other rules; the callers check it, so
// dt cannot overflow.
//
// State, for dense key ids k in [0, cap):
//   state int64[cap, 2]   row k = (last_ts, last value bits); last_ts == kRateNone: never seen.
//                         16-byte rows.
//
// The C++ twin (csrc/rate_cpu.cpp) is the plain loop and defines the result. The device
// (csrc/rate_hip.hip) takes the batch stably sorted by key. The accepted samples of a key are the
// strict record highs of its timestamps, so an element's baseline is not the row before it but
// the exclusive prefix arg-max of (t, v) over its run, the key's row in front, earliest on ties:
//   combine(a, b) = b.t > a.t ? b : a        (a earlier; strict, so the earlier one keeps a tie)
// which is associative (it is max over the pairs ordered by t, then by reversed position), with
// the identity (kRateNone, *). One segmented scan of the pair gives `after`; `before` is the
// lane in front's `after`, or the carry. accepted = t > before.t; based = accepted and before.t
// is a timestamp. Nothing is reassociated but that selection, and inc / dt / rate are computed
// per element from the selected pair by the functions below: the device's rows, table and count
// equal the twin's bit for bit.
//
// About one row leaves per element, so the rows are not appended and sorted by arrival index as
// the other rules' few transitions are. The scan writes (inc bits, dt) at the element's ARRIVAL
// index (dt == 0: no row, a real row has dt > 0), and the rows are compacted in arrival order
// over tiles of kLookupTile elements: rate_mask (ballot words, tile counts), lookup_scan
// (csrc/mxs_lookup.h), rate_emit.
#pragma once
#include <cstdint>
#include <stdexcept>

#include "mxs_common.h"
#include "mxs_lookup.h"
#include "mxs_sustain.h"

namespace mxs {

constexpr int64_t kRateNone = INT64_MIN;  // last_ts of a key that was never seen
constexpr int64_t kRateNoGap = INT64_MAX; // max_gap of a rule without one

struct RateRule {
  int32_t kind, when;   // kSustainLong / kSustainDouble; LookupWhen (kLookupAll: no rule)
  int64_t per_ms, max_gap;
  double thr;
};

MXS_HD int64_t rate_bits(double d) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __double_as_longlong(d);
#else
  int64_t b;
  std::memcpy(&b, &d, sizeof b);
  return b;
#endif
}

// The increase from the baseline `last` to `v` (bits of `kind`), as bits of `kind`.
MXS_HD int64_t rate_increase(int kind, int64_t v, int64_t last) {
  if (kind == kSustainDouble) {
    const double a = lookup_f64(v), b = lookup_f64(last);
    return a >= b ? rate_bits(a - b) : v;
  }
  return v >= last ? (int64_t)((uint64_t)v - (uint64_t)last) : v;
}

// The rate: a multiply, then a divide. Both sides and both kernels call this one function.
MXS_HD double rate_of(int kind, int64_t inc_bits, int64_t per_ms, int64_t dt) {
  const double prod = sustain_value(kind, inc_bits) * (double)per_ms;
  return prod / (double)dt;
}

// Whether the based element (inc, dt) leaves as a row, and its rate. dt == 0: no row.
MXS_HD bool rate_keep(const RateRule& r, int64_t inc_bits, int64_t dt, double* rate) {
  if (dt <= 0 || dt > r.max_gap) return false;
  *rate = rate_of(r.kind, inc_bits, r.per_ms, dt);
  return r.when == kLookupAll || lookup_cmp(r.when, *rate, r.thr);
}

// The checked rule of both sides. `max_gap` 0: none. Throws std::invalid_argument.
inline RateRule rate_rule(int kind, int when, int64_t thr_bits, int64_t per_ms, int64_t max_gap) {
  if (kind != kSustainLong && kind != kSustainDouble)
    throw std::invalid_argument("rate: unknown value kind");
  if (when < 0 || when >= kLookupWhens) throw std::invalid_argument("rate: unknown comparison");
  if (per_ms < 1) throw std::invalid_argument("rate: per_ms must be >= 1");
  if (max_gap < 0 || max_gap >= kSustainTsLimit)
    throw std::invalid_argument("rate: max_gap must lie in [1, 2**62), or be 0 for none");
  RateRule r = {};
  r.kind = kind, r.when = when, r.per_ms = per_ms;
  r.max_gap = max_gap ? max_gap : kRateNoGap;
  r.thr = lookup_f64(thr_bits);
  return r;
}

namespace gpu {
// The batch sorted by key (skeys, perm = arrival index of each sorted row). scratch: n rows of
// (inc bits, dt), 16-byte aligned, written at every arrival index; out_ooo: one uint32 the call
// zeroes and leaves at the number of ignored elements.
void rate_scan(const int64_t* skeys, const int64_t* perm, const int64_t* vals, const int64_t* ts,
               int64_t n, int kind, int64_t* state, int64_t cap, int64_t* scratch,
               uint32_t* out_ooo, intptr_t stream);
// words / counts: lookup_mask's layout (csrc/mxs_lookup.h) over the scratch rows.
void rate_mask(const int64_t* scratch, int64_t n, const RateRule& rule, uint64_t* words,
               uint32_t* counts, intptr_t stream);
// The kept rows in arrival order -> the five columns; `kept` is lookup_scan's total.
void rate_emit(const int64_t* scratch, const int64_t* keys, const int64_t* ts, int64_t n,
               const RateRule& rule, const uint64_t* words, const uint32_t* counts,
               const int64_t* offsets, int64_t kept, int64_t* out_key, int64_t* out_rate,
               int64_t* out_inc, int64_t* out_dt, int64_t* out_ts, intptr_t stream);
}  // namespace gpu

namespace cpu {
// Arrival order; the five columns hold n words each; returns the number of rows and adds the
// ignored elements to *out_of_order.
int64_t rate_update(const int64_t* keys, const int64_t* vals, const int64_t* ts, int64_t n,
                    const RateRule& rule, int64_t* state, int64_t cap, int64_t* out_key,
                    int64_t* out_rate, int64_t* out_inc, int64_t* out_dt, int64_t* out_ts,
                    int64_t* out_of_order);
}  // namespace cpu

}  // namespace mxs
