// mxstream — keyed latest-value lookup (``samples.connect(rules).key_by(..).process(
// LookupLatest(..))``): a rule stream upserts one value per key, every sample of the other stream
// reads the value in force for its key and only the samples that satisfy the comparison leave.
//
// State: one table int64[cap, 2]; row k = (value bits, present 0 / 1) of key id k. A key id at or
// beyond cap (or negative) has no rule.
//
// Kernels (csrc/lookup_hip.hip) and their C++ twins (csrc/lookup_cpu.cpp):
//   lookup_upsert  rules in arrival order, the last rule of a key wins. The device takes the
//                  batch stably sorted by key with `perm` = the arrival index of every sorted row;
//                  the row that ends its key's run stores (vals[perm], 1). The twin is the plain
//                  loop in arrival order.
//   lookup_mask    per sample (k, v): t = the table's value of k, else the default, else the row
//                  is dropped; kept iff `when` is kLookupAll or ``v <when> t`` on the two doubles
//                  (Java's rules: NaN is false but for !=, -0.0 == 0.0). A tile is kLookupTile
//                  rows; words[tile * 64 + j] holds rows [64 j, 64 j + 64) of the tile, bit b =
//                  row 64 j + b; counts[tile] = the tile's kept rows. Rows >= n are 0 bits.
//   lookup_scan    offsets = the exclusive scan of counts, meta[0] = the total
//   lookup_emit    the kept rows in input order as four columns (key, value bits, looked-up
//                  bits, ts): row at offsets[tile] + popcount of the tile's earlier words +
//                  popcount of the lower bits of its own word
//   lookup_gather  every row kept (no comparison, a default): the four columns without mask/scan
#pragma once
#include <cstdint>
#include <cstring>

#include "mxs_common.h"

namespace mxs {

constexpr int kLookupTile = 4096;
constexpr int kLookupWords = kLookupTile / 64;  // mask words of a tile
constexpr int kLookupMeta = 2;                  // [kept rows, unused]

enum LookupWhen : int {
  kLookupAll = 0, kLookupGt, kLookupGe, kLookupLt, kLookupLe, kLookupEq, kLookupNe, kLookupWhens
};

MXS_HD double lookup_f64(int64_t bits) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __longlong_as_double(bits);
#else
  double d;
  std::memcpy(&d, &bits, sizeof d);
  return d;
#endif
}

// ``a <when> b`` as Java compares two doubles.
MXS_HD bool lookup_cmp(int when, double a, double b) {
  switch (when) {
    case kLookupGt: return a > b;
    case kLookupGe: return a >= b;
    case kLookupLt: return a < b;
    case kLookupLe: return a <= b;
    case kLookupEq: return a == b;
    case kLookupNe: return a != b;
    default: return true;
  }
}

// One sample against the value in force: `present` says whether `tbits` holds one.
MXS_HD bool lookup_keep(int when, int64_t vbits, bool present, int64_t tbits) {
  return present && lookup_cmp(when, lookup_f64(vbits), lookup_f64(tbits));
}

namespace gpu {
void lookup_upsert(const int64_t* skeys, const int64_t* perm, const int64_t* vals, int64_t n,
                   int64_t* table, int64_t cap, intptr_t stream);
void lookup_mask(const int64_t* keys, const int64_t* vals, int64_t n, const int64_t* table,
                 int64_t cap, int when, bool has_default, int64_t default_bits, uint64_t* words,
                 uint32_t* counts, intptr_t stream);
void lookup_scan(const uint32_t* counts, int64_t ntiles, int64_t* offsets, int64_t* meta,
                 intptr_t stream);
void lookup_emit(const int64_t* keys, const int64_t* vals, const int64_t* ts, int64_t n,
                 const int64_t* table, int64_t cap, bool has_default, int64_t default_bits,
                 const uint64_t* words, const uint32_t* counts, const int64_t* offsets,
                 int64_t kept, int64_t* out_key, int64_t* out_val, int64_t* out_t, int64_t* out_ts,
                 intptr_t stream);
void lookup_gather(const int64_t* keys, const int64_t* vals, const int64_t* ts, int64_t n,
                   const int64_t* table, int64_t cap, int64_t default_bits, int64_t* out_key,
                   int64_t* out_val, int64_t* out_t, int64_t* out_ts, intptr_t stream);
}  // namespace gpu

namespace cpu {
// Arrival order, no sort: a later rule of a key overwrites the earlier one.
void lookup_upsert(const int64_t* keys, const int64_t* vals, int64_t n, int64_t* table,
                   int64_t cap);
void lookup_mask(const int64_t* keys, const int64_t* vals, int64_t n, const int64_t* table,
                 int64_t cap, int when, bool has_default, int64_t default_bits, uint64_t* words,
                 uint32_t* counts);
void lookup_scan(const uint32_t* counts, int64_t ntiles, int64_t* offsets, int64_t* meta);
void lookup_emit(const int64_t* keys, const int64_t* vals, const int64_t* ts, int64_t n,
                 const int64_t* table, int64_t cap, bool has_default, int64_t default_bits,
                 const uint64_t* words, int64_t kept, int64_t* out_key, int64_t* out_val,
                 int64_t* out_t, int64_t* out_ts);
void lookup_gather(const int64_t* keys, const int64_t* vals, const int64_t* ts, int64_t n,
                   const int64_t* table, int64_t cap, int64_t default_bits, int64_t* out_key,
                   int64_t* out_val, int64_t* out_t, int64_t* out_ts);
}  // namespace cpu

}  // namespace mxs
