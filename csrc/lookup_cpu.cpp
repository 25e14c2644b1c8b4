// mxstream — C++ twins of the latest-value lookup kernels (csrc/lookup_hip.hip; design:
// csrc/mxs_lookup.h). Plain loops: they define the result the kernels are compared against array
// for array.
#include <stdexcept>

#include "mxs_lookup.h"

namespace mxs {
namespace cpu {

namespace {

// The value in force for key k: the table's, else the default (when there is one).
inline bool in_force(const int64_t* table, int64_t cap, int64_t k, bool has_default,
                     int64_t default_bits, int64_t* tbits) {
  if (k >= 0 && k < cap && table[2 * k + 1] != 0) {
    *tbits = table[2 * k];
    return true;
  }
  *tbits = default_bits;
  return has_default;
}

void check_when(int when) {
  if (when < 0 || when >= kLookupWhens) throw std::invalid_argument("lookup: unknown comparison");
}

}  // namespace

void lookup_upsert(const int64_t* keys, const int64_t* vals, int64_t n, int64_t* table,
                   int64_t cap) {
  for (int64_t i = 0; i < n; ++i) {
    const int64_t k = keys[i];
    if (k < 0 || k >= cap) throw std::invalid_argument("lookup_upsert: key outside the table");
    table[2 * k] = vals[i];
    table[2 * k + 1] = 1;
  }
}

void lookup_mask(const int64_t* keys, const int64_t* vals, int64_t n, const int64_t* table,
                 int64_t cap, int when, bool has_default, int64_t default_bits, uint64_t* words,
                 uint32_t* counts) {
  check_when(when);
  const int64_t ntiles = (n + kLookupTile - 1) / kLookupTile;
  for (int64_t t = 0; t < ntiles; ++t) {
    uint32_t c = 0;
    for (int j = 0; j < kLookupWords; ++j) {
      uint64_t w = 0;
      for (int b = 0; b < 64; ++b) {
        const int64_t i = t * kLookupTile + j * 64 + b;
        if (i >= n) break;
        int64_t tb;
        const bool present = in_force(table, cap, keys[i], has_default, default_bits, &tb);
        if (lookup_keep(when, vals[i], present, tb)) {
          w |= 1ull << b;
          ++c;
        }
      }
      words[t * kLookupWords + j] = w;
    }
    counts[t] = c;
  }
}

void lookup_scan(const uint32_t* counts, int64_t ntiles, int64_t* offsets, int64_t* meta) {
  int64_t run = 0;
  for (int64_t t = 0; t < ntiles; ++t) {
    offsets[t] = run;
    run += counts[t];
  }
  meta[0] = run;
  meta[1] = 0;
}

void lookup_emit(const int64_t* keys, const int64_t* vals, const int64_t* ts, int64_t n,
                 const int64_t* table, int64_t cap, bool has_default, int64_t default_bits,
                 const uint64_t* words, int64_t kept, int64_t* out_key, int64_t* out_val,
                 int64_t* out_t, int64_t* out_ts) {
  int64_t o = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (!((words[i >> 6] >> (i & 63)) & 1ull)) continue;
    if (o >= kept) throw std::invalid_argument("lookup_emit: more kept rows than counted");
    int64_t tb;
    in_force(table, cap, keys[i], has_default, default_bits, &tb);
    out_key[o] = keys[i];
    out_val[o] = vals[i];
    out_t[o] = tb;
    out_ts[o] = ts[i];
    ++o;
  }
  if (o != kept) throw std::invalid_argument("lookup_emit: fewer kept rows than counted");
}

void lookup_gather(const int64_t* keys, const int64_t* vals, const int64_t* ts, int64_t n,
                   const int64_t* table, int64_t cap, int64_t default_bits, int64_t* out_key,
                   int64_t* out_val, int64_t* out_t, int64_t* out_ts) {
  for (int64_t i = 0; i < n; ++i) {
    int64_t tb;
    in_force(table, cap, keys[i], true, default_bits, &tb);
    out_key[i] = keys[i];
    out_val[i] = vals[i];
    out_t[i] = tb;
    out_ts[i] = ts[i];
  }
}

}  // namespace cpu
}  // namespace mxs
