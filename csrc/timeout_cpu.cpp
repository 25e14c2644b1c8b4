// mxstream — C++ twins of the keyed timer kernels (csrc/timeout_hip.hip; design:
// csrc/mxs_timeout.h). Plain loops: they define the result the kernels are compared against array
// for array.
#include <stdexcept>

#include "mxs_timeout.h"

namespace mxs {
namespace cpu {

void timeout_update(const int64_t* keys, const int64_t* ts, int64_t n, int64_t timeout,
                    int64_t* state, int64_t* deadline, int64_t* tile_min, int64_t cap) {
  if (timeout <= 0) throw std::invalid_argument("timeout_update: timeout must be positive");
  for (int64_t i = 0; i < n; ++i) {
    const int64_t k = keys[i];
    if (k < 0 || k >= cap) throw std::invalid_argument("timeout_update: key outside the table");
    if (ts[i] >= kTimeoutNone - timeout)
      throw std::invalid_argument("timeout_update: timestamp + timeout overflows");
  }
  for (int64_t i = 0; i < n; ++i) {  // arrival order: a later row of a key overwrites `last`
    const int64_t k = keys[i];
    state[2 * k] += 1;
    state[2 * k + 1] = ts[i];
    deadline[k] = ts[i] + timeout;
  }
  for (int64_t i = 0; i < n; ++i) {  // the bound moves to every key's new deadline only
    const int64_t k = keys[i], t = k / kTimeoutTile;
    if (deadline[k] < tile_min[t]) tile_min[t] = deadline[k];
  }
}

void timeout_mask(const int64_t* deadline, int64_t cap, int64_t w, int64_t* tile_min,
                  uint64_t* words, uint32_t* counts) {
  const bool skip = timeout_tileskip();
  const int64_t ntiles = timeout_tiles(cap);
  for (int64_t t = 0; t < ntiles; ++t) {
    if (skip && tile_min[t] > w) {
      counts[t] = 0;
      continue;
    }
    uint32_t c = 0;
    int64_t left = kTimeoutNone;
    for (int j = 0; j < kTimeoutWords; ++j) {
      uint64_t word = 0;
      for (int b = 0; b < 64; ++b) {
        const int64_t k = t * kTimeoutTile + j * 64 + b;
        if (k >= cap) break;
        if (timeout_due(deadline[k], w)) {
          word |= 1ull << b;
          ++c;
        } else if (deadline[k] < left) {
          left = deadline[k];
        }
      }
      words[t * kTimeoutWords + j] = word;
    }
    counts[t] = c;
    tile_min[t] = left;
  }
}

void timeout_emit(const int64_t* state, int64_t* deadline, int64_t cap, const uint64_t* words,
                  const uint32_t* counts, int64_t total, int64_t* out_key, int64_t* out_count,
                  int64_t* out_last, int64_t* out_deadline) {
  const int64_t ntiles = timeout_tiles(cap);
  int64_t o = 0;
  for (int64_t t = 0; t < ntiles; ++t) {
    if (counts[t] == 0) continue;
    for (int64_t k = t * kTimeoutTile; k < cap && k < (t + 1) * kTimeoutTile; ++k) {
      if (!((words[k >> 6] >> (k & 63)) & 1ull)) continue;
      if (o >= total) throw std::invalid_argument("timeout_emit: more due keys than counted");
      out_key[o] = k;
      out_count[o] = state[2 * k];
      out_last[o] = state[2 * k + 1];
      out_deadline[o] = deadline[k];
      deadline[k] = kTimeoutNone;
      ++o;
    }
  }
  if (o != total) throw std::invalid_argument("timeout_emit: fewer due keys than counted");
}

}  // namespace cpu
}  // namespace mxs
