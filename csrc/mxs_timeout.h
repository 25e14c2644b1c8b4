// mxstream — keyed event-time timers (``stream.key_by(k).process(CountWithTimeout(timeout))``):
// every key counts its elements and remembers the timestamp of the last one; once the watermark
// passes ``last + timeout`` the key emits (key, count, last).
//
// The per-record operator registers one timer per element and lets every timer but the one at
// ``last + timeout`` find a newer `last`. The batch model keeps that one timer only: a key is
// *armed* with deadline = last + timeout by every element (again after it fired, also when the
// deadline already lies at or below the watermark) and disarmed by its firing.
//
// State, for dense key ids k in [0, cap):
//   state    int64[cap, 2]   row k = (count, last); 16-byte rows, zero = never seen
//   deadline int64[cap]      last + timeout while armed, else kTimeoutNone (INT64_MAX)
//   tile_min int64[ceil(cap / kTimeoutTile)]   tile_min[t] <= min(deadline[k] for k in tile t):
//            a lower bound that update lowers and a firing that scans the tile makes exact.
//
// The end-of-input watermark is INT64_MAX, the sentinel's value: armed is
// ``deadline != kTimeoutNone && deadline <= w`` (timeout_due). A batch with
// max(ts) + timeout >= INT64_MAX is refused by the callers.
//
// Kernels (csrc/timeout_hip.hip) and their C++ twins (csrc/timeout_cpu.cpp):
//   timeout_update  a batch in arrival order: count += the key's rows, last = the timestamp of
//                   the key's last row, deadline = last + timeout, tile_min lowered with the
//                   key's new deadline. The device takes the batch stably sorted by key with
//                   `perm` = the arrival index of every sorted row; only the row that ends its
//                   key's run writes. The twin is the plain loop in arrival order.
//   timeout_mask    tile t = key ids [t * kTimeoutTile, + kTimeoutTile). A tile whose tile_min
//                   lies above w is skipped: counts[t] = 0, its words are not written
//                   (MXS_TIMEOUT_TILESKIP=0 scans every tile). A scanned tile writes
//                   words[t * 64 + j], bit b = key id t * kTimeoutTile + 64 j + b is due
//                   (ids >= cap are never due), counts[t] = its due keys, and tile_min[t] = the
//                   exact minimum of the deadlines that stay armed.
//   lookup_scan     (csrc/mxs_lookup.h) offsets = the exclusive scan of counts, meta[0] = total
//   timeout_emit    the due keys in key order as four columns (key id, count, last, deadline),
//                   row at offsets[tile] + popcount of the tile's earlier bits; every emitted
//                   key's deadline becomes kTimeoutNone.
#pragma once
#include <cstdint>
#include <cstdlib>

#include "mxs_common.h"

namespace mxs {

constexpr int kTimeoutTile = 4096;
constexpr int kTimeoutWords = kTimeoutTile / 64;  // mask words of a tile
constexpr int64_t kTimeoutNone = INT64_MAX;       // deadline of a key that is not armed

MXS_HD bool timeout_due(int64_t deadline, int64_t w) {
  return deadline != kTimeoutNone && deadline <= w;
}

MXS_HD int64_t timeout_tiles(int64_t cap) { return (cap + kTimeoutTile - 1) / kTimeoutTile; }

// MXS_TIMEOUT_TILESKIP (default 1), read per call: a process can run both sides of the A/B.
inline bool timeout_tileskip() {
  const char* e = std::getenv("MXS_TIMEOUT_TILESKIP");
  return !(e && e[0] == '0' && e[1] == '\0');
}

namespace gpu {
void timeout_update(const int64_t* skeys, const int64_t* perm, const int64_t* ts, int64_t n,
                    int64_t timeout, int64_t* state, int64_t* deadline, int64_t* tile_min,
                    int64_t cap, intptr_t stream);
void timeout_mask(const int64_t* deadline, int64_t cap, int64_t w, int64_t* tile_min,
                  uint64_t* words, uint32_t* counts, intptr_t stream);
void timeout_emit(const int64_t* state, int64_t* deadline, int64_t cap, const uint64_t* words,
                  const uint32_t* counts, const int64_t* offsets, int64_t total, int64_t* out_key,
                  int64_t* out_count, int64_t* out_last, int64_t* out_deadline, intptr_t stream);
}  // namespace gpu

namespace cpu {
void timeout_update(const int64_t* keys, const int64_t* ts, int64_t n, int64_t timeout,
                    int64_t* state, int64_t* deadline, int64_t* tile_min, int64_t cap);
void timeout_mask(const int64_t* deadline, int64_t cap, int64_t w, int64_t* tile_min,
                  uint64_t* words, uint32_t* counts);
void timeout_emit(const int64_t* state, int64_t* deadline, int64_t cap, const uint64_t* words,
                  const uint32_t* counts, int64_t total, int64_t* out_key, int64_t* out_count,
                  int64_t* out_last, int64_t* out_deadline);
}  // namespace cpu

}  // namespace mxs
