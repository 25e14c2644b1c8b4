// mxstream — the event-time reorder buffer in front of the keyed rules
// (``stream.key_by(k).process(EventTimeOrdered(rule))``): rows are held until the watermark
// reaches them and leave in (timestamp, arrival) order; a row at or behind the watermark on
// arrival is late and dropped.
//
// State: one linear arena of 24-byte rows as three int64 columns (key id, ts, value bits), SoA:
// the rule wants three contiguous columns and the cut reads only `ts`. A pushed batch becomes one
// *chunk*, a run sorted by (ts, arrival) appended at the arena's tail; the host keeps
// (offset, head, n) per chunk. A watermark W releases, from every chunk, the prefix with
// ts <= W -- the chunk's head moves, no retained row does. The released prefixes of several
// chunks are merged by one stable radix sort of (ts - lo, arena index) pairs collected in chunk
// order, so equal timestamps stay in arrival order. Retained rows move only when the arena is
// consolidated into one chunk (too many chunks, a full arena, a restore).
//
// Three kernels (csrc/reorder_hip.hip), each with a plain-loop twin (csrc/reorder_cpu.cpp) that
// defines the result:
//   reorder_cut      one lane per chunk: the upper bound of W in ts[begin, end) -> cut
//   reorder_collect  output-centric: position p of the release belongs to the chunk c with
//                    dest[c] <= p < dest[c + 1]; src = begin[c] + p - dest[c]; writes the sort
//                    key ts[src] - lo and the value src
//   reorder_gather   dst column[i] = src column[perm[i]] for the three columns
// Timestamps lie strictly inside (-2**62, 2**62), which the callers check, so ts - lo cannot
// overflow. Every index is guarded: a perm or src outside its column writes nothing / reads
// nothing and raises the error flag.
#pragma once
#include <cstdint>

#include "mxs_common.h"

namespace mxs {

constexpr int kReorderTile = 4096;       // output positions a workgroup of the collect owns
constexpr int kReorderMaxChunks = 1024;  // chunks one cut / collect takes (LDS: 8 KiB of offsets)

// The upper bound of w in the ascending ts[b, e): the first position whose ts > w.
MXS_HD int64_t reorder_upper_bound(const int64_t* ts, int64_t b, int64_t e, int64_t w) {
  while (b < e) {
    const int64_t mid = b + ((e - b) >> 1);
    if (ts[mid] <= w) b = mid + 1; else e = mid;
  }
  return b;
}

namespace gpu {
// begin / end / cut: k words each, 0 <= begin <= end <= n_arena (checked by the caller).
void reorder_cut(const int64_t* ts, int64_t n_arena, const int64_t* begin, const int64_t* end,
                 int64_t k, int64_t w, int64_t* cut, intptr_t stream);
// begin: k words; dest: k + 1 words, dest[0] = 0, non-decreasing, dest[k] = total;
// out_key / out_src: total words; err: one uint32 the caller zeroed, set on a guarded index.
void reorder_collect(const int64_t* ts, int64_t n_arena, const int64_t* begin, const int64_t* dest,
                     int64_t k, int64_t total, int64_t lo, int64_t* out_key, int64_t* out_src,
                     uint32_t* err, intptr_t stream);
// src columns hold n_src words, dst columns m; perm: m words in [0, n_src).
void reorder_gather(const int64_t* perm, int64_t m, const int64_t* src_key, const int64_t* src_ts,
                    const int64_t* src_bits, int64_t n_src, int64_t* dst_key, int64_t* dst_ts,
                    int64_t* dst_bits, uint32_t* err, intptr_t stream);
}  // namespace gpu

namespace cpu {
void reorder_cut(const int64_t* ts, int64_t n_arena, const int64_t* begin, const int64_t* end,
                 int64_t k, int64_t w, int64_t* cut);
void reorder_collect(const int64_t* ts, int64_t n_arena, const int64_t* begin, const int64_t* dest,
                     int64_t k, int64_t total, int64_t lo, int64_t* out_key, int64_t* out_src);
void reorder_gather(const int64_t* perm, int64_t m, const int64_t* src_key, const int64_t* src_ts,
                    const int64_t* src_bits, int64_t n_src, int64_t* dst_key, int64_t* dst_ts,
                    int64_t* dst_bits);
}  // namespace cpu

}  // namespace mxs
