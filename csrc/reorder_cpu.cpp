// mxstream — C++ twins of the reorder-buffer kernels (csrc/reorder_hip.hip; design:
// csrc/mxs_reorder.h). Plain loops: they define the result the kernels are compared against array
// for array, the total order (ts, arrival) included.
#include <stdexcept>

#include "mxs_reorder.h"

namespace mxs {
namespace cpu {

void reorder_cut(const int64_t* ts, int64_t n_arena, const int64_t* begin, const int64_t* end,
                 int64_t k, int64_t w, int64_t* cut) {
  for (int64_t c = 0; c < k; ++c) {
    if (begin[c] < 0 || end[c] < begin[c] || end[c] > n_arena)
      throw std::invalid_argument("reorder_cut: a chunk outside the arena");
    int64_t p = begin[c];
    while (p < end[c] && ts[p] <= w) ++p;
    cut[c] = p;
  }
}

void reorder_collect(const int64_t* ts, int64_t n_arena, const int64_t* begin, const int64_t* dest,
                     int64_t k, int64_t total, int64_t lo, int64_t* out_key, int64_t* out_src) {
  if (k <= 0 || total <= 0) return;
  if (dest[0] != 0 || dest[k] != total)
    throw std::invalid_argument("reorder_collect: offsets do not cover the output");
  for (int64_t c = 0; c < k; ++c) {
    const int64_t len = dest[c + 1] - dest[c];
    if (len < 0 || begin[c] < 0 || begin[c] + len > n_arena)
      throw std::invalid_argument("reorder_collect: a chunk outside the arena");
    for (int64_t j = 0; j < len; ++j) {
      out_key[dest[c] + j] = ts[begin[c] + j] - lo;
      out_src[dest[c] + j] = begin[c] + j;
    }
  }
}

void reorder_gather(const int64_t* perm, int64_t m, const int64_t* src_key, const int64_t* src_ts,
                    const int64_t* src_bits, int64_t n_src, int64_t* dst_key, int64_t* dst_ts,
                    int64_t* dst_bits) {
  for (int64_t i = 0; i < m; ++i)
    if (perm[i] < 0 || perm[i] >= n_src)
      throw std::invalid_argument("reorder_gather: an index outside the source");
  for (int64_t i = 0; i < m; ++i) {
    const int64_t p = perm[i];
    dst_key[i] = src_key[p];
    dst_ts[i] = src_ts[p];
    dst_bits[i] = src_bits[p];
  }
}

}  // namespace cpu
}  // namespace mxs
