// mxstream — the event-time reorder buffer on gfx950: cut the chunks at a watermark, collect the
// released prefixes as (ts - lo, arena index) pairs, gather rows by index (declarations and the
// design: csrc/mxs_reorder.h; C++ twins: csrc/reorder_cpu.cpp).
//
// The collect is output-centric like ijoin_expand_kernel (csrc/ijoin_hip.hip): a workgroup owns
// kReorderTile consecutive output positions whatever chunk they come from, keeps the k + 1
// destination offsets in LDS and finds a position's chunk by a binary search there. Inside a chunk
// the rows are consecutive, so the loads of `ts` are coalesced up to the chunk ends. No atomics
// but the error flag, no device counter.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "mxs_reorder.h"
#include "rule_scan.h"

namespace mxs {
namespace {

constexpr int kReorderBlock = 256;

// ---- cut -----------------------------------------------------------------------------------
// One lane per chunk. A chunk whose bounds do not lie in the arena is cut at its begin.
__global__ __launch_bounds__(kReorderBlock) void reorder_cut_kernel(
    const int64_t* __restrict__ ts, int64_t n_arena, const int64_t* __restrict__ begin,
    const int64_t* __restrict__ end, int64_t k, int64_t w, int64_t* __restrict__ cut) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= k) return;
  const int64_t b = begin[c], e = end[c];
  cut[c] = (b < 0 || e < b || e > n_arena) ? b : reorder_upper_bound(ts, b, e, w);
}

// ---- collect -------------------------------------------------------------------------------
__global__ __launch_bounds__(kReorderBlock) void reorder_collect_kernel(
    const int64_t* __restrict__ ts, int64_t n_arena, const int64_t* __restrict__ begin,
    const int64_t* __restrict__ dest, int32_t k, int64_t total, int64_t lo, int64_t ntiles,
    int64_t* __restrict__ out_key, int64_t* __restrict__ out_src, uint32_t* __restrict__ err) {
  // sdest[c]: the first output position of chunk c; sdest[k] = total
  __shared__ int64_t sdest[kReorderMaxChunks + 1];
  for (int32_t c = threadIdx.x; c <= k; c += kReorderBlock) sdest[c] = dest[c];
  __syncthreads();
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t tb = tile * kReorderTile;
    const int64_t te = tb + kReorderTile < total ? tb + kReorderTile : total;
    int32_t c = -1;     // the lane's chunk and the first position of the next one
    int64_t nxt = tb;
    for (int64_t p = tb + threadIdx.x; p < te; p += kReorderBlock) {
      if (p >= nxt) {
        // the last chunk c' > c with sdest[c'] <= p (sdest[0] = 0 <= p < total = sdest[k]): of
        // several chunks that start at one position all but the last are empty
        int32_t l = c < 0 ? 0 : c, h = k;
        while (h - l > 1) {
          const int32_t mid = (l + h) >> 1;
          if (sdest[mid] <= p) l = mid; else h = mid;
        }
        c = l;
        nxt = sdest[c + 1];
      }
      const int64_t src = begin[c] + (p - sdest[c]);
      if (src < 0 || src >= n_arena || p >= nxt) {
        atomicOr(err, 1u);
        out_key[p] = 0;
        out_src[p] = 0;
      } else {
        out_key[p] = ts[src] - lo;
        out_src[p] = src;
      }
    }
  }
}

// ---- gather --------------------------------------------------------------------------------
__global__ __launch_bounds__(kReorderBlock) void reorder_gather_kernel(
    const int64_t* __restrict__ perm, int64_t m, const int64_t* __restrict__ src_key,
    const int64_t* __restrict__ src_ts, const int64_t* __restrict__ src_bits, int64_t n_src,
    int64_t* __restrict__ dst_key, int64_t* __restrict__ dst_ts, int64_t* __restrict__ dst_bits,
    uint32_t* __restrict__ err) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = perm[i];
    if (p < 0 || p >= n_src) {
      atomicOr(err, 1u);
      continue;
    }
    dst_key[i] = src_key[p];
    dst_ts[i] = src_ts[p];
    dst_bits[i] = src_bits[p];
  }
}

}  // namespace

namespace gpu {

void reorder_cut(const int64_t* ts, int64_t n_arena, const int64_t* begin, const int64_t* end,
                 int64_t k, int64_t w, int64_t* cut, intptr_t stream) {
  if (k <= 0) return;
  if (k > kReorderMaxChunks) throw std::invalid_argument("reorder_cut: too many chunks");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(reorder_cut_kernel, dim3(grid_of(k, kReorderBlock, 1 << 16)),
                     dim3(kReorderBlock), 0, s, ts, n_arena, begin, end, k, w, cut);
  MXS_HIP_CHECK(hipGetLastError());
}

void reorder_collect(const int64_t* ts, int64_t n_arena, const int64_t* begin, const int64_t* dest,
                     int64_t k, int64_t total, int64_t lo, int64_t* out_key, int64_t* out_src,
                     uint32_t* err, intptr_t stream) {
  if (k <= 0 || total <= 0) return;
  if (k > kReorderMaxChunks) throw std::invalid_argument("reorder_collect: too many chunks");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t ntiles = (total + kReorderTile - 1) / kReorderTile;
  hipLaunchKernelGGL(reorder_collect_kernel, dim3(grid_of(ntiles, 1, 1 << 16)),
                     dim3(kReorderBlock), 0, s, ts, n_arena, begin, dest, (int32_t)k, total, lo,
                     ntiles, out_key, out_src, err);
  MXS_HIP_CHECK(hipGetLastError());
}

void reorder_gather(const int64_t* perm, int64_t m, const int64_t* src_key, const int64_t* src_ts,
                    const int64_t* src_bits, int64_t n_src, int64_t* dst_key, int64_t* dst_ts,
                    int64_t* dst_bits, uint32_t* err, intptr_t stream) {
  if (m <= 0) return;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(reorder_gather_kernel, dim3(grid_of(m, kReorderBlock, 1 << 16)),
                     dim3(kReorderBlock), 0, s, perm, m, src_key, src_ts, src_bits, n_src, dst_key,
                     dst_ts, dst_bits, err);
  MXS_HIP_CHECK(hipGetLastError());
}

}  // namespace gpu
}  // namespace mxs
