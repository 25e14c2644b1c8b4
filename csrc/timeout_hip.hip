// mxstream — keyed event-time timers on gfx950: count and last-seen per key, one armed deadline
// per key, and a firing that reads only the key tiles whose earliest deadline the watermark has
// reached (declarations, layouts and the model: csrc/mxs_timeout.h; C++ twins:
// csrc/timeout_cpu.cpp).
//
// update: the batch arrives stably sorted by key; the row that ends its key's run finds the run's
// start by a galloping binary search over the sorted keys and is the key's only writer, so the
// state needs no atomics. Only tile_min is shared between keys: a wave reduces its rows' new
// deadlines per tile (rows of a tile are neighbours in the sorted batch) and issues at most one
// 64-bit atomicMin per tile, and none when a plain load already shows a bound at or below it.
// mask / emit: the order-preserving compaction of the lookup (ballot words, tile counts, one
// scan workgroup, popcount offsets) over key ids instead of rows; a workgroup of 256 threads owns
// a tile of 4096 key ids and reads their deadlines with 16-byte loads.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "mxs_timeout.h"
#include "rule_scan.h"

namespace mxs {
namespace {

constexpr int kTimeoutBlock = 256;
constexpr int kTimeoutWaves = kTimeoutBlock / 64;
constexpr int kMaskRounds = kTimeoutTile / (2 * kTimeoutBlock);  // 16-byte loads per lane and tile
constexpr int kEmitRounds = kTimeoutTile / kTimeoutBlock;        // key ids per lane and tile
constexpr int kTimeoutMaxGrid = 1 << 20;  // larger tables stride over their tiles
constexpr int kTimeoutTileLog2 = 12;
static_assert((1 << kTimeoutTileLog2) == kTimeoutTile, "tile size");

__device__ __forceinline__ int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

// ---- update --------------------------------------------------------------------------------
// First index of key k in skeys[0, i] (skeys[i] == k): gallop back from i, then bisect.
__device__ __forceinline__ int64_t run_start(const int64_t* __restrict__ skeys, int64_t i,
                                             int64_t k) {
  int64_t hi = i, step = 1;  // skeys[hi] == k throughout
  int64_t lo = -1;           // skeys[lo] != k, or -1
  while (true) {
    const int64_t p = hi - step;
    if (p < 0) break;
    if (skeys[p] != k) {
      lo = p;
      break;
    }
    hi = p;
    step <<= 1;
  }
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (skeys[mid] == k) hi = mid; else lo = mid;
  }
  return hi;
}

__global__ __launch_bounds__(kTimeoutBlock) void timeout_update_kernel(
    const int64_t* __restrict__ skeys, const int64_t* __restrict__ perm,
    const int64_t* __restrict__ ts, int64_t n, int64_t timeout, ll2* __restrict__ state,
    int64_t* __restrict__ deadline, int64_t* __restrict__ tile_min, int64_t cap) {
  const int lane = threadIdx.x & 63;
  // `base` is the same for a wave's 64 lanes: they leave the loop together (shuffles below).
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < n;
       base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = base + lane;
    int64_t tile = INT64_MAX;     // rows past the batch: a tile of their own, nothing to lower
    int64_t mine = kTimeoutNone;  // the deadline this row stored
    if (i < n) {
      const int64_t k = skeys[i];
      tile = k >> kTimeoutTileLog2;
      const bool tail = i + 1 == n || skeys[i + 1] != k;
      if (tail && (uint64_t)k < (uint64_t)cap) {
        const int64_t src = perm[i];
        if ((uint64_t)src < (uint64_t)n) {
          const int64_t last = ts[src];
          ll2 row = state[k];
          row.x += i - run_start(skeys, i, k) + 1;
          row.y = last;
          state[k] = row;
          mine = last + timeout;
          deadline[k] = mine;
        }
      }
    }
    // Minimum over the lanes at and after this one that share its tile (sorted: one segment).
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t od = __shfl_down(mine, d);
      const int64_t ot = __shfl_down(tile, d);
      if (lane + d < 64 && ot == tile) mine = min64(mine, od);
    }
    const int64_t pt = __shfl_up(tile, 1);
    const bool head = lane == 0 || pt != tile;
    if (head && mine != kTimeoutNone) {
      // tile_min only falls while this kernel runs: a stale value is never below the true one,
      // so the plain load can ask for a needless atomic but cannot skip a needed one.
      if (mine < tile_min[tile]) atomicMin((long long*)&tile_min[tile], (long long)mine);
    }
  }
}

// ---- mask ----------------------------------------------------------------------------------
// Bits 0..31 of x moved to the even bit positions 0, 2, .., 62.
__device__ __forceinline__ uint64_t spread32(uint64_t x) {
  x &= 0xffffffffull;
  x = (x | (x << 16)) & 0x0000ffff0000ffffull;
  x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
  x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
  x = (x | (x << 2)) & 0x3333333333333333ull;
  x = (x | (x << 1)) & 0x5555555555555555ull;
  return x;
}

// Round r of a tile: wave v holds key ids [128 (4 r + v), + 128), lane l the ids 2 l and 2 l + 1
// of them = mask words 2 (4 r + v) and 2 (4 r + v) + 1.
template <bool kSkip>
__global__ __launch_bounds__(kTimeoutBlock) void timeout_mask_kernel(
    const int64_t* __restrict__ deadline, int64_t cap, int64_t w, int64_t ntiles,
    int64_t* __restrict__ tile_min, uint64_t* __restrict__ words, uint32_t* __restrict__ counts) {
  __shared__ uint32_t wcount[kTimeoutWaves];
  __shared__ int64_t wleft[kTimeoutWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    if (kSkip && tile_min[tile] > w) {  // uniform over the workgroup
      if (threadIdx.x == 0) counts[tile] = 0;
      continue;
    }
    ll2 d[kMaskRounds];
#pragma unroll
    for (int r = 0; r < kMaskRounds; ++r) {
      const int64_t k = tile * kTimeoutTile + (int64_t)(r * kTimeoutWaves + wave) * 128 + 2 * lane;
      d[r].x = kTimeoutNone, d[r].y = kTimeoutNone;
      if (k + 1 < cap)
        d[r] = *reinterpret_cast<const ll2*>(deadline + k);  // k is even: 16-byte aligned
      else if (k < cap)
        d[r].x = deadline[k];
    }
    uint32_t due = 0;
    int64_t left = kTimeoutNone;  // earliest deadline that stays armed
#pragma unroll
    for (int r = 0; r < kMaskRounds; ++r) {
      const bool fx = timeout_due(d[r].x, w), fy = timeout_due(d[r].y, w);
      const uint64_t even = __ballot(fx), odd = __ballot(fy);
      if (!fx) left = min64(left, d[r].x);
      if (!fy) left = min64(left, d[r].y);
      const uint64_t w0 = spread32(even) | (spread32(odd) << 1);
      const uint64_t w1 = spread32(even >> 32) | (spread32(odd >> 32) << 1);
      if (lane == 0) {
        uint64_t* out = words + tile * kTimeoutWords + 2 * (r * kTimeoutWaves + wave);
        out[0] = w0;
        out[1] = w1;
      }
      due += (uint32_t)(__popcll(even) + __popcll(odd));
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) left = min64(left, __shfl_down(left, s));
    if (lane == 0) {
      wcount[wave] = due;
      wleft[wave] = left;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t c = 0;
      int64_t m = kTimeoutNone;
      for (int v = 0; v < kTimeoutWaves; ++v) {
        c += wcount[v];
        m = min64(m, wleft[v]);
      }
      counts[tile] = c;
      tile_min[tile] = m;
    }
    __syncthreads();  // wcount / wleft are rewritten for the workgroup's next tile
  }
}

// ---- emit ----------------------------------------------------------------------------------
__global__ __launch_bounds__(kTimeoutBlock) void timeout_emit_kernel(
    const ll2* __restrict__ state, int64_t* __restrict__ deadline, int64_t cap, int64_t ntiles,
    const uint64_t* __restrict__ words, const uint32_t* __restrict__ counts,
    const int64_t* __restrict__ offsets, int64_t total, int64_t* __restrict__ out_key,
    int64_t* __restrict__ out_count, int64_t* __restrict__ out_last,
    int64_t* __restrict__ out_deadline) {
  __shared__ uint64_t tword[kTimeoutWords];
  __shared__ uint32_t tpre[kTimeoutWords];  // due keys of the tile's earlier words
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    if (counts[tile] == 0) continue;  // uniform over the workgroup; its words may be unwritten
    if (wave == 0) {
      const uint64_t w = words[tile * kTimeoutWords + lane];
      uint32_t incl = (uint32_t)__popcll(w);
      const uint32_t own = incl;
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(incl, d);
        if (lane >= d) incl += y;
      }
      tword[lane] = w;
      tpre[lane] = incl - own;
    }
    __syncthreads();
    const int64_t off = offsets[tile];
    const int64_t base = tile * kTimeoutTile + threadIdx.x;
#pragma unroll 4
    for (int r = 0; r < kEmitRounds; ++r) {
      const int j = r * kTimeoutWaves + wave;
      const uint64_t w = tword[j];
      if (w == 0) continue;  // uniform over the wave
      const int64_t k = base + (int64_t)r * kTimeoutBlock;
      if (!((w >> lane) & 1ull) || k >= cap) continue;
      const int64_t pos = off + tpre[j] + __popcll(w & ((1ull << lane) - 1ull));
      if (pos >= total) continue;
      const ll2 row = state[k];
      out_key[pos] = k;
      out_count[pos] = row.x;
      out_last[pos] = row.y;
      out_deadline[pos] = deadline[k];
      deadline[k] = kTimeoutNone;
    }
    __syncthreads();  // tword / tpre are refilled for the workgroup's next tile
  }
}

void check_tables(const int64_t* state, const int64_t* deadline, const int64_t* tile_min,
                  int64_t cap, const char* what) {
  if (cap < 1 || deadline == nullptr)
    throw std::invalid_argument(std::string(what) + ": bad table");
  if (((uintptr_t)state & 15u) || ((uintptr_t)deadline & 15u))
    throw std::invalid_argument(std::string(what) + ": the tables must be 16-byte aligned");
}

}  // namespace

namespace gpu {

void timeout_update(const int64_t* skeys, const int64_t* perm, const int64_t* ts, int64_t n,
                    int64_t timeout, int64_t* state, int64_t* deadline, int64_t* tile_min,
                    int64_t cap, intptr_t stream) {
  check_tables(state, deadline, tile_min, cap, "timeout_update");
  if (state == nullptr || tile_min == nullptr)
    throw std::invalid_argument("timeout_update: bad table");
  if (n < 0) throw std::invalid_argument("timeout_update: negative row count");
  if (timeout <= 0) throw std::invalid_argument("timeout_update: timeout must be positive");
  if (n == 0) return;
  hipLaunchKernelGGL(timeout_update_kernel, dim3(grid_of(n, kTimeoutBlock, 8192)),
                     dim3(kTimeoutBlock), 0, (hipStream_t)stream, skeys, perm, ts, n, timeout,
                     reinterpret_cast<ll2*>(state), deadline, tile_min, cap);
  MXS_HIP_CHECK(hipGetLastError());
}

void timeout_mask(const int64_t* deadline, int64_t cap, int64_t w, int64_t* tile_min,
                  uint64_t* words, uint32_t* counts, intptr_t stream) {
  check_tables(nullptr, deadline, tile_min, cap, "timeout_mask");
  if (tile_min == nullptr) throw std::invalid_argument("timeout_mask: bad table");
  const int64_t ntiles = timeout_tiles(cap);
  const dim3 grid(grid_of(ntiles, 1, kTimeoutMaxGrid));
  hipStream_t s = (hipStream_t)stream;
  if (timeout_tileskip())
    hipLaunchKernelGGL(timeout_mask_kernel<true>, grid, dim3(kTimeoutBlock), 0, s, deadline, cap,
                       w, ntiles, tile_min, words, counts);
  else
    hipLaunchKernelGGL(timeout_mask_kernel<false>, grid, dim3(kTimeoutBlock), 0, s, deadline, cap,
                       w, ntiles, tile_min, words, counts);
  MXS_HIP_CHECK(hipGetLastError());
}

// `words`, `counts` and `offsets` must be timeout_mask's and lookup_scan's output for these same
// tables and `total` the scan's total: a row past `total` is never written.
void timeout_emit(const int64_t* state, int64_t* deadline, int64_t cap, const uint64_t* words,
                  const uint32_t* counts, const int64_t* offsets, int64_t total, int64_t* out_key,
                  int64_t* out_count, int64_t* out_last, int64_t* out_deadline,
                  intptr_t stream) {
  check_tables(state, deadline, nullptr, cap, "timeout_emit");
  if (state == nullptr) throw std::invalid_argument("timeout_emit: bad table");
  if (total < 0 || total > cap) throw std::invalid_argument("timeout_emit: bad row count");
  if (total == 0) return;
  const int64_t ntiles = timeout_tiles(cap);
  hipLaunchKernelGGL(timeout_emit_kernel, dim3(grid_of(ntiles, 1, kTimeoutMaxGrid)),
                     dim3(kTimeoutBlock), 0, (hipStream_t)stream,
                     reinterpret_cast<const ll2*>(state), deadline, cap, ntiles, words, counts,
                     offsets, total, out_key, out_count, out_last, out_deadline);
  MXS_HIP_CHECK(hipGetLastError());
}

}  // namespace gpu
}  // namespace mxs
