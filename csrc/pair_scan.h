// mxstream — "scan the counts and compact the non-empty rows", the three passes that the window
// join (csrc/join_hip.hip), the interval join (csrc/ijoin_hip.hip) and the list windows' key scan
// (csrc/listwin_hip.hip) share. Device code and its launch: include from a .hip file.
//
// n elements have a 64-bit count each. The passes give every element its exclusive offset and
// every element with a count its rank among those, in element order, without atomics: tiles of
// kJoinScanTile elements are summed (pass 1), one workgroup scans the tile totals (pass 2), and
// every tile scans its elements again from its tile's offset (pass 3). What a count is and what
// is written is the caller's, a policy object passed by value to the kernels:
//   typename P::Add             the add of two counts: SatAdd or Add64
//   uint64_t count(i)           element i's count, already clamped or widened
//   void element(i, o)          pass 3, every element: its exclusive offset o
//   void nonempty(i, h, o)      pass 3, every element with a count: its rank h and its offset o
//   void finish(total, m)       pass 2, thread 0: the sum of all counts and how many are not 0
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mxs_blockscan.h"
#include "mxs_hip_util.h"
#include "mxs_join.h"

namespace mxs {

constexpr int kPairScanThreads = 1024;
constexpr int kPairScanPer = kJoinScanTile / kPairScanThreads;  // 4 elements per thread

// The joins' add: pair totals saturate at kJoinMaxPairs.
struct SatAdd {
  __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const {
    return join_sat_add(a, b);
  }
};

// Pass 1: per tile, the total and the number of non-empty elements.
template <class P>
__global__ __launch_bounds__(kPairScanThreads) void pair_tile_sums_kernel(
    P p, int64_t n, uint64_t* __restrict__ tsum, uint32_t* __restrict__ tne) {
  __shared__ uint64_t ws[16];
  __shared__ uint32_t wn[16];
  __shared__ uint64_t tot;
  __shared__ uint32_t totn;
  const typename P::Add add{};
  const int64_t k0 = (int64_t)blockIdx.x * kJoinScanTile + (int64_t)threadIdx.x * kPairScanPer;
  uint64_t s = 0;
  uint32_t ne = 0;
#pragma unroll
  for (int j = 0; j < kPairScanPer; ++j) {
    const uint64_t c = k0 + j < n ? p.count(k0 + j) : 0ull;
    s = add(s, c);
    ne += c ? 1u : 0u;
  }
  block_excl_scan<uint64_t>(s, ws, &tot, add);
  block_excl_scan<uint32_t>(ne, wn, &totn, Add32());
  if (threadIdx.x == 0) {
    tsum[blockIdx.x] = tot;
    tne[blockIdx.x] = totn;
  }
}

// Pass 2 (one workgroup): exclusive scan of the tile totals, kPairScanThreads tiles per round
// with a carry, so any number of tiles; then the policy's epilogue.
template <class P>
__global__ __launch_bounds__(kPairScanThreads) void pair_tile_scan_kernel(
    P p, uint64_t* __restrict__ tsum, uint32_t* __restrict__ tne, int64_t ntiles) {
  __shared__ uint64_t ws[16];
  __shared__ uint32_t wn[16];
  __shared__ uint64_t tot;
  __shared__ uint32_t totn;
  const typename P::Add add{};
  uint64_t carry = 0;
  uint32_t carry_n = 0;
  for (int64_t base = 0; base < ntiles; base += kPairScanThreads) {
    const int64_t t = base + threadIdx.x;
    const uint64_t s = t < ntiles ? tsum[t] : 0ull;
    const uint32_t e = t < ntiles ? tne[t] : 0u;
    const uint64_t bs = block_excl_scan<uint64_t>(s, ws, &tot, add);
    const uint32_t be = block_excl_scan<uint32_t>(e, wn, &totn, Add32());
    if (t < ntiles) {
      tsum[t] = add(carry, bs);
      tne[t] = carry_n + be;
    }
    carry = add(carry, tot);
    carry_n += totn;
    __syncthreads();  // tot / totn are rewritten by the next round
  }
  if (threadIdx.x == 0) p.finish(carry, carry_n);
}

// Pass 3: per tile, every element's exclusive offset and the rows of the non-empty ones, in
// element order.
template <class P>
__global__ __launch_bounds__(kPairScanThreads) void pair_tile_write_kernel(
    P p, int64_t n, const uint64_t* __restrict__ tsum, const uint32_t* __restrict__ tne) {
  __shared__ uint64_t ws[16];
  __shared__ uint32_t wn[16];
  __shared__ uint64_t tot;
  __shared__ uint32_t totn;
  const typename P::Add add{};
  const int64_t k0 = (int64_t)blockIdx.x * kJoinScanTile + (int64_t)threadIdx.x * kPairScanPer;
  uint64_t c[kPairScanPer];
  uint64_t s = 0;
  uint32_t ne = 0;
#pragma unroll
  for (int j = 0; j < kPairScanPer; ++j) {
    c[j] = k0 + j < n ? p.count(k0 + j) : 0ull;
    s = add(s, c[j]);
    ne += c[j] ? 1u : 0u;
  }
  uint64_t o = add(tsum[blockIdx.x], block_excl_scan<uint64_t>(s, ws, &tot, add));
  int64_t h = (int64_t)tne[blockIdx.x] + block_excl_scan<uint32_t>(ne, wn, &totn, Add32());
#pragma unroll
  for (int j = 0; j < kPairScanPer; ++j) {
    const int64_t i = k0 + j;
    if (i < n) {
      p.element(i, o);
      if (c[j]) {
        p.nonempty(i, h, o);
        ++h;
      }
    }
    o = add(o, c[j]);
  }
}

// Scratch for n elements: per tile a 64-bit total and a 32-bit non-empty count.
inline int64_t pair_scan_scratch_bytes(int64_t n) {
  const int64_t nt = (n + kJoinScanTile - 1) / kJoinScanTile;
  return nt * (int64_t)(sizeof(uint64_t) + sizeof(uint32_t)) + 64;
}

// The three passes over n >= 0 elements (the caller has checked that the tiles fit a grid).
// With no element only pass 2 runs, for the policy's epilogue.
template <class P>
void pair_scan_launch(const P& p, int64_t n, void* scratch, hipStream_t s) {
  const int64_t nt = (n + kJoinScanTile - 1) / kJoinScanTile;
  uint64_t* tsum = reinterpret_cast<uint64_t*>(scratch);
  uint32_t* tne = reinterpret_cast<uint32_t*>(tsum + nt);
  const dim3 grid((unsigned)nt), block(kPairScanThreads);
  if (nt) hipLaunchKernelGGL(pair_tile_sums_kernel<P>, grid, block, 0, s, p, n, tsum, tne);
  hipLaunchKernelGGL(pair_tile_scan_kernel<P>, dim3(1), block, 0, s, p, tsum, tne, nt);
  if (nt) hipLaunchKernelGGL(pair_tile_write_kernel<P>, grid, block, 0, s, p, n, tsum, tne);
  MXS_HIP_CHECK(hipGetLastError());
}

}  // namespace mxs
