// mxstream — the block-wide exclusive scan and the plain add operators for every unit that scans
// inside a workgroup (csrc/pair_scan.h, csrc/lookup_hip.hip). Device code only: include from a
// .hip file.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mxs {

struct Add32 {
  __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; }
};
struct Add64 {
  __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const { return a + b; }
};

// Block-wide exclusive scan of one value per thread (up to 1024 threads) under an associative
// `op` with identity 0: wave shuffles + wave totals. `wsum` holds one word per wave.
template <class T, class Op>
__device__ __forceinline__ T block_excl_scan(T v, T* wsum, T* total, Op op) {
  T incl = v;
  for (int d = 1; d < 64; d <<= 1) {
    const T y = __shfl_up(incl, d);
    if ((int)(threadIdx.x & 63) >= d) incl = op(y, incl);
  }
  T excl = __shfl_up(incl, 1);
  if ((threadIdx.x & 63) == 0) excl = 0;
  const int wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 63) wsum[wv] = incl;
  __syncthreads();
  if (threadIdx.x == 0) {
    T t = 0;
    for (int i = 0; i < nw; ++i) {
      const T c = wsum[i];
      wsum[i] = t;
      t = op(t, c);
    }
    *total = t;
  }
  __syncthreads();
  const T r = op(wsum[wv], excl);
  __syncthreads();
  return r;
}

}  // namespace mxs
