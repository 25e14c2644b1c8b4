// mxstream — keyed latest-value lookup on gfx950: upsert the rule batches into a dense table,
// probe it with every sample and compact the samples that satisfy the comparison
// (declarations and layouts: csrc/mxs_lookup.h; C++ twins: csrc/lookup_cpu.cpp).
//
// The probe is the order-preserving compaction of the filters (ballot words per 64 rows, tile
// counts, one scan workgroup, popcount offsets) with a table gather in front of the predicate: a
// workgroup of 256 threads owns a tile of 4096 samples, 16 rows per lane, every row one 16-byte
// table load. The comparison and "has a default" are template arguments. No atomics, no
// workgroup waits for another, all offsets 64-bit.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "mxs_hip_util.h"
#include "mxs_lookup.h"
#include "mxs_blockscan.h"

namespace mxs {
namespace {

constexpr int kLookupBlock = 256;
constexpr int kLookupWaves = kLookupBlock / 64;
constexpr int kLookupRounds = kLookupTile / kLookupBlock;  // rows per lane of a tile
constexpr int kLookupBatch = 8;            // rounds whose loads are in flight together
constexpr int kLookupMaxGrid = 1 << 20;    // longer inputs stride over their tiles
constexpr int kScanThreads = 1024;

// The value in force for key k (one 16-byte load when k is inside the table).
template <bool kHasDefault>
__device__ __forceinline__ bool in_force(const ll2* __restrict__ table, int64_t cap, int64_t k,
                                         int64_t default_bits, int64_t* tbits) {
  if ((uint64_t)k < (uint64_t)cap) {
    const ll2 row = table[k];
    if (row.y != 0) {
      *tbits = row.x;
      return true;
    }
  }
  *tbits = default_bits;
  return kHasDefault;
}

// ---- upsert --------------------------------------------------------------------------------
// The batch sorted stably by key: the last row of a key's run is its last rule in arrival order.
__global__ __launch_bounds__(256) void lookup_upsert_kernel(
    const int64_t* __restrict__ skeys, const int64_t* __restrict__ perm,
    const int64_t* __restrict__ vals, int64_t n, ll2* __restrict__ table, int64_t cap) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = skeys[i];
    if (i + 1 < n && skeys[i + 1] == k) continue;
    const int64_t src = perm[i];
    if ((uint64_t)k >= (uint64_t)cap || (uint64_t)src >= (uint64_t)n) continue;
    ll2 row;
    row.x = vals[src];
    row.y = 1;
    table[k] = row;
  }
}

// ---- mask ----------------------------------------------------------------------------------
// Round r of a tile: wave w holds rows [256 r + 64 w, + 64) = mask word 4 r + w.
template <int kWhen, bool kHasDefault>
__global__ __launch_bounds__(kLookupBlock) void lookup_mask_kernel(
    const int64_t* __restrict__ keys, const int64_t* __restrict__ vals, int64_t n,
    const ll2* __restrict__ table, int64_t cap, int64_t default_bits, int64_t ntiles,
    uint64_t* __restrict__ words, uint32_t* __restrict__ counts) {
  __shared__ uint32_t wcount[kLookupWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t base = tile * kLookupTile + threadIdx.x;
    uint32_t kept = 0;
    // kLookupBatch rounds at a time: all their keys, then all their table rows, are in flight
    // before the first comparison (the table rows are random 16-byte gathers).
#pragma unroll
    for (int r0 = 0; r0 < kLookupRounds; r0 += kLookupBatch) {
      int64_t k[kLookupBatch], v[kLookupBatch];
      ll2 row[kLookupBatch];
#pragma unroll
      for (int j = 0; j < kLookupBatch; ++j) {
        const int64_t i = base + (int64_t)(r0 + j) * kLookupBlock;
        k[j] = i < n ? keys[i] : -1;  // -1: outside every table
        v[j] = i < n ? vals[i] : 0;
      }
#pragma unroll
      for (int j = 0; j < kLookupBatch; ++j) {
        row[j].x = 0, row[j].y = 0;
        if ((uint64_t)k[j] < (uint64_t)cap) row[j] = table[k[j]];
      }
#pragma unroll
      for (int j = 0; j < kLookupBatch; ++j) {
        const int64_t i = base + (int64_t)(r0 + j) * kLookupBlock;
        const bool present = row[j].y != 0;
        const bool keep = i < n && lookup_keep(kWhen, v[j], present || kHasDefault,
                                               present ? row[j].x : default_bits);
        const uint64_t word = __ballot(keep);
        if (lane == 0) words[tile * kLookupWords + (r0 + j) * kLookupWaves + wave] = word;
        kept += (uint32_t)__popcll(word);
      }
    }
    if (lane == 0) wcount[wave] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t c = 0;
      for (int w = 0; w < kLookupWaves; ++w) c += wcount[w];
      counts[tile] = c;
    }
    __syncthreads();  // wcount is rewritten for the workgroup's next tile
  }
}

// ---- scan (one workgroup: kScanThreads tiles per round with a carry) -------------------------
__global__ __launch_bounds__(kScanThreads) void lookup_scan_kernel(
    const uint32_t* __restrict__ counts, int64_t ntiles, int64_t* __restrict__ offsets,
    int64_t* __restrict__ meta) {
  __shared__ uint64_t ws[16];
  __shared__ uint64_t tot;
  uint64_t carry = 0;
  for (int64_t base = 0; base < ntiles; base += kScanThreads) {
    const int64_t t = base + threadIdx.x;
    const uint64_t c = t < ntiles ? (uint64_t)counts[t] : 0ull;
    const uint64_t ex = block_excl_scan<uint64_t>(c, ws, &tot, Add64());
    if (t < ntiles) offsets[t] = (int64_t)(carry + ex);
    carry += tot;
    __syncthreads();  // tot is rewritten by the next round
  }
  if (threadIdx.x == 0) {
    meta[0] = (int64_t)carry;
    meta[1] = 0;
  }
}

// ---- emit ----------------------------------------------------------------------------------
template <bool kHasDefault>
__global__ __launch_bounds__(kLookupBlock) void lookup_emit_kernel(
    const int64_t* __restrict__ keys, const int64_t* __restrict__ vals,
    const int64_t* __restrict__ ts, int64_t n, const ll2* __restrict__ table, int64_t cap,
    int64_t default_bits, int64_t ntiles, const uint64_t* __restrict__ words,
    const uint32_t* __restrict__ counts, const int64_t* __restrict__ offsets, int64_t kept,
    int64_t* __restrict__ out_key, int64_t* __restrict__ out_val, int64_t* __restrict__ out_t,
    int64_t* __restrict__ out_ts) {
  __shared__ uint64_t tword[kLookupWords];
  __shared__ uint32_t tpre[kLookupWords];  // kept rows of the tile's earlier words
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    if (counts[tile] == 0) continue;  // uniform over the workgroup
    if (wave == 0) {
      const uint64_t w = words[tile * kLookupWords + lane];
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
    const int64_t base = tile * kLookupTile + threadIdx.x;
#pragma unroll 4
    for (int r = 0; r < kLookupRounds; ++r) {
      const int j = r * kLookupWaves + wave;
      const uint64_t w = tword[j];
      if (w == 0) continue;  // uniform over the wave
      const int64_t i = base + (int64_t)r * kLookupBlock;
      if (!((w >> lane) & 1ull) || i >= n) continue;
      const int64_t pos = off + tpre[j] + __popcll(w & ((1ull << lane) - 1ull));
      if (pos >= kept) continue;
      const int64_t k = keys[i];
      int64_t tb;
      in_force<kHasDefault>(table, cap, k, default_bits, &tb);
      out_key[pos] = k;
      out_val[pos] = vals[i];
      out_t[pos] = tb;
      out_ts[pos] = ts[i];
    }
    __syncthreads();  // tword / tpre are refilled for the workgroup's next tile
  }
}

// ---- gather (every row kept) -----------------------------------------------------------------
__global__ __launch_bounds__(256) void lookup_gather_kernel(
    const int64_t* __restrict__ keys, const int64_t* __restrict__ vals,
    const int64_t* __restrict__ ts, int64_t n, const ll2* __restrict__ table, int64_t cap,
    int64_t default_bits, int64_t* __restrict__ out_key, int64_t* __restrict__ out_val,
    int64_t* __restrict__ out_t, int64_t* __restrict__ out_ts) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = keys[i];
    int64_t tb;
    in_force<true>(table, cap, k, default_bits, &tb);
    out_key[i] = k;
    out_val[i] = vals[i];
    out_t[i] = tb;
    out_ts[i] = ts[i];
  }
}

template <int kWhen>
void launch_mask(bool has_default, dim3 grid, hipStream_t s, const int64_t* keys,
                 const int64_t* vals, int64_t n, const ll2* table, int64_t cap,
                 int64_t default_bits, int64_t ntiles, uint64_t* words, uint32_t* counts) {
  if (has_default)
    hipLaunchKernelGGL((lookup_mask_kernel<kWhen, true>), grid, dim3(kLookupBlock), 0, s, keys,
                       vals, n, table, cap, default_bits, ntiles, words, counts);
  else
    hipLaunchKernelGGL((lookup_mask_kernel<kWhen, false>), grid, dim3(kLookupBlock), 0, s, keys,
                       vals, n, table, cap, default_bits, ntiles, words, counts);
}

void check_table(const int64_t* table, int64_t cap, const char* what) {
  if (cap < 0 || (cap > 0 && table == nullptr))
    throw std::invalid_argument(std::string(what) + ": bad table");
  if ((uintptr_t)table & 15u)
    throw std::invalid_argument(std::string(what) + ": the table must be 16-byte aligned");
}

}  // namespace

namespace gpu {

void lookup_upsert(const int64_t* skeys, const int64_t* perm, const int64_t* vals, int64_t n,
                   int64_t* table, int64_t cap, intptr_t stream) {
  check_table(table, cap, "lookup_upsert");
  if (n < 0) throw std::invalid_argument("lookup_upsert: negative row count");
  if (n == 0) return;
  hipLaunchKernelGGL(lookup_upsert_kernel, dim3(grid_of(n, 256, 8192)), dim3(256), 0,
                     (hipStream_t)stream, skeys, perm, vals, n, reinterpret_cast<ll2*>(table),
                     cap);
  MXS_HIP_CHECK(hipGetLastError());
}

void lookup_mask(const int64_t* keys, const int64_t* vals, int64_t n, const int64_t* table,
                 int64_t cap, int when, bool has_default, int64_t default_bits, uint64_t* words,
                 uint32_t* counts, intptr_t stream) {
  check_table(table, cap, "lookup_mask");
  if (n < 0) throw std::invalid_argument("lookup_mask: negative row count");
  if (when < 0 || when >= kLookupWhens) throw std::invalid_argument("lookup: unknown comparison");
  if (n == 0) return;
  const int64_t ntiles = (n + kLookupTile - 1) / kLookupTile;
  const dim3 grid(grid_of(ntiles, 1, kLookupMaxGrid));
  const ll2* t = reinterpret_cast<const ll2*>(table);
  hipStream_t s = (hipStream_t)stream;
#define LOOKUP_MASK_CASE(W)                                                                  \
  case W:                                                                                    \
    launch_mask<W>(has_default, grid, s, keys, vals, n, t, cap, default_bits, ntiles, words, \
                   counts);                                                                  \
    break
  switch (when) {
    LOOKUP_MASK_CASE(kLookupAll);
    LOOKUP_MASK_CASE(kLookupGt);
    LOOKUP_MASK_CASE(kLookupGe);
    LOOKUP_MASK_CASE(kLookupLt);
    LOOKUP_MASK_CASE(kLookupLe);
    LOOKUP_MASK_CASE(kLookupEq);
    LOOKUP_MASK_CASE(kLookupNe);
  }
#undef LOOKUP_MASK_CASE
  MXS_HIP_CHECK(hipGetLastError());
}

void lookup_scan(const uint32_t* counts, int64_t ntiles, int64_t* offsets, int64_t* meta,
                 intptr_t stream) {
  if (ntiles < 0) throw std::invalid_argument("lookup_scan: negative tile count");
  hipLaunchKernelGGL(lookup_scan_kernel, dim3(1), dim3(kScanThreads), 0, (hipStream_t)stream,
                     counts, ntiles, offsets, meta);
  MXS_HIP_CHECK(hipGetLastError());
}

// `words`, `counts` and `offsets` must be lookup_mask's and lookup_scan's output for these same
// columns and `kept` the scan's total: a row past `kept` is never written.
void lookup_emit(const int64_t* keys, const int64_t* vals, const int64_t* ts, int64_t n,
                 const int64_t* table, int64_t cap, bool has_default, int64_t default_bits,
                 const uint64_t* words, const uint32_t* counts, const int64_t* offsets,
                 int64_t kept, int64_t* out_key, int64_t* out_val, int64_t* out_t, int64_t* out_ts,
                 intptr_t stream) {
  check_table(table, cap, "lookup_emit");
  if (n < 0 || kept < 0 || kept > n) throw std::invalid_argument("lookup_emit: bad row counts");
  if (n == 0 || kept == 0) return;
  const int64_t ntiles = (n + kLookupTile - 1) / kLookupTile;
  const dim3 grid(grid_of(ntiles, 1, kLookupMaxGrid));
  const ll2* t = reinterpret_cast<const ll2*>(table);
  hipStream_t s = (hipStream_t)stream;
  if (has_default)
    hipLaunchKernelGGL(lookup_emit_kernel<true>, grid, dim3(kLookupBlock), 0, s, keys, vals, ts, n,
                       t, cap, default_bits, ntiles, words, counts, offsets, kept, out_key,
                       out_val, out_t, out_ts);
  else
    hipLaunchKernelGGL(lookup_emit_kernel<false>, grid, dim3(kLookupBlock), 0, s, keys, vals, ts,
                       n, t, cap, default_bits, ntiles, words, counts, offsets, kept, out_key,
                       out_val, out_t, out_ts);
  MXS_HIP_CHECK(hipGetLastError());
}

void lookup_gather(const int64_t* keys, const int64_t* vals, const int64_t* ts, int64_t n,
                   const int64_t* table, int64_t cap, int64_t default_bits, int64_t* out_key,
                   int64_t* out_val, int64_t* out_t, int64_t* out_ts, intptr_t stream) {
  check_table(table, cap, "lookup_gather");
  if (n < 0) throw std::invalid_argument("lookup_gather: negative row count");
  if (n == 0) return;
  hipLaunchKernelGGL(lookup_gather_kernel, dim3(grid_of(n, 256, 16384)), dim3(256), 0,
                     (hipStream_t)stream, keys, vals, ts, n, reinterpret_cast<const ll2*>(table),
                     cap, default_bits, out_key, out_val, out_t, out_ts);
  MXS_HIP_CHECK(hipGetLastError());
}

}  // namespace gpu
}  // namespace mxs
