// mxstream — counter rates on gfx950: the increase and the rate between consecutive accepted
// samples of a key's cumulative counter (declarations, the model and the algebra:
// csrc/mxs_rate.h; C++ twin: csrc/rate_cpu.cpp).
//
// scan: the batch arrives stably sorted by key and is scanned in the frame of csrc/rule_scan.h,
// as fsm_scan_kernel does: a wave owns the key runs that begin in its 64 sorted rows and walks on
// a run that leaves them, so a key's 16-byte row has one reader and one writer and no atomics
// touch the state. What is this rule's own: an element is the pair (t, v), a stretch of elements
// is its arg-max by t, earliest on ties, and an element's baseline is the exclusive prefix of
// that over its run with the key's row in front. A based element writes (inc bits, dt) at its
// ARRIVAL index, every other owned element dt = 0 there: the scratch needs no memset. Ignored
// elements are counted with one ballot and at most one atomicAdd per wave and chunk.
// mask / emit: the order-preserving compaction of the lookup (csrc/lookup_hip.hip) over the
// scratch rows, read coalesced, 16 bytes per lane: ballot words and tile counts, lookup_scan for
// the offsets and the total, then the five columns of the kept rows in arrival order. Mask and
// emit compute the rate with the twin's own function (rate_keep -> rate_of).
// No LDS in the scan, no scratch beyond the n rows.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "mxs_rate.h"
#include "rule_scan.h"

namespace mxs {
namespace {

constexpr int kRateBlock = 256;
constexpr int kRateMaxGrid = 8192;
constexpr int kRateWaves = kRateBlock / 64;
constexpr int kRateRounds = kLookupTile / kRateBlock;  // rows per lane of a tile
constexpr int kRateTileGrid = 1 << 20;                 // longer inputs stride over their tiles

template <int kKind>
__global__ __launch_bounds__(kRateBlock) void rate_scan_kernel(
    const int64_t* __restrict__ skeys, const int64_t* __restrict__ perm,
    const int64_t* __restrict__ vals, const int64_t* __restrict__ ts, int64_t n,
    ll2* __restrict__ state, int64_t cap, ll2* __restrict__ scratch,
    uint32_t* __restrict__ out_ooo) {
  const int lane = threadIdx.x & 63;
  // Every loop condition is wave-uniform (csrc/rule_scan.h).
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < n;
       base += (int64_t)gridDim.x * blockDim.x) {
    bool cont = false;  // walking on a run that left the wave's own chunk
    int64_t ck = 0, ct = kRateNone, cv = 0;
    for (int64_t b0 = base;; b0 += 64) {
      RuleFrame fr = rule_heads(skeys, n, b0, lane, cont);
      if (fr.leave) break;
      rule_owned(skeys, perm, n, cap, lane, cont, ck, fr);
      const int64_t k = fr.k, src = fr.src;
      const bool ok = fr.ok;
      // a lane outside the wave's runs is the identity: it never wins a combine
      const int64_t t = ok ? ts[src] : kRateNone;
      const int64_t v = ok ? vals[src] : 0;
      if (!cont) {
        ll2 row;
        row.x = kRateNone, row.y = 0;
        if (ok) row = state[k];  // one 16-byte load; a run's lanes read the same row
        ct = row.x, cv = row.y;
      }
      // Inclusive segmented wave scan (Hillis-Steele) of the pair; y is the earlier one and
      // keeps a tie.
      int64_t st = t, sv = v;
      int f = fr.head;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int64_t yt = (int64_t)__shfl_up((long long)st, o);
        const int64_t yv = (int64_t)__shfl_up((long long)sv, o);
        const int g = __shfl_up(f, o);
        if (lane >= o && !f) {
          if (!(st > yt)) st = yt, sv = yv;
          f = g;
        }
      }
      // The key's accepted sample after this element, and the one before it.
      const bool newer = st > ct;
      const int64_t at = newer ? st : ct, av = newer ? sv : cv;
      const int64_t bt = rule_before(at, ct, fr.head, lane);
      const int64_t bv = rule_before(av, cv, fr.head, lane);
      const bool accepted = ok && t > bt;
      const bool based = accepted && bt != kRateNone;
      if (fr.act && (uint64_t)src < (uint64_t)n) {
        ll2 row;
        row.x = based ? rate_increase(kKind, v, bv) : 0;
        row.y = based ? t - bt : 0;  // > 0 for a row, 0: none
        scratch[src] = row;          // one 16-byte store at the arrival index
      }
      if (fr.tail && ok) {
        ll2 row;
        row.x = at, row.y = av;
        state[k] = row;  // one 16-byte store by the lane that ends the run
      }
      const unsigned long long im = __ballot(ok && !accepted);
      if (lane == 0 && im) atomicAdd(out_ooo, (uint32_t)__popcll(im));
      if (!rule_run_goes_on(fr.act, __ballot(fr.tail))) break;
      cont = true;
      ck = __shfl(k, 63);
      ct = (int64_t)__shfl((long long)at, 63);
      cv = (int64_t)__shfl((long long)av, 63);
    }
  }
}

// ---- mask ----------------------------------------------------------------------------------
// Round r of a tile: wave w holds rows [256 r + 64 w, + 64) = mask word 4 r + w (lookup_mask's
// layout).
__global__ __launch_bounds__(kRateBlock) void rate_mask_kernel(
    const ll2* __restrict__ scratch, int64_t n, const RateRule rule, int64_t ntiles,
    uint64_t* __restrict__ words, uint32_t* __restrict__ counts) {
  __shared__ uint32_t wcount[kRateWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t base = tile * kLookupTile + threadIdx.x;
    uint32_t kept = 0;
#pragma unroll 4
    for (int r = 0; r < kRateRounds; ++r) {
      const int64_t i = base + (int64_t)r * kRateBlock;
      ll2 row;
      row.x = 0, row.y = 0;
      if (i < n) row = scratch[i];
      double rate;
      const bool keep = rate_keep(rule, row.x, row.y, &rate);
      const uint64_t word = __ballot(keep);
      if (lane == 0) words[tile * kLookupWords + r * kRateWaves + wave] = word;
      kept += (uint32_t)__popcll(word);
    }
    if (lane == 0) wcount[wave] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t c = 0;
      for (int w = 0; w < kRateWaves; ++w) c += wcount[w];
      counts[tile] = c;
    }
    __syncthreads();  // wcount is rewritten for the workgroup's next tile
  }
}

// ---- emit ----------------------------------------------------------------------------------
__global__ __launch_bounds__(kRateBlock) void rate_emit_kernel(
    const ll2* __restrict__ scratch, const int64_t* __restrict__ keys,
    const int64_t* __restrict__ ts, int64_t n, const RateRule rule, int64_t ntiles,
    const uint64_t* __restrict__ words, const uint32_t* __restrict__ counts,
    const int64_t* __restrict__ offsets, int64_t kept, int64_t* __restrict__ out_key,
    int64_t* __restrict__ out_rate, int64_t* __restrict__ out_inc, int64_t* __restrict__ out_dt,
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
    for (int r = 0; r < kRateRounds; ++r) {
      const int j = r * kRateWaves + wave;
      const uint64_t w = tword[j];
      if (w == 0) continue;  // uniform over the wave
      const int64_t i = base + (int64_t)r * kRateBlock;
      if (!((w >> lane) & 1ull) || i >= n) continue;
      const int64_t pos = off + tpre[j] + __popcll(w & ((1ull << lane) - 1ull));
      if (pos >= kept) continue;
      const ll2 row = scratch[i];
      out_key[pos] = keys[i];
      out_rate[pos] = rate_bits(rate_of(rule.kind, row.x, rule.per_ms, row.y));
      out_inc[pos] = row.x;
      out_dt[pos] = row.y;
      out_ts[pos] = ts[i];
    }
    __syncthreads();  // tword / tpre are refilled for the workgroup's next tile
  }
}

void check_scratch(const int64_t* scratch, int64_t n, const char* what) {
  if (n < 0 || n >= ((int64_t)1 << 31))
    throw std::invalid_argument(std::string(what) + ": bad row count");
  if (n > 0 && (scratch == nullptr || ((uintptr_t)scratch & 15u)))
    throw std::invalid_argument(std::string(what) + ": the scratch rows must be 16-byte aligned");
}

}  // namespace

namespace gpu {

void rate_scan(const int64_t* skeys, const int64_t* perm, const int64_t* vals, const int64_t* ts,
               int64_t n, int kind, int64_t* state, int64_t cap, int64_t* scratch,
               uint32_t* out_ooo, intptr_t stream) {
  if (cap < 1 || state == nullptr || ((uintptr_t)state & 15u))
    throw std::invalid_argument("rate_scan: the table must be 16-byte aligned, cap >= 1");
  check_scratch(scratch, n, "rate_scan");
  if (kind != kSustainLong && kind != kSustainDouble)
    throw std::invalid_argument("rate_scan: unknown value kind");
  if (out_ooo == nullptr) throw std::invalid_argument("rate_scan: no counter");
  hipStream_t s = (hipStream_t)stream;
  MXS_HIP_CHECK(hipMemsetAsync(out_ooo, 0, sizeof(uint32_t), s));
  if (n == 0) return;
  const dim3 grid(grid_of(n, kRateBlock, kRateMaxGrid));
  ll2* st = reinterpret_cast<ll2*>(state);
  ll2* sc = reinterpret_cast<ll2*>(scratch);
  if (kind == kSustainDouble)
    hipLaunchKernelGGL(rate_scan_kernel<kSustainDouble>, grid, dim3(kRateBlock), 0, s, skeys, perm,
                       vals, ts, n, st, cap, sc, out_ooo);
  else
    hipLaunchKernelGGL(rate_scan_kernel<kSustainLong>, grid, dim3(kRateBlock), 0, s, skeys, perm,
                       vals, ts, n, st, cap, sc, out_ooo);
  MXS_HIP_CHECK(hipGetLastError());
}

void rate_mask(const int64_t* scratch, int64_t n, const RateRule& rule, uint64_t* words,
               uint32_t* counts, intptr_t stream) {
  check_scratch(scratch, n, "rate_mask");
  if (n == 0) return;
  const int64_t ntiles = (n + kLookupTile - 1) / kLookupTile;
  hipLaunchKernelGGL(rate_mask_kernel, dim3(grid_of(ntiles, 1, kRateTileGrid)), dim3(kRateBlock),
                     0, (hipStream_t)stream, reinterpret_cast<const ll2*>(scratch), n, rule,
                     ntiles, words, counts);
  MXS_HIP_CHECK(hipGetLastError());
}

// `words`, `counts` and `offsets` must be rate_mask's and lookup_scan's output for these same
// scratch rows and `kept` the scan's total: a row past `kept` is never written.
void rate_emit(const int64_t* scratch, const int64_t* keys, const int64_t* ts, int64_t n,
               const RateRule& rule, const uint64_t* words, const uint32_t* counts,
               const int64_t* offsets, int64_t kept, int64_t* out_key, int64_t* out_rate,
               int64_t* out_inc, int64_t* out_dt, int64_t* out_ts, intptr_t stream) {
  check_scratch(scratch, n, "rate_emit");
  if (kept < 0 || kept > n) throw std::invalid_argument("rate_emit: bad row counts");
  if (n == 0 || kept == 0) return;
  const int64_t ntiles = (n + kLookupTile - 1) / kLookupTile;
  hipLaunchKernelGGL(rate_emit_kernel, dim3(grid_of(ntiles, 1, kRateTileGrid)), dim3(kRateBlock),
                     0, (hipStream_t)stream, reinterpret_cast<const ll2*>(scratch), keys, ts, n,
                     rule, ntiles, words, counts, offsets, kept, out_key, out_rate, out_inc,
                     out_dt, out_ts);
  MXS_HIP_CHECK(hipGetLastError());
}

}  // namespace gpu
}  // namespace mxs
