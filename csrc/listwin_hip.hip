// mxstream — pane arena and counting-sort firing of `process` (list-state) windows on gfx950
// (declarations and the design: csrc/mxs_listwin.h; C++ twins: csrc/listwin_cpu.cpp).
//
// ComputeCpuMiddle.java:34-48 keeps every element of a (host, 1-min window) and takes the
// median. The elements of a batch are appended to their pane's device buffer (block-aggregated
// cursors: one global atomic per touched pane per workgroup). A firing counts the window's
// elements per dense key id, scans the counts (order-preserving, so segments come out in key
// order) and scatters the values into their key segments as order bits; the per-segment median
// selection (segment_median_select, csrc/kernels_hip.hip) never needs a comparison sort of the
// whole window. func "distinct" counts the different words of every segment instead
// (segment_distinct_short / segment_distinct_long below: hash sets in LDS and in a device scratch).
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "mxs_hip_util.h"
#include "mxs_listwin.h"
#include "pair_scan.h"

namespace mxs {
namespace {

__device__ __forceinline__ int lw_slot(int64_t t, int64_t offset, int64_t pane, int ring,
                                       int64_t late_ts) {
  if (t < late_ts) return ring;  // late: dropped (counted in the extra bin)
  return (int)(lw_floor_div(t - offset, pane) & (int64_t)(ring - 1));
}

constexpr int kLwBlock = 256;
constexpr int kLwItems = 16;  // elements per thread per tile (4096-element tiles)

__global__ __launch_bounds__(kLwBlock) void lw_pane_count_kernel(const int64_t* __restrict__ ts,
                                                                 int64_t n, int64_t offset,
                                                                 int64_t pane, int ring,
                                                                 int64_t late_ts,
                                                                 int64_t* __restrict__ counts) {
  extern __shared__ uint32_t hist[];  // ring + 1 bins
  for (int i = threadIdx.x; i <= ring; i += blockDim.x) hist[i] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    atomicAdd(&hist[lw_slot(ts[i], offset, pane, ring, late_ts)], 1u);
  __syncthreads();
  for (int i = threadIdx.x; i <= ring; i += blockDim.x)
    if (hist[i]) atomicAdd((unsigned long long*)&counts[i], (unsigned long long)hist[i]);
}

// A tile of kLwBlock * kLwItems elements: LDS counts per ring slot -> one global cursor atomic
// per touched slot -> every element's position = slot base + its LDS rank.
__global__ __launch_bounds__(kLwBlock) void lw_pane_scatter_kernel(
    const int64_t* __restrict__ keys, const int64_t* __restrict__ ts,
    const uint64_t* __restrict__ vals, int64_t n, int64_t offset, int64_t pane, int ring,
    int64_t late_ts, const int64_t* __restrict__ tab, int64_t* __restrict__ cursor) {
  extern __shared__ uint32_t sm[];
  uint32_t* cnt = sm;                                         // ring + 1
  unsigned long long* base = (unsigned long long*)(sm + ((ring + 2) & ~1));  // ring
  const int64_t tile = (int64_t)kLwBlock * kLwItems;
  for (int64_t t0 = (int64_t)blockIdx.x * tile; t0 < n; t0 += (int64_t)gridDim.x * tile) {
    for (int i = threadIdx.x; i <= ring; i += blockDim.x) cnt[i] = 0;
    __syncthreads();
    int slot[kLwItems];
#pragma unroll
    for (int u = 0; u < kLwItems; ++u) {
      const int64_t i = t0 + (int64_t)u * kLwBlock + threadIdx.x;
      slot[u] = i < n ? lw_slot(ts[i], offset, pane, ring, late_ts) : ring;
      if (i < n && slot[u] < ring) atomicAdd(&cnt[slot[u]], 1u);
    }
    __syncthreads();
    for (int r = threadIdx.x; r < ring; r += blockDim.x) {
      const uint32_t c = cnt[r];
      base[r] = c ? atomicAdd((unsigned long long*)&cursor[r], (unsigned long long)c) : 0ull;
      cnt[r] = 0;  // reused as the tile's rank cursor
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kLwItems; ++u) {
      const int64_t i = t0 + (int64_t)u * kLwBlock + threadIdx.x;
      if (i < n && slot[u] < ring) {
        const int r = slot[u];
        const unsigned long long pos = base[r] + atomicAdd(&cnt[r], 1u);
        const int64_t key = keys[i];
        reinterpret_cast<int64_t*>(tab[r])[pos] = key;
        reinterpret_cast<uint64_t*>(tab[ring + r])[pos] = vals[i];
        uint32_t* kc = reinterpret_cast<uint32_t*>(tab[3 * ring + r]);
        if (kc)  // rank of the element among its key's elements of this pane
          reinterpret_cast<uint32_t*>(tab[2 * ring + r])[pos] =
              atomicAdd(&kc[key - tab[4 * ring + r]], 1u);
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kLwBlock) void lw_key_count_kernel(LwPanes w, int64_t kmin,
                                                                uint32_t* __restrict__ counts) {
  const LwPane& p = w.p[blockIdx.y];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.len;
       i += (int64_t)gridDim.x * blockDim.x)
    atomicAdd(&counts[p.keys[i] - kmin], 1u);
}

__global__ __launch_bounds__(kLwBlock) void lw_key_scatter_kernel(LwPanes w, int64_t kmin,
                                                                  int64_t* __restrict__ cursor,
                                                                  uint64_t* __restrict__ out) {
  const LwPane& p = w.p[blockIdx.y];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.len;
       i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long pos =
        atomicAdd((unsigned long long*)&cursor[p.keys[i] - kmin], 1ull);
    out[pos] = f64_order_bits(p.vals[i]);
  }
}

// Per key of the window: the panes' counts -> each pane's prefix and the total.
__global__ __launch_bounds__(kLwBlock) void lw_rank_prefix_kernel(LwRankPanes w, int64_t kmin,
                                                                  int64_t nkeys,
                                                                  uint32_t* __restrict__ total,
                                                                  uint32_t* __restrict__ pre) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nkeys;
       k += (int64_t)gridDim.x * blockDim.x) {
    const int64_t key = kmin + k;
    uint32_t run = 0;
    for (int j = 0; j < w.n; ++j) {
      const LwRankPane& p = w.p[j];
      const int64_t o = key - p.kbase;
      pre[(int64_t)j * nkeys + k] = run;
      run += (o >= 0 && o < p.ksize) ? p.counts[o] : 0u;
    }
    total[k] = run;
  }
}

// Placement without atomics: segment start + earlier panes' count of the key + rank.
__global__ __launch_bounds__(kLwBlock) void lw_rank_scatter_kernel(LwRankPanes w, int64_t kmin,
                                                                   int64_t nkeys,
                                                                   const int64_t* __restrict__ offs,
                                                                   const uint32_t* __restrict__ pre,
                                                                   uint64_t* __restrict__ out) {
  const LwRankPane& p = w.p[blockIdx.y];
  const uint32_t* pj = pre + (int64_t)blockIdx.y * nkeys;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.len;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = p.keys[i] - kmin;
    out[offs[k] + pj[k] + p.ranks[i]] = f64_order_bits(p.vals[i]);
  }
}

// ---- order-preserving scan of the key counts (csrc/pair_scan.h, plain 64-bit sums) ----------
static_assert(kLwScanTile == kJoinScanTile, "lw_scan_scratch_bytes is sized by the pair scan");

struct LwScan {
  using Add = Add64;
  const uint32_t* counts;
  int64_t nkeys, kmin;
  int64_t *offs, *heads, *head_keys, *nheads;

  __device__ __forceinline__ uint64_t count(int64_t i) const { return counts[i]; }
  __device__ __forceinline__ void element(int64_t i, uint64_t o) const { offs[i] = (int64_t)o; }
  // the (start, key) of a non-empty key, in key order
  __device__ __forceinline__ void nonempty(int64_t i, int64_t h, uint64_t o) const {
    heads[h] = (int64_t)o;
    head_keys[h] = kmin + i;
  }
  __device__ __forceinline__ void finish(uint64_t total, uint32_t m) const {
    offs[nkeys] = (int64_t)total;
    *nheads = (int64_t)m;
  }
};

// ---- distinct count of every segment (func "distinct") -------------------------------------
// The slot of word x in a table of `cap` (power of two) slots is the top log2(cap) bits of
// mix64(x) (bijective, so different words differ somewhere in the mixed word); in a table of
// any size m it is mulhi(mix64(x), m). Tables are at most half full, so linear probing ends;
// the loops are bounded by the table size all the same and report a hit bound in
// meta[kDistinctErr].
__device__ __forceinline__ void lw_wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// One wave per segment, four per workgroup (the median kernel's layout and LDS budget: 4 x 2048
// words). The wave clears cap = max(128, next_pow2(2n)) slots, every lane reads its words from
// global memory once and claims a slot with a 64-bit LDS compare-and-swap: old value empty =
// claimed (a new word), old value x = duplicate, anything else = next slot. A segment of more
// than kDistinctLds words is only listed here (one atomic reserves its list entry and its 2n
// scratch words) and counted by segment_distinct_long_kernel.
__global__ __launch_bounds__(256) void segment_distinct_short_kernel(
    const int64_t* __restrict__ heads, int64_t nseg, int64_t total,
    const uint64_t* __restrict__ ord, int64_t* __restrict__ out, int64_t* __restrict__ list,
    int64_t list_cap, int64_t* __restrict__ meta) {
  __shared__ unsigned long long tab[4][2 * kDistinctLds];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned long long* t = tab[w];
  for (int64_t s = (int64_t)blockIdx.x * 4 + w; s < nseg; s += (int64_t)gridDim.x * 4) {
    const int64_t a = heads[s], e = s + 1 < nseg ? heads[s + 1] : total;
    const int64_t n = e - a;
    if (n <= 0) {
      if (lane == 0) out[s] = 0;
      continue;
    }
    if (n > kDistinctLds) {
      if (lane == 0) {
        out[s] = 0;
        const unsigned long long c =
            atomicAdd((unsigned long long*)&meta[kDistinctCursor],
                      (1ull << kDistinctWordBits) + 2ull * (unsigned long long)n);
        const int64_t idx = (int64_t)(c >> kDistinctWordBits);
        if (idx < list_cap) {
          list[idx * kDistinctEntry] = s;
          list[idx * kDistinctEntry + 1] = (int64_t)(c & ((1ull << kDistinctWordBits) - 1ull));
        } else {
          meta[kDistinctErr] = 2;
        }
      }
      continue;
    }
    int cap = 128;
    while (cap < 2 * (int)n) cap <<= 1;
    const int shift = 33 + __clz(cap);  // 64 - log2(cap)
    for (int i = lane; i < cap; i += 64) t[i] = kDistinctEmpty;
    lw_wave_lds_sync();
    uint32_t claims = 0;
    bool saw_empty = false, spun = false;
    // Four independent loads per lane in flight before the first insert (a word past the end
    // reads as the empty marker without counting as one).
    for (int i0 = lane; i0 < (int)n; i0 += 4 * 64) {
      unsigned long long x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * 64;
        x[u] = i < (int)n ? ord[a + i] : (unsigned long long)kDistinctEmpty;
        saw_empty = saw_empty || (i < (int)n && x[u] == kDistinctEmpty);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (x[u] == kDistinctEmpty) continue;
        int slot = (int)(mix64(x[u]) >> shift);
        int probes = 0;
        for (; probes < cap; ++probes) {
          const unsigned long long old =
              atomicCAS(&t[slot], (unsigned long long)kDistinctEmpty, x[u]);
          if (old == kDistinctEmpty) {
            ++claims;
            break;
          }
          if (old == x[u]) break;
          slot = (slot + 1) & (cap - 1);
        }
        spun = spun || probes == cap;
      }
    }
    for (int o = 32; o >= 1; o >>= 1) claims += __shfl_xor(claims, o);
    const bool any_empty = __ballot(saw_empty) != 0ull, any_spun = __ballot(spun) != 0ull;
    if (lane == 0) {
      out[s] = (int64_t)claims + (any_empty ? 1 : 0);
      if (any_spun) meta[kDistinctErr] = 1;
    }
    lw_wave_lds_sync();  // every lane is done with the table before the next segment clears it
  }
}

// The listed long segments, laid end to end in list order (entry j starts at element base_j / 2:
// the short pass reserved 2n words per segment with one atomic, so bases ascend with j). Every
// workgroup takes tiles of kDistinctTile of those elements, so one hot key's segment is spread
// over many workgroups that insert into the same table with 64-bit global compare-and-swap; a
// relaxed load first keeps duplicates (the common case of a hot key) off the atomic unit -- a
// slot only ever goes from empty to one word, so a value seen there is final. Claims are summed
// per workgroup and added to out[s] with one atomic; the first workgroup to flag that it saw
// the empty marker adds one for it.
__global__ __launch_bounds__(256) void segment_distinct_long_kernel(
    const int64_t* __restrict__ heads, int64_t nseg, int64_t total,
    const uint64_t* __restrict__ ord, int64_t* __restrict__ list, int64_t n_long,
    int64_t long_elems, uint64_t* __restrict__ scratch, int64_t* __restrict__ out,
    int64_t* __restrict__ meta) {
  __shared__ uint32_t wsum[4], wflag[4];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int64_t t0 = (int64_t)blockIdx.x * kDistinctTile; t0 < long_elems;
       t0 += (int64_t)gridDim.x * kDistinctTile) {
    const int64_t t1 = t0 + kDistinctTile < long_elems ? t0 + kDistinctTile : long_elems;
    // the last entry that starts at or before t0 (entry 0 starts at 0)
    int64_t lo = 0, hi = n_long;
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if ((list[mid * kDistinctEntry + 1] >> 1) <= t0) lo = mid; else hi = mid;
    }
    for (int64_t j = lo; j < n_long; ++j) {
      const int64_t s = list[j * kDistinctEntry], base = list[j * kDistinctEntry + 1];
      const int64_t e0 = base >> 1;
      if (e0 >= t1) break;
      const int64_t a = heads[s], n = (s + 1 < nseg ? heads[s + 1] : total) - a;
      const int64_t b = (t0 > e0 ? t0 : e0) - e0, e = (t1 < e0 + n ? t1 : e0 + n) - e0;
      const uint64_t m = 2ull * (uint64_t)n;
      unsigned long long* tb = reinterpret_cast<unsigned long long*>(scratch + base);
      uint32_t claims = 0;
      bool saw_empty = false, spun = false;
      for (int64_t i = b + threadIdx.x; i < e; i += 256) {
        const unsigned long long x = ord[a + i];
        if (x == kDistinctEmpty) {
          saw_empty = true;
          continue;
        }
        uint64_t slot = __umul64hi(mix64(x), m);
        uint64_t probes = 0;
        for (; probes < m; ++probes) {
          unsigned long long old =
              __hip_atomic_load(&tb[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (old == kDistinctEmpty) {
            old = atomicCAS(&tb[slot], (unsigned long long)kDistinctEmpty, x);
            if (old == kDistinctEmpty) {
              ++claims;
              break;
            }
          }
          if (old == x) break;
          slot = slot + 1 == m ? 0 : slot + 1;
        }
        spun = spun || probes == m;
      }
      for (int o = 32; o >= 1; o >>= 1) claims += __shfl_xor(claims, o);
      const bool any_empty = __ballot(saw_empty) != 0ull, any_spun = __ballot(spun) != 0ull;
      if (lane == 0) {
        wsum[w] = claims;
        wflag[w] = (any_empty ? 1u : 0u) | (any_spun ? 2u : 0u);
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        unsigned long long sum = (unsigned long long)wsum[0] + wsum[1] + wsum[2] + wsum[3];
        const uint32_t f = wflag[0] | wflag[1] | wflag[2] | wflag[3];
        if ((f & 1u) &&
            atomicCAS((unsigned long long*)&list[j * kDistinctEntry + 2], 0ull, 1ull) == 0ull)
          ++sum;
        if (sum) atomicAdd((unsigned long long*)&out[s], sum);
        if (f & 2u) meta[kDistinctErr] = 1;
      }
      __syncthreads();
    }
  }
}

}  // namespace

namespace gpu {

void lw_pane_count(const int64_t* ts, int64_t n, int64_t offset, int64_t pane, int ring,
                   int64_t late_ts, int64_t* counts, intptr_t stream) {
  if (n <= 0) return;
  if (ring < 1 || ring > kLwMaxRing || (ring & (ring - 1)))
    throw std::invalid_argument("lw_pane_count: ring must be a power of two <= 4096");
  const size_t lds = sizeof(uint32_t) * (size_t)(ring + 1);
  hipLaunchKernelGGL(lw_pane_count_kernel, dim3(grid_of(n, kLwBlock * 16, 2048)), dim3(kLwBlock),
                     lds, (hipStream_t)stream, ts, n, offset, pane, ring, late_ts, counts);
  MXS_HIP_CHECK(hipGetLastError());
}

void lw_pane_scatter(const int64_t* keys, const int64_t* ts, const uint64_t* vals, int64_t n,
                     int64_t offset, int64_t pane, int ring, int64_t late_ts, const int64_t* tab,
                     int64_t* cursor, intptr_t stream) {
  if (n <= 0) return;
  if (ring < 1 || ring > kLwMaxRing || (ring & (ring - 1)))
    throw std::invalid_argument("lw_pane_scatter: ring must be a power of two <= 4096");
  const size_t lds = sizeof(uint32_t) * (size_t)((ring + 2) & ~1) + sizeof(uint64_t) * ring;
  hipLaunchKernelGGL(lw_pane_scatter_kernel, dim3(grid_of(n, kLwBlock * kLwItems, 4096)),
                     dim3(kLwBlock), lds, (hipStream_t)stream, keys, ts, vals, n, offset, pane,
                     ring, late_ts, tab, cursor);
  MXS_HIP_CHECK(hipGetLastError());
}

void lw_key_count(const LwPanes& w, int64_t kmin, int64_t nkeys, uint32_t* counts,
                  intptr_t stream) {
  if (w.n <= 0 || w.n > kLwMaxPanes) throw std::invalid_argument("lw_key_count: 1..64 panes");
  (void)nkeys;
  int64_t mx = 0;
  for (int i = 0; i < w.n; ++i) mx = w.p[i].len > mx ? w.p[i].len : mx;
  if (mx <= 0) return;
  hipLaunchKernelGGL(lw_key_count_kernel, dim3(grid_of(mx, kLwBlock * 8, 4096), w.n),
                     dim3(kLwBlock), 0, (hipStream_t)stream, w, kmin, counts);
  MXS_HIP_CHECK(hipGetLastError());
}

int64_t lw_scan_scratch_bytes(int64_t nkeys) { return pair_scan_scratch_bytes(nkeys); }

void lw_scan(const uint32_t* counts, int64_t nkeys, int64_t kmin, void* scratch, int64_t* offs,
             int64_t* heads, int64_t* head_keys, int64_t* nheads, intptr_t stream) {
  if (nkeys <= 0) throw std::invalid_argument("lw_scan: empty key range");
  if (nkeys > (16ll << 20))  // the callers' key ranges are far below; kept as their contract
    throw std::invalid_argument("lw_scan: more than 16 Mi keys");
  const LwScan p = {counts, nkeys, kmin, offs, heads, head_keys, nheads};
  pair_scan_launch(p, nkeys, scratch, (hipStream_t)stream);
}

void lw_key_scatter(const LwPanes& w, int64_t kmin, int64_t* cursor, uint64_t* out_ord,
                    intptr_t stream) {
  if (w.n <= 0 || w.n > kLwMaxPanes) throw std::invalid_argument("lw_key_scatter: 1..64 panes");
  int64_t mx = 0;
  for (int i = 0; i < w.n; ++i) mx = w.p[i].len > mx ? w.p[i].len : mx;
  if (mx <= 0) return;
  hipLaunchKernelGGL(lw_key_scatter_kernel, dim3(grid_of(mx, kLwBlock * 8, 4096), w.n),
                     dim3(kLwBlock), 0, (hipStream_t)stream, w, kmin, cursor, out_ord);
  MXS_HIP_CHECK(hipGetLastError());
}

void lw_rank_prefix(const LwRankPanes& w, int64_t kmin, int64_t nkeys, uint32_t* total,
                    uint32_t* pre, intptr_t stream) {
  if (w.n <= 0 || w.n > kLwMaxRankPanes) throw std::invalid_argument("lw_rank_prefix: 1..32 panes");
  if (nkeys <= 0) return;
  hipLaunchKernelGGL(lw_rank_prefix_kernel, dim3(grid_of(nkeys, kLwBlock, 4096)), dim3(kLwBlock),
                     0, (hipStream_t)stream, w, kmin, nkeys, total, pre);
  MXS_HIP_CHECK(hipGetLastError());
}

void lw_rank_scatter(const LwRankPanes& w, int64_t kmin, int64_t nkeys, const int64_t* offs,
                     const uint32_t* pre, uint64_t* out_ord, intptr_t stream) {
  if (w.n <= 0 || w.n > kLwMaxRankPanes) throw std::invalid_argument("lw_rank_scatter: 1..32 panes");
  int64_t mx = 0;
  for (int i = 0; i < w.n; ++i) mx = w.p[i].len > mx ? w.p[i].len : mx;
  if (mx <= 0) return;
  hipLaunchKernelGGL(lw_rank_scatter_kernel, dim3(grid_of(mx, kLwBlock * 8, 4096), w.n),
                     dim3(kLwBlock), 0, (hipStream_t)stream, w, kmin, nkeys, offs, pre, out_ord);
  MXS_HIP_CHECK(hipGetLastError());
}

void segment_distinct_short(const int64_t* heads, int64_t nseg, int64_t total, const uint64_t* ord,
                            int64_t* out, int64_t* list, int64_t list_cap, int64_t* meta,
                            intptr_t stream) {
  if (total < 0 || total >= (1ll << (kDistinctWordBits - 2)))
    throw std::invalid_argument("segment_distinct: total out of range");
  if (list_cap < total / (kDistinctLds + 1))
    throw std::invalid_argument("segment_distinct: list shorter than total / 1025 entries");
  if (nseg <= 0) return;
  hipLaunchKernelGGL(segment_distinct_short_kernel, dim3(grid_of(nseg, 4, 16384)), dim3(256), 0,
                     (hipStream_t)stream, heads, nseg, total, ord, out, list, list_cap, meta);
  MXS_HIP_CHECK(hipGetLastError());
}

void segment_distinct_long(const int64_t* heads, int64_t nseg, int64_t total, const uint64_t* ord,
                           int64_t* list, int64_t n_long, int64_t long_elems, uint64_t* scratch,
                           int64_t* out, int64_t* meta, intptr_t stream) {
  if (n_long <= 0 || long_elems <= 0) return;
  if (n_long > nseg || long_elems > total || long_elems < n_long * (int64_t)(kDistinctLds + 1))
    throw std::invalid_argument("segment_distinct: long-segment counts out of range");
  hipLaunchKernelGGL(segment_distinct_long_kernel, dim3(grid_of(long_elems, kDistinctTile, 8192)),
                     dim3(256), 0, (hipStream_t)stream, heads, nseg, total, ord, list, n_long,
                     long_elems, scratch, out, meta);
  MXS_HIP_CHECK(hipGetLastError());
}

}  // namespace gpu
}  // namespace mxs
