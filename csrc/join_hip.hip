// mxstream — keyed window joins on gfx950: match the two sides' key segments, scan the pair
// counts, expand every matched key's nL x nR pairs (declarations and the layout of the plan:
// csrc/mxs_join.h; C++ twins: csrc/join_cpu.cpp).
//
// The expand is output-centric: a workgroup owns kJoinTile consecutive output positions, finds
// the matched segments that overlap them by two binary searches in the plan's (strictly
// increasing) first-pair column and keeps their tile-relative starts in LDS. A hot key's millions
// of pairs are thus spread over as many workgroups as it has tiles, and thousands of small keys
// share one. Every lane writes two consecutive positions per column with one 16-byte store; a
// wave covers 128 consecutive positions (1 KiB per column and store). No atomics and no device
// counter: every position is known from the scan.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "mxs_join.h"
#include "mxs_blockscan.h"

namespace mxs {
namespace {

#define JOIN_CHECK(x)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (x);                                                                    \
    if (e_ != hipSuccess)                                                                   \
      throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(e_) + " at " + \
                               __FILE__ + ":" + std::to_string(__LINE__));                  \
  } while (0)

int grid_of(int64_t n, int per_block, int cap) {
  int64_t g = (n + per_block - 1) / per_block;
  if (g < 1) g = 1;
  return (int)(g < cap ? g : cap);
}

__device__ __forceinline__ int64_t seg_len(const int64_t* __restrict__ heads, int64_t nseg,
                                           int64_t total, int64_t i) {
  return (i + 1 < nseg ? heads[i + 1] : total) - heads[i];
}

// ---- match ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void join_match_kernel(
    const int64_t* __restrict__ lkeys, const int64_t* __restrict__ lheads, int64_t kl,
    int64_t ltotal, const int64_t* __restrict__ rkeys, const int64_t* __restrict__ rheads,
    int64_t kr, int64_t rtotal, int64_t* __restrict__ match, uint64_t* __restrict__ cnt) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < kl;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t key = lkeys[i];
    int64_t lo = 0, hi = kr;  // first right segment whose key is >= key
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (rkeys[mid] < key) lo = mid + 1; else hi = mid;
    }
    const bool hit = lo < kr && rkeys[lo] == key;
    match[i] = hit ? lo : -1;
    cnt[i] = hit ? join_sat_mul((uint64_t)seg_len(lheads, kl, ltotal, i),
                                (uint64_t)seg_len(rheads, kr, rtotal, lo))
                 : 0ull;
  }
}

// ---- scan (64-bit, saturating; the tiles + one-workgroup tile scan of lw_scan) ---------------
constexpr int kScanThreads = 1024;
constexpr int kScanPer = kJoinScanTile / kScanThreads;  // 4 segments per thread

// Pass 1: per tile, the pair total and the number of matched (non-empty) segments.
__global__ __launch_bounds__(kScanThreads) void join_tile_sums_kernel(
    const uint64_t* __restrict__ cnt, int64_t kl, uint64_t* __restrict__ tsum,
    uint32_t* __restrict__ tne) {
  __shared__ uint64_t ws[16];
  __shared__ uint32_t wn[16];
  __shared__ uint64_t tot;
  __shared__ uint32_t totn;
  const int64_t k0 = (int64_t)blockIdx.x * kJoinScanTile + (int64_t)threadIdx.x * kScanPer;
  uint64_t s = 0;
  uint32_t ne = 0;
#pragma unroll
  for (int j = 0; j < kScanPer; ++j) {
    const uint64_t c = k0 + j < kl ? cnt[k0 + j] : 0ull;
    s = join_sat_add(s, c);
    ne += c ? 1u : 0u;
  }
  block_excl_scan<uint64_t>(s, ws, &tot, SatAdd());
  block_excl_scan<uint32_t>(ne, wn, &totn, Add32());
  if (threadIdx.x == 0) {
    tsum[blockIdx.x] = tot;
    tne[blockIdx.x] = totn;
  }
}

// Pass 2 (one workgroup): exclusive scan of the tile totals, kScanThreads tiles per round with a
// carry, so any number of tiles; the totals P, m and the error word.
__global__ __launch_bounds__(kScanThreads) void join_tile_scan_kernel(
    uint64_t* __restrict__ tsum, uint32_t* __restrict__ tne, int64_t ntiles, int64_t kl,
    int64_t* __restrict__ pair_off, int64_t* __restrict__ plan, int64_t* __restrict__ meta) {
  __shared__ uint64_t ws[16];
  __shared__ uint32_t wn[16];
  __shared__ uint64_t tot;
  __shared__ uint32_t totn;
  uint64_t carry = 0;
  uint32_t carry_n = 0;
  for (int64_t base = 0; base < ntiles; base += kScanThreads) {
    const int64_t t = base + threadIdx.x;
    const uint64_t s = t < ntiles ? tsum[t] : 0ull;
    const uint32_t e = t < ntiles ? tne[t] : 0u;
    const uint64_t bs = block_excl_scan<uint64_t>(s, ws, &tot, SatAdd());
    const uint32_t be = block_excl_scan<uint32_t>(e, wn, &totn, Add32());
    if (t < ntiles) {
      tsum[t] = join_sat_add(carry, bs);
      tne[t] = carry_n + be;
    }
    carry = join_sat_add(carry, tot);
    carry_n += totn;
    __syncthreads();  // tot / totn are rewritten by the next round
  }
  if (threadIdx.x == 0) {
    pair_off[kl] = (int64_t)carry;
    plan[(int64_t)kJoinFirst * (kl + 1) + carry_n] = (int64_t)carry;
    meta[kJoinP] = (int64_t)carry;
    meta[kJoinM] = (int64_t)carry_n;
    meta[kJoinErr] = carry >= (uint64_t)kJoinMaxPairs ? 1 : 0;
  }
}

// Pass 3: per tile, every segment's exclusive offset and the plan rows of the matched ones, in
// segment order.
__global__ __launch_bounds__(kScanThreads) void join_tile_write_kernel(
    const uint64_t* __restrict__ cnt, const int64_t* __restrict__ match,
    const int64_t* __restrict__ lkeys, const int64_t* __restrict__ lheads, int64_t kl,
    const int64_t* __restrict__ rheads, int64_t kr, int64_t rtotal,
    const uint64_t* __restrict__ tsum, const uint32_t* __restrict__ tne,
    int64_t* __restrict__ pair_off, int64_t* __restrict__ plan) {
  __shared__ uint64_t ws[16];
  __shared__ uint32_t wn[16];
  __shared__ uint64_t tot;
  __shared__ uint32_t totn;
  const int64_t k0 = (int64_t)blockIdx.x * kJoinScanTile + (int64_t)threadIdx.x * kScanPer;
  uint64_t c[kScanPer];
  uint64_t s = 0;
  uint32_t ne = 0;
#pragma unroll
  for (int j = 0; j < kScanPer; ++j) {
    c[j] = k0 + j < kl ? cnt[k0 + j] : 0ull;
    s = join_sat_add(s, c[j]);
    ne += c[j] ? 1u : 0u;
  }
  uint64_t o = join_sat_add(tsum[blockIdx.x], block_excl_scan<uint64_t>(s, ws, &tot, SatAdd()));
  int64_t h = (int64_t)tne[blockIdx.x] + block_excl_scan<uint32_t>(ne, wn, &totn, Add32());
  const int64_t stride = kl + 1;
#pragma unroll
  for (int j = 0; j < kScanPer; ++j) {
    const int64_t i = k0 + j;
    if (i < kl) {
      pair_off[i] = (int64_t)o;
      if (c[j]) {
        const int64_t rj = match[i];
        plan[kJoinFirst * stride + h] = (int64_t)o;
        plan[kJoinKey * stride + h] = lkeys[i];
        plan[kJoinLs * stride + h] = lheads[i];
        plan[kJoinRs * stride + h] = rheads[rj];
        plan[kJoinNr * stride + h] = seg_len(rheads, kr, rtotal, rj);
        ++h;
      }
    }
    o = join_sat_add(o, c[j]);
  }
}

// ---- expand --------------------------------------------------------------------------------
typedef long long ll2 __attribute__((ext_vector_type(2)));

constexpr int kJoinStep = 2 * kJoinBlock;        // positions a workgroup covers per store round
constexpr int kJoinRounds = kJoinTile / kJoinStep;

// q = (a, b) advanced to a * nr + b + d (d < 2^31): one 32-bit division while everything fits.
__device__ __forceinline__ void join_divmod(uint64_t q, uint64_t nr, uint64_t* a, uint64_t* b) {
  if (((q | nr) >> 32) == 0) {
    *a = (uint32_t)q / (uint32_t)nr;
    *b = (uint32_t)q % (uint32_t)nr;
  } else {
    *a = q / nr;
    *b = q % nr;
  }
}

__global__ __launch_bounds__(kJoinBlock) void join_expand_kernel(
    const int64_t* __restrict__ plan, int64_t stride, int64_t m, const uint64_t* __restrict__ lord,
    const uint64_t* __restrict__ rord, int64_t p0, int64_t p1, int64_t ntiles,
    int64_t* __restrict__ out_key, int64_t* __restrict__ out_l, int64_t* __restrict__ out_r) {
  // rel[k]: the tile-relative first position of the tile's k-th segment (rel[0] = 0: the segment
  // that owns the tile's first position started at or before it), rel[ns] = the tile's length.
  __shared__ int32_t rel[kJoinTile + 1];
  const int64_t* __restrict__ first = plan + kJoinFirst * stride;
  const int64_t* __restrict__ pkey = plan + kJoinKey * stride;
  const int64_t* __restrict__ pls = plan + kJoinLs * stride;
  const int64_t* __restrict__ prs = plan + kJoinRs * stride;
  const int64_t* __restrict__ pnr = plan + kJoinNr * stride;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t tb = p0 + tile * kJoinTile;
    const int32_t len = (int32_t)(p1 - tb < kJoinTile ? p1 - tb : kJoinTile);
    const int64_t te = tb + len;
    // s0 = the last segment with first <= tb; s1 = the first segment after s0 with first >= te
    // (first[m] = P >= te). Both searches are uniform over the workgroup.
    int64_t lo = 0, hi = m;  // first[lo] <= tb < first[hi]
    int64_t lo2 = 0, hi2 = m;  // first[lo2] < te <= first[hi2]
    while (hi - lo > 1 || hi2 - lo2 > 1) {
      if (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (first[mid] <= tb) lo = mid; else hi = mid;
      }
      if (hi2 - lo2 > 1) {
        const int64_t mid = lo2 + ((hi2 - lo2) >> 1);
        if (first[mid] < te) lo2 = mid; else hi2 = mid;
      }
    }
    const int64_t s0 = lo;
    const int32_t ns = (int32_t)(hi2 - s0);  // 1 <= ns <= len: offsets strictly increase
    const int64_t qbase = tb - first[s0];    // pairs of segment s0 before the tile
    for (int32_t k = threadIdx.x; k <= ns; k += kJoinBlock)
      rel[k] = k == 0 ? 0 : (k == ns ? len : (int32_t)(first[s0 + k] - tb));
    __syncthreads();

    int32_t k = -1, nxt = 0;  // the lane's segment of the tile and the start of the next one
    int64_t key = 0, ls = 0, rs = 0;
    uint64_t nr = 1, a = 0, b = 0;
#pragma unroll 2
    for (int r = 0; r < kJoinRounds; ++r) {
      const int32_t pr = r * kJoinStep + 2 * (int32_t)threadIdx.x;
      if (pr >= len) break;
      if (pr >= nxt) {
        // another segment: the last k' > k with rel[k'] <= pr (rel[k + 1] = nxt <= pr < rel[ns])
        int32_t l2 = k + 1, h2 = ns;
        while (h2 - l2 > 1) {
          const int32_t mid = (l2 + h2) >> 1;
          if (rel[mid] <= pr) l2 = mid; else h2 = mid;
        }
        k = l2;
        nxt = rel[k + 1];
        key = pkey[s0 + k];
        ls = pls[s0 + k];
        rs = prs[s0 + k];
        nr = (uint64_t)pnr[s0 + k];
        const uint64_t q = (uint64_t)(pr - rel[k]) + (k == 0 ? (uint64_t)qbase : 0ull);
        join_divmod(q, nr, &a, &b);
      } else {
        // the same segment, kJoinStep positions on: carry (a, b) forward
        const uint64_t bb = b + kJoinStep;
        if (bb < nr) {
          b = bb;
        } else {
          uint64_t da, nb;
          join_divmod(bb, nr, &da, &nb);
          a += da;
          b = nb;
        }
      }
      ll2 vk, vl, vr;
      vk.x = key;
      vl.x = (int64_t)f64_from_order_bits(lord[ls + (int64_t)a]);
      vr.x = (int64_t)f64_from_order_bits(rord[rs + (int64_t)b]);
      const int64_t o = tb - p0 + pr;
      if (pr + 1 < len) {
        if (pr + 1 < nxt) {  // the next pair of the same segment
          const bool wrap = b + 1 == nr;
          vk.y = key;
          vl.y = wrap ? (int64_t)f64_from_order_bits(lord[ls + (int64_t)a + 1]) : vl.x;
          vr.y = (int64_t)f64_from_order_bits(rord[rs + (wrap ? 0 : (int64_t)b + 1)]);
        } else {  // the first pair of the next segment
          vk.y = pkey[s0 + k + 1];
          vl.y = (int64_t)f64_from_order_bits(lord[pls[s0 + k + 1]]);
          vr.y = (int64_t)f64_from_order_bits(rord[prs[s0 + k + 1]]);
        }
        *reinterpret_cast<ll2*>(out_key + o) = vk;
        *reinterpret_cast<ll2*>(out_l + o) = vl;
        *reinterpret_cast<ll2*>(out_r + o) = vr;
      } else {  // the odd last position of the range
        out_key[o] = vk.x;
        out_l[o] = vl.x;
        out_r[o] = vr.x;
      }
    }
    __syncthreads();  // rel is refilled for the workgroup's next tile
  }
}

}  // namespace

namespace gpu {

void join_match(const JoinSide& l, const JoinSide& r, int64_t* match, uint64_t* cnt,
                intptr_t stream) {
  if (l.nseg <= 0) return;
  hipLaunchKernelGGL(join_match_kernel, dim3(grid_of(l.nseg, 256, 2048)), dim3(256), 0,
                     (hipStream_t)stream, l.keys, l.heads, l.nseg, l.total, r.keys, r.heads,
                     r.nseg, r.total, match, cnt);
  JOIN_CHECK(hipGetLastError());
}

int64_t join_scan_scratch_bytes(int64_t kl) {
  const int64_t nt = (kl + kJoinScanTile - 1) / kJoinScanTile;
  return nt * (int64_t)(sizeof(uint64_t) + sizeof(uint32_t)) + 64;
}

void join_scan(const JoinSide& l, const JoinSide& r, const int64_t* match, const uint64_t* cnt,
               void* scratch, int64_t* pair_off, int64_t* plan, int64_t* meta, intptr_t stream) {
  const int64_t kl = l.nseg;
  if (kl < 0) throw std::invalid_argument("join_scan: negative segment count");
  const int64_t nt = (kl + kJoinScanTile - 1) / kJoinScanTile;
  if (nt > 0x7FFFFFFFll) throw std::invalid_argument("join_scan: too many segments");
  uint64_t* tsum = reinterpret_cast<uint64_t*>(scratch);
  uint32_t* tne = reinterpret_cast<uint32_t*>(tsum + nt);
  hipStream_t s = (hipStream_t)stream;
  if (nt)
    hipLaunchKernelGGL(join_tile_sums_kernel, dim3((unsigned)nt), dim3(kScanThreads), 0, s, cnt,
                       kl, tsum, tne);
  hipLaunchKernelGGL(join_tile_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, tsum, tne, nt, kl,
                     pair_off, plan, meta);
  if (nt)
    hipLaunchKernelGGL(join_tile_write_kernel, dim3((unsigned)nt), dim3(kScanThreads), 0, s, cnt,
                       match, l.keys, l.heads, kl, r.heads, r.nseg, r.total, tsum, tne, pair_off,
                       plan);
  JOIN_CHECK(hipGetLastError());
}

void join_expand(const int64_t* plan, int64_t kl, int64_t m, int64_t P, const uint64_t* lord,
                 const uint64_t* rord, int64_t p0, int64_t p1, int64_t* out_key, int64_t* out_l,
                 int64_t* out_r, intptr_t stream) {
  if (p0 < 0 || p1 < p0 || p1 > P || P >= kJoinMaxPairs)
    throw std::invalid_argument("join_expand: pair range outside [0, P)");
  if (m < 0 || m > kl || (P > 0 && m == 0))
    throw std::invalid_argument("join_expand: matched segment count out of range");
  if (((uintptr_t)out_key | (uintptr_t)out_l | (uintptr_t)out_r) & 15u)
    throw std::invalid_argument("join_expand: output columns must be 16-byte aligned");
  if (p0 == p1) return;
  const int64_t ntiles = (p1 - p0 + kJoinTile - 1) / kJoinTile;
  // 8 workgroups per CU are resident; a longer range strides over its tiles.
  hipLaunchKernelGGL(join_expand_kernel, dim3(grid_of(ntiles, 1, 2048)), dim3(kJoinBlock), 0,
                     (hipStream_t)stream, plan, kl + 1, m, lord, rord, p0, p1, ntiles, out_key,
                     out_l, out_r);
  JOIN_CHECK(hipGetLastError());
}

}  // namespace gpu
}  // namespace mxs
