// mxstream — keyed window joins on gfx950: match the two sides' key segments, scan the pair
// counts, expand every matched key's nL x nR pairs (declarations and the layout of the plan:
// csrc/mxs_join.h; C++ twins: csrc/join_cpu.cpp).
//
// The expand is output-centric: a workgroup owns kJoinTile consecutive output positions, finds
// the matched segments that overlap them by two binary searches in the plan's (strictly
// increasing) first-pair column and keeps their tile-relative starts in LDS (the tile frame,
// csrc/pair_expand.h, which the interval join's expand shares). A hot key's millions of pairs
// are thus spread over as many workgroups as it has tiles, and thousands of small keys share
// one. Every lane writes two consecutive positions per column with one 16-byte store; a wave
// covers 128 consecutive positions (1 KiB per column and store). No atomics and no device
// counter: every position is known from the scan.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "mxs_hip_util.h"
#include "mxs_join.h"
#include "pair_expand.h"
#include "pair_scan.h"

namespace mxs {
namespace {

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

// ---- scan (csrc/pair_scan.h over the left segments: 64-bit, saturating) -----------------------
struct JoinScan {
  using Add = SatAdd;
  const uint64_t* cnt;
  const int64_t *match, *lkeys, *lheads;
  int64_t kl;
  const int64_t* rheads;
  int64_t kr, rtotal;
  int64_t *pair_off, *plan, *meta;

  __device__ __forceinline__ uint64_t count(int64_t i) const { return cnt[i]; }
  __device__ __forceinline__ void element(int64_t i, uint64_t o) const {
    pair_off[i] = (int64_t)o;
  }
  // the plan row of matched segment i
  __device__ __forceinline__ void nonempty(int64_t i, int64_t h, uint64_t o) const {
    const int64_t stride = kl + 1, rj = match[i];
    plan[kJoinFirst * stride + h] = (int64_t)o;
    plan[kJoinKey * stride + h] = lkeys[i];
    plan[kJoinLs * stride + h] = lheads[i];
    plan[kJoinRs * stride + h] = rheads[rj];
    plan[kJoinNr * stride + h] = seg_len(rheads, kr, rtotal, rj);
  }
  // the totals P, m and the error word
  __device__ __forceinline__ void finish(uint64_t P, uint32_t m) const {
    pair_off[kl] = (int64_t)P;
    plan[(int64_t)kJoinFirst * (kl + 1) + m] = (int64_t)P;
    meta[kJoinP] = (int64_t)P;
    meta[kJoinM] = (int64_t)m;
    meta[kJoinErr] = P >= (uint64_t)kJoinMaxPairs ? 1 : 0;
  }
};

// ---- expand --------------------------------------------------------------------------------
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
  __shared__ int32_t rel[kJoinTile + 1];  // the tile's segment starts (pair_tile_begin)
  const int64_t* __restrict__ first = plan + kJoinFirst * stride;
  const int64_t* __restrict__ pkey = plan + kJoinKey * stride;
  const int64_t* __restrict__ pls = plan + kJoinLs * stride;
  const int64_t* __restrict__ prs = plan + kJoinRs * stride;
  const int64_t* __restrict__ pnr = plan + kJoinNr * stride;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const PairTile t = pair_tile_begin(first, m, p0, p1, tile, rel);
    const int64_t tb = t.tb, s0 = t.s0;
    const int32_t len = t.len;

    int32_t k = -1, nxt = 0;  // the lane's segment of the tile and the start of the next one
    int64_t key = 0, ls = 0, rs = 0;
    uint64_t nr = 1, a = 0, b = 0;
#pragma unroll 2
    for (int r = 0; r < kPairRounds; ++r) {
      const int32_t pr = r * kPairStep + 2 * (int32_t)threadIdx.x;
      if (pr >= len) break;
      if (pr >= nxt) {
        k = pair_lane_row(rel, k, t.ns, pr);  // another segment
        nxt = rel[k + 1];
        key = pkey[s0 + k];
        ls = pls[s0 + k];
        rs = prs[s0 + k];
        nr = (uint64_t)pnr[s0 + k];
        const uint64_t q = (uint64_t)(pr - rel[k]) + (k == 0 ? (uint64_t)t.qbase : 0ull);
        join_divmod(q, nr, &a, &b);
      } else {
        // the same segment, kPairStep positions on: carry (a, b) forward
        const uint64_t bb = b + kPairStep;
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
  MXS_HIP_CHECK(hipGetLastError());
}

int64_t join_scan_scratch_bytes(int64_t kl) { return pair_scan_scratch_bytes(kl); }

void join_scan(const JoinSide& l, const JoinSide& r, const int64_t* match, const uint64_t* cnt,
               void* scratch, int64_t* pair_off, int64_t* plan, int64_t* meta, intptr_t stream) {
  const int64_t kl = l.nseg;
  if (kl < 0) throw std::invalid_argument("join_scan: negative segment count");
  const int64_t nt = (kl + kJoinScanTile - 1) / kJoinScanTile;
  if (nt > 0x7FFFFFFFll) throw std::invalid_argument("join_scan: too many segments");
  const JoinScan p = {cnt, match, l.keys, l.heads, kl, r.heads, r.nseg, r.total,
                      pair_off, plan, meta};
  pair_scan_launch(p, kl, scratch, (hipStream_t)stream);
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
  MXS_HIP_CHECK(hipGetLastError());
}

}  // namespace gpu
}  // namespace mxs
