// mxstream — keyed interval joins on gfx950: probe the other side's sorted buffer with a sorted
// batch, scan the pair counts, expand the pairs, merge the batch into its own buffer
// (declarations and layouts: csrc/mxs_ijoin.h; C++ twins: csrc/ijoin_cpu.cpp).
//
// The scan is the window join's (csrc/pair_scan.h) and so is the expand's tile frame
// (csrc/pair_expand.h), with single probing elements as segments. Inside a plan row the other
// side's rows are consecutive, so a position needs one subtraction, no division. Every lane
// writes two consecutive positions per column with one 16-byte store. No atomics and no device
// counter.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "mxs_hip_util.h"
#include "mxs_ijoin.h"
#include "pair_expand.h"
#include "pair_scan.h"

namespace mxs {
namespace {

// ---- probe ---------------------------------------------------------------------------------
// The batch is sorted, so neighbouring lanes search neighbouring places of the other buffer.
__global__ __launch_bounds__(256) void ijoin_probe_kernel(
    const int64_t* __restrict__ bkey, const int64_t* __restrict__ bts, int64_t nb,
    const int64_t* __restrict__ okey, const int64_t* __restrict__ ots, int64_t no, int64_t rlo,
    int64_t rhi, int64_t cutoff, int64_t* __restrict__ lb, uint64_t* __restrict__ cnt) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nb;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t l;
    uint64_t c;
    ijoin_range(okey, ots, no, bkey[i], bts[i], rlo, rhi, cutoff, &l, &c);
    lb[i] = l;
    cnt[i] = c;
  }
}

// ---- scan (csrc/pair_scan.h over single elements, their counts clamped) -----------------------
struct IJoinScan {
  using Add = SatAdd;
  const uint64_t* cnt;
  const int64_t* lb;
  int64_t n;
  int64_t *plan, *meta;

  __device__ __forceinline__ uint64_t count(int64_t i) const {
    const uint64_t c = cnt[i];
    return c > (uint64_t)kJoinMaxPairs ? (uint64_t)kJoinMaxPairs : c;
  }
  __device__ __forceinline__ void element(int64_t, uint64_t) const {}
  // the plan row of non-empty element i
  __device__ __forceinline__ void nonempty(int64_t i, int64_t h, uint64_t o) const {
    const int64_t stride = n + 1;
    plan[kIJoinFirst * stride + h] = (int64_t)o;
    plan[kIJoinIdx * stride + h] = i;
    plan[kIJoinLb * stride + h] = lb[i];
  }
  // the totals P, m and the error word
  __device__ __forceinline__ void finish(uint64_t P, uint32_t m) const {
    plan[(int64_t)kIJoinFirst * (n + 1) + m] = (int64_t)P;
    meta[0] = (int64_t)P;
    meta[1] = (int64_t)m;
    meta[2] = P >= (uint64_t)kJoinMaxPairs ? 1 : 0;
    meta[3] = 0;
  }
};

// ---- expand --------------------------------------------------------------------------------
// kLeft: the batch is the left side (its value goes to out_l).
template <bool kLeft>
__global__ __launch_bounds__(kJoinBlock) void ijoin_expand_kernel(
    const int64_t* __restrict__ plan, int64_t stride, int64_t m, const int64_t* __restrict__ bkey,
    const int64_t* __restrict__ bts, const int64_t* __restrict__ bval,
    const int64_t* __restrict__ ots, const int64_t* __restrict__ oval, int64_t p0, int64_t p1,
    int64_t ntiles, int64_t* __restrict__ out_key, int64_t* __restrict__ out_l,
    int64_t* __restrict__ out_r, int64_t* __restrict__ out_ts) {
  __shared__ int32_t rel[kJoinTile + 1];  // the tile's plan row starts (pair_tile_begin)
  const int64_t* __restrict__ first = plan + kIJoinFirst * stride;
  const int64_t* __restrict__ pidx = plan + kIJoinIdx * stride;
  const int64_t* __restrict__ plb = plan + kIJoinLb * stride;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const PairTile t = pair_tile_begin(first, m, p0, p1, tile, rel);
    const int64_t tb = t.tb, s0 = t.s0;
    const int32_t len = t.len;

    int32_t k = -1, nxt = 0;  // the lane's plan row of the tile and the start of the next one
    int64_t key = 0, bt = 0, bv = 0, o = 0;
#pragma unroll 2
    for (int r = 0; r < kPairRounds; ++r) {
      const int32_t pr = r * kPairStep + 2 * (int32_t)threadIdx.x;
      if (pr >= len) break;
      if (pr >= nxt) {
        k = pair_lane_row(rel, k, t.ns, pr);  // another row
        nxt = rel[k + 1];
        const int64_t i = pidx[s0 + k];
        key = bkey[i];
        bt = bts[i];
        bv = bval[i];
        o = plb[s0 + k] + (int64_t)(pr - rel[k]) + (k == 0 ? t.qbase : 0);
      } else {
        o += kPairStep;  // the same row, kPairStep positions on
      }
      ll2 vk, vb, vo, vt;
      int64_t t = ots[o];
      vk.x = key;
      vb.x = bv;
      vo.x = oval[o];
      vt.x = bt > t ? bt : t;
      const int64_t w = tb - p0 + pr;
      if (pr + 1 < len) {
        if (pr + 1 < nxt) {  // the next pair of the same row
          t = ots[o + 1];
          vk.y = key;
          vb.y = bv;
          vo.y = oval[o + 1];
          vt.y = bt > t ? bt : t;
        } else {  // the first pair of the next row
          const int64_t i = pidx[s0 + k + 1], o2 = plb[s0 + k + 1];
          const int64_t bt2 = bts[i];
          t = ots[o2];
          vk.y = bkey[i];
          vb.y = bval[i];
          vo.y = oval[o2];
          vt.y = bt2 > t ? bt2 : t;
        }
        *reinterpret_cast<ll2*>(out_key + w) = vk;
        *reinterpret_cast<ll2*>(out_l + w) = kLeft ? vb : vo;
        *reinterpret_cast<ll2*>(out_r + w) = kLeft ? vo : vb;
        *reinterpret_cast<ll2*>(out_ts + w) = vt;
      } else {  // the odd last position of the range
        out_key[w] = vk.x;
        out_l[w] = kLeft ? vb.x : vo.x;
        out_r[w] = kLeft ? vo.x : vb.x;
        out_ts[w] = vt.x;
      }
    }
    __syncthreads();  // rel is refilled for the workgroup's next tile
  }
}

// ---- merge ---------------------------------------------------------------------------------
// Thread g < no moves old row g, thread g >= no batch row g - no; the two rank rules give every
// row of the union its own position (old rows first on ties).
__global__ __launch_bounds__(256) void ijoin_merge_kernel(
    const int64_t* __restrict__ okey, const int64_t* __restrict__ ots,
    const int64_t* __restrict__ oval, int64_t no, const int64_t* __restrict__ bkey,
    const int64_t* __restrict__ bts, const int64_t* __restrict__ bval, int64_t nb,
    int64_t* __restrict__ out_key, int64_t* __restrict__ out_ts, int64_t* __restrict__ out_val) {
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < no + nb;
       g += (int64_t)gridDim.x * blockDim.x) {
    int64_t k, t, v, d;
    if (g < no) {
      k = okey[g], t = ots[g], v = oval[g];
      d = g + ijoin_lower(bkey, bts, nb, k, t);
    } else {
      const int64_t i = g - no;
      k = bkey[i], t = bts[i], v = bval[i];
      d = i + ijoin_upper(okey, ots, no, k, t);
    }
    out_key[d] = k;
    out_ts[d] = t;
    out_val[d] = v;
  }
}

// ---- purge ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ijoin_keep_kernel(const int64_t* __restrict__ ts, int64_t n,
                                                         int64_t cutoff,
                                                         uint64_t* __restrict__ cnt) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    cnt[i] = ts[i] > cutoff ? 1ull : 0ull;
}

__global__ __launch_bounds__(256) void ijoin_gather_kernel(
    const int64_t* __restrict__ pidx, int64_t m, const int64_t* __restrict__ skey,
    const int64_t* __restrict__ sts, const int64_t* __restrict__ sval,
    int64_t* __restrict__ out_key, int64_t* __restrict__ out_ts, int64_t* __restrict__ out_val) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m;
       j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = pidx[j];
    out_key[j] = skey[i];
    out_ts[j] = sts[i];
    out_val[j] = sval[i];
  }
}

}  // namespace

namespace gpu {

void ijoin_probe(const IJoinCols& batch, const IJoinCols& other, int64_t rlo, int64_t rhi,
                 int64_t cutoff, int64_t* lb, uint64_t* cnt, intptr_t stream) {
  if (batch.n <= 0) return;
  hipLaunchKernelGGL(ijoin_probe_kernel, dim3(grid_of(batch.n, 256, 4096)), dim3(256), 0,
                     (hipStream_t)stream, batch.key, batch.ts, batch.n, other.key, other.ts,
                     other.n, rlo, rhi, cutoff, lb, cnt);
  MXS_HIP_CHECK(hipGetLastError());
}

int64_t ijoin_scan_scratch_bytes(int64_t n) { return pair_scan_scratch_bytes(n); }

void ijoin_scan(const uint64_t* cnt, const int64_t* lb, int64_t n, void* scratch, int64_t* plan,
                int64_t* meta, intptr_t stream) {
  if (n < 0) throw std::invalid_argument("ijoin_scan: negative element count");
  const int64_t nt = (n + kJoinScanTile - 1) / kJoinScanTile;
  if (nt > 0x7FFFFFFFll) throw std::invalid_argument("ijoin_scan: too many elements");
  const IJoinScan p = {cnt, lb, n, plan, meta};
  pair_scan_launch(p, n, scratch, (hipStream_t)stream);
}

// `plan` must be ijoin_scan's output for ijoin_probe's (lb, cnt) of this very `batch` against
// this very `other`: the kernel reads other rows lb[j] .. lb[j] + cnt - 1 and batch rows idx[j]
// as the plan names them. The range, the row count and the alignment are checked here; that the
// plan's rows lie inside the two buffers cannot be checked on the host and is the caller's to
// keep (ops/kernels.py holds plan and buffers together in one IJoinPlan).
void ijoin_expand(const int64_t* plan, int64_t n, int64_t m, int64_t P, const IJoinCols& batch,
                  const IJoinCols& other, int side, int64_t p0, int64_t p1, int64_t* out_key,
                  int64_t* out_l, int64_t* out_r, int64_t* out_ts, intptr_t stream) {
  if (p0 < 0 || p1 < p0 || p1 > P || P >= kJoinMaxPairs)
    throw std::invalid_argument("ijoin_expand: pair range outside [0, P)");
  if (m < 0 || m > n || n != batch.n || (P > 0 && m == 0))
    throw std::invalid_argument("ijoin_expand: plan row count out of range");
  if (P > 0 && other.n <= 0) throw std::invalid_argument("ijoin_expand: pairs of an empty buffer");
  if (side != 0 && side != 1) throw std::invalid_argument("ijoin_expand: side must be 0 or 1");
  if (((uintptr_t)out_key | (uintptr_t)out_l | (uintptr_t)out_r | (uintptr_t)out_ts) & 15u)
    throw std::invalid_argument("ijoin_expand: output columns must be 16-byte aligned");
  if (p0 == p1) return;
  const int64_t ntiles = (p1 - p0 + kJoinTile - 1) / kJoinTile;
  // 8 workgroups per CU are resident; a longer range strides over its tiles.
  const dim3 grid(grid_of(ntiles, 1, 2048));
  hipStream_t s = (hipStream_t)stream;
  if (side == 0)
    hipLaunchKernelGGL(ijoin_expand_kernel<true>, grid, dim3(kJoinBlock), 0, s, plan, n + 1, m,
                       batch.key, batch.ts, batch.val, other.ts, other.val, p0, p1, ntiles,
                       out_key, out_l, out_r, out_ts);
  else
    hipLaunchKernelGGL(ijoin_expand_kernel<false>, grid, dim3(kJoinBlock), 0, s, plan, n + 1, m,
                       batch.key, batch.ts, batch.val, other.ts, other.val, p0, p1, ntiles,
                       out_key, out_l, out_r, out_ts);
  MXS_HIP_CHECK(hipGetLastError());
}

void ijoin_merge(const IJoinCols& old, const IJoinCols& batch, int64_t* out_key, int64_t* out_ts,
                 int64_t* out_val, intptr_t stream) {
  if (old.n < 0 || batch.n < 0) throw std::invalid_argument("ijoin_merge: negative row count");
  if (old.n + batch.n == 0) return;
  hipLaunchKernelGGL(ijoin_merge_kernel, dim3(grid_of(old.n + batch.n, 256, 8192)), dim3(256), 0,
                     (hipStream_t)stream, old.key, old.ts, old.val, old.n, batch.key, batch.ts,
                     batch.val, batch.n, out_key, out_ts, out_val);
  MXS_HIP_CHECK(hipGetLastError());
}

void ijoin_keep(const int64_t* ts, int64_t n, int64_t cutoff, uint64_t* cnt, intptr_t stream) {
  if (n <= 0) return;
  hipLaunchKernelGGL(ijoin_keep_kernel, dim3(grid_of(n, 256, 8192)), dim3(256), 0,
                     (hipStream_t)stream, ts, n, cutoff, cnt);
  MXS_HIP_CHECK(hipGetLastError());
}

void ijoin_gather(const int64_t* plan, int64_t n, int64_t m, const IJoinCols& src,
                  int64_t* out_key, int64_t* out_ts, int64_t* out_val, intptr_t stream) {
  if (m < 0 || m > n || n != src.n)
    throw std::invalid_argument("ijoin_gather: survivor count out of range");
  if (m == 0) return;
  hipLaunchKernelGGL(ijoin_gather_kernel, dim3(grid_of(m, 256, 8192)), dim3(256), 0,
                     (hipStream_t)stream, plan + (int64_t)kIJoinIdx * (n + 1), m, src.key, src.ts,
                     src.val, out_key, out_ts, out_val);
  MXS_HIP_CHECK(hipGetLastError());
}

}  // namespace gpu
}  // namespace mxs
