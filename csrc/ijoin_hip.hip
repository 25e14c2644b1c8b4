// mxstream — keyed interval joins on gfx950: probe the other side's sorted buffer with a sorted
// batch, scan the pair counts, expand the pairs, merge the batch into its own buffer
// (declarations and layouts: csrc/mxs_ijoin.h; C++ twins: csrc/ijoin_cpu.cpp).
//
// The expand is the window join's (csrc/join_hip.hip) with single probing elements as segments:
// a workgroup owns kJoinTile consecutive output positions, finds the plan rows that overlap them
// by two uniform binary searches in the (strictly increasing) first-pair column and keeps their
// tile-relative starts in LDS. Inside a plan row the other side's rows are consecutive, so a
// position needs one subtraction, no division. Every lane writes two consecutive positions per
// column with one 16-byte store. No atomics and no device counter.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "mxs_ijoin.h"
#include "mxs_blockscan.h"

namespace mxs {
namespace {

#define IJOIN_CHECK(x)                                                                      \
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

// ---- scan (the window join's three passes over single elements) ------------------------------
constexpr int kScanThreads = 1024;
constexpr int kScanPer = kJoinScanTile / kScanThreads;  // 4 elements per thread

__device__ __forceinline__ uint64_t clamp_cnt(uint64_t c) {
  return c > (uint64_t)kJoinMaxPairs ? (uint64_t)kJoinMaxPairs : c;
}

// Pass 1: per tile, the pair total and the number of non-empty elements.
__global__ __launch_bounds__(kScanThreads) void ijoin_tile_sums_kernel(
    const uint64_t* __restrict__ cnt, int64_t n, uint64_t* __restrict__ tsum,
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
    const uint64_t c = k0 + j < n ? clamp_cnt(cnt[k0 + j]) : 0ull;
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
// carry; the totals P, m and the error word.
__global__ __launch_bounds__(kScanThreads) void ijoin_tile_scan_kernel(
    uint64_t* __restrict__ tsum, uint32_t* __restrict__ tne, int64_t ntiles, int64_t n,
    int64_t* __restrict__ plan, int64_t* __restrict__ meta) {
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
    plan[(int64_t)kIJoinFirst * (n + 1) + carry_n] = (int64_t)carry;
    meta[0] = (int64_t)carry;
    meta[1] = (int64_t)carry_n;
    meta[2] = carry >= (uint64_t)kJoinMaxPairs ? 1 : 0;
    meta[3] = 0;
  }
}

// Pass 3: per tile, the plan rows of the non-empty elements, in element order.
__global__ __launch_bounds__(kScanThreads) void ijoin_tile_write_kernel(
    const uint64_t* __restrict__ cnt, const int64_t* __restrict__ lb, int64_t n,
    const uint64_t* __restrict__ tsum, const uint32_t* __restrict__ tne,
    int64_t* __restrict__ plan) {
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
    c[j] = k0 + j < n ? clamp_cnt(cnt[k0 + j]) : 0ull;
    s = join_sat_add(s, c[j]);
    ne += c[j] ? 1u : 0u;
  }
  uint64_t o = join_sat_add(tsum[blockIdx.x], block_excl_scan<uint64_t>(s, ws, &tot, SatAdd()));
  int64_t h = (int64_t)tne[blockIdx.x] + block_excl_scan<uint32_t>(ne, wn, &totn, Add32());
  const int64_t stride = n + 1;
#pragma unroll
  for (int j = 0; j < kScanPer; ++j) {
    const int64_t i = k0 + j;
    if (i < n && c[j]) {
      plan[kIJoinFirst * stride + h] = (int64_t)o;
      plan[kIJoinIdx * stride + h] = i;
      plan[kIJoinLb * stride + h] = lb[i];
      ++h;
    }
    o = join_sat_add(o, c[j]);
  }
}

// ---- expand --------------------------------------------------------------------------------
typedef long long ll2 __attribute__((ext_vector_type(2)));

constexpr int kIJoinStep = 2 * kJoinBlock;  // positions a workgroup covers per store round
constexpr int kIJoinRounds = kJoinTile / kIJoinStep;

// kLeft: the batch is the left side (its value goes to out_l).
template <bool kLeft>
__global__ __launch_bounds__(kJoinBlock) void ijoin_expand_kernel(
    const int64_t* __restrict__ plan, int64_t stride, int64_t m, const int64_t* __restrict__ bkey,
    const int64_t* __restrict__ bts, const int64_t* __restrict__ bval,
    const int64_t* __restrict__ ots, const int64_t* __restrict__ oval, int64_t p0, int64_t p1,
    int64_t ntiles, int64_t* __restrict__ out_key, int64_t* __restrict__ out_l,
    int64_t* __restrict__ out_r, int64_t* __restrict__ out_ts) {
  // rel[k]: the tile-relative first position of the tile's k-th plan row (rel[0] = 0: the row
  // that owns the tile's first position started at or before it), rel[ns] = the tile's length.
  __shared__ int32_t rel[kJoinTile + 1];
  const int64_t* __restrict__ first = plan + kIJoinFirst * stride;
  const int64_t* __restrict__ pidx = plan + kIJoinIdx * stride;
  const int64_t* __restrict__ plb = plan + kIJoinLb * stride;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t tb = p0 + tile * kJoinTile;
    const int32_t len = (int32_t)(p1 - tb < kJoinTile ? p1 - tb : kJoinTile);
    const int64_t te = tb + len;
    // s0 = the last row with first <= tb; the tile's rows end before the first row with
    // first >= te (first[m] = P >= te). Both searches are uniform over the workgroup.
    int64_t lo = 0, hi = m;    // first[lo] <= tb < first[hi]
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
    const int64_t qbase = tb - first[s0];    // pairs of row s0 before the tile
    for (int32_t k = threadIdx.x; k <= ns; k += kJoinBlock)
      rel[k] = k == 0 ? 0 : (k == ns ? len : (int32_t)(first[s0 + k] - tb));
    __syncthreads();

    int32_t k = -1, nxt = 0;  // the lane's plan row of the tile and the start of the next one
    int64_t key = 0, bt = 0, bv = 0, o = 0;
#pragma unroll 2
    for (int r = 0; r < kIJoinRounds; ++r) {
      const int32_t pr = r * kIJoinStep + 2 * (int32_t)threadIdx.x;
      if (pr >= len) break;
      if (pr >= nxt) {
        // another row: the last k' > k with rel[k'] <= pr (rel[k + 1] = nxt <= pr < rel[ns])
        int32_t l2 = k + 1, h2 = ns;
        while (h2 - l2 > 1) {
          const int32_t mid = (l2 + h2) >> 1;
          if (rel[mid] <= pr) l2 = mid; else h2 = mid;
        }
        k = l2;
        nxt = rel[k + 1];
        const int64_t i = pidx[s0 + k];
        key = bkey[i];
        bt = bts[i];
        bv = bval[i];
        o = plb[s0 + k] + (int64_t)(pr - rel[k]) + (k == 0 ? qbase : 0);
      } else {
        o += kIJoinStep;  // the same row, kIJoinStep positions on
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
  IJOIN_CHECK(hipGetLastError());
}

int64_t ijoin_scan_scratch_bytes(int64_t n) {
  const int64_t nt = (n + kJoinScanTile - 1) / kJoinScanTile;
  return nt * (int64_t)(sizeof(uint64_t) + sizeof(uint32_t)) + 64;
}

void ijoin_scan(const uint64_t* cnt, const int64_t* lb, int64_t n, void* scratch, int64_t* plan,
                int64_t* meta, intptr_t stream) {
  if (n < 0) throw std::invalid_argument("ijoin_scan: negative element count");
  const int64_t nt = (n + kJoinScanTile - 1) / kJoinScanTile;
  if (nt > 0x7FFFFFFFll) throw std::invalid_argument("ijoin_scan: too many elements");
  uint64_t* tsum = reinterpret_cast<uint64_t*>(scratch);
  uint32_t* tne = reinterpret_cast<uint32_t*>(tsum + nt);
  hipStream_t s = (hipStream_t)stream;
  if (nt)
    hipLaunchKernelGGL(ijoin_tile_sums_kernel, dim3((unsigned)nt), dim3(kScanThreads), 0, s, cnt,
                       n, tsum, tne);
  hipLaunchKernelGGL(ijoin_tile_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, tsum, tne, nt, n,
                     plan, meta);
  if (nt)
    hipLaunchKernelGGL(ijoin_tile_write_kernel, dim3((unsigned)nt), dim3(kScanThreads), 0, s, cnt,
                       lb, n, tsum, tne, plan);
  IJOIN_CHECK(hipGetLastError());
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
  IJOIN_CHECK(hipGetLastError());
}

void ijoin_merge(const IJoinCols& old, const IJoinCols& batch, int64_t* out_key, int64_t* out_ts,
                 int64_t* out_val, intptr_t stream) {
  if (old.n < 0 || batch.n < 0) throw std::invalid_argument("ijoin_merge: negative row count");
  if (old.n + batch.n == 0) return;
  hipLaunchKernelGGL(ijoin_merge_kernel, dim3(grid_of(old.n + batch.n, 256, 8192)), dim3(256), 0,
                     (hipStream_t)stream, old.key, old.ts, old.val, old.n, batch.key, batch.ts,
                     batch.val, batch.n, out_key, out_ts, out_val);
  IJOIN_CHECK(hipGetLastError());
}

void ijoin_keep(const int64_t* ts, int64_t n, int64_t cutoff, uint64_t* cnt, intptr_t stream) {
  if (n <= 0) return;
  hipLaunchKernelGGL(ijoin_keep_kernel, dim3(grid_of(n, 256, 8192)), dim3(256), 0,
                     (hipStream_t)stream, ts, n, cutoff, cnt);
  IJOIN_CHECK(hipGetLastError());
}

void ijoin_gather(const int64_t* plan, int64_t n, int64_t m, const IJoinCols& src,
                  int64_t* out_key, int64_t* out_ts, int64_t* out_val, intptr_t stream) {
  if (m < 0 || m > n || n != src.n)
    throw std::invalid_argument("ijoin_gather: survivor count out of range");
  if (m == 0) return;
  hipLaunchKernelGGL(ijoin_gather_kernel, dim3(grid_of(m, 256, 8192)), dim3(256), 0,
                     (hipStream_t)stream, plan + (int64_t)kIJoinIdx * (n + 1), m, src.key, src.ts,
                     src.val, out_key, out_ts, out_val);
  IJOIN_CHECK(hipGetLastError());
}

}  // namespace gpu
}  // namespace mxs
