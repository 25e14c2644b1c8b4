// mxstream — broadcast rule set on gfx950: test every sample against up to 64 rules and write one
// row per sample and rule that it breaks (declarations and layouts: csrc/mxs_ruleset.h; C++ twins:
// csrc/ruleset_cpu.cpp).
//
// The frame is the lookup's (csrc/lookup_hip.hip): a workgroup of 256 threads owns a tile of 4096
// samples, 16 per lane; round r of wave w is the tile's group 4 r + w. The rules are compacted
// once per workgroup into LDS, ascending by id; every lane reads the same entry (a broadcast) and
// the entry goes to scalar registers, so the comparison is chosen by a scalar branch outside the
// loop over a lane's samples. The count pass writes the groups' row sums, lookup_scan turns the
// tile counts into 64-bit offsets, the emit pass recomputes the masks and writes the rows: a wave
// lists its group's rows as (sample, rule id) pairs in LDS and then writes 64 consecutive rows per
// store (a lane that wrote its own rows one behind the other left every store instruction with
// 64 scattered 8-byte pieces: profiles/ruleset_broadcast.md). No atomics, no workgroup waits for
// another.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "mxs_hip_util.h"
#include "mxs_ruleset.h"

namespace mxs {
namespace {

constexpr int kRuleSetBlock = 256;
constexpr int kRuleSetWaves = kRuleSetBlock / 64;
constexpr int kRuleSetRounds = kLookupTile / kRuleSetBlock;  // samples per lane of a tile
constexpr int kRuleSetMaxGrid = 1 << 20;                     // longer inputs stride over tiles

struct RuleSetLds {
  int64_t thr[kRuleSetMax];    // compacted: threshold bits of the p-th active rule
  int32_t id[kRuleSetMax];     //            its id, ascending
  int32_t code[kRuleSetMax];   //            its comparison
  int64_t by_id[kRuleSetMax];  // threshold bits of rule id r (the emitted column)
  int32_t n;                   // active rules
};

// Wave 0 compacts the table: lane r holds row r, a ballot and a popcount give its place.
__device__ __forceinline__ void stage_rules(const ll2* __restrict__ rules, RuleSetLds& s) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    const ll2 row = rules[lane];
    const bool on = ruleset_active(row.y);
    const uint64_t b = __ballot(on);
    if (on) {
      const int p = __popcll(b & ((1ull << lane) - 1ull));
      s.thr[p] = row.x;
      s.id[p] = lane;
      s.code[p] = (int32_t)row.y;
    }
    s.by_id[lane] = row.x;
    if (lane == 0) s.n = __popcll(b);
  }
  __syncthreads();
}

template <int kWhen, int N>
__device__ __forceinline__ void apply_rule(const double (&v)[N], double t, uint64_t bit,
                                           uint64_t (&m)[N]) {
#pragma unroll
  for (int j = 0; j < N; ++j) m[j] |= lookup_cmp(kWhen, v[j], t) ? bit : 0ull;
}

// m[j] |= the rules that v[j] breaks. An LDS entry is the same for every lane: through
// readfirstlane it is a scalar, and the switch a scalar branch around N straight compares.
template <int N>
__device__ __forceinline__ void broken(const RuleSetLds& s, const double (&v)[N],
                                       uint64_t (&m)[N]) {
  const int nrules = __builtin_amdgcn_readfirstlane(s.n);
  for (int p = 0; p < nrules; ++p) {
    const int64_t tb = s.thr[p];
    const int lo = __builtin_amdgcn_readfirstlane((int)(uint32_t)tb);
    const int hi = __builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)tb >> 32));
    const double t = __hiloint2double(hi, lo);
    const uint64_t bit = 1ull << (__builtin_amdgcn_readfirstlane(s.id[p]) & 63);
    switch (__builtin_amdgcn_readfirstlane(s.code[p])) {
      case kLookupGt: apply_rule<kLookupGt>(v, t, bit, m); break;
      case kLookupGe: apply_rule<kLookupGe>(v, t, bit, m); break;
      case kLookupLt: apply_rule<kLookupLt>(v, t, bit, m); break;
      case kLookupLe: apply_rule<kLookupLe>(v, t, bit, m); break;
      case kLookupEq: apply_rule<kLookupEq>(v, t, bit, m); break;
      case kLookupNe: apply_rule<kLookupNe>(v, t, bit, m); break;
      default: break;
    }
  }
}

// What lanes of a wave wrote to LDS is read by other lanes of the same wave: a fence at wavefront
// scope on either side of a wave barrier (LDS operations of one wave complete in order).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- count ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kRuleSetBlock) void ruleset_count_kernel(
    const int64_t* __restrict__ vals, int64_t n, const ll2* __restrict__ rules, int64_t ntiles,
    uint32_t* __restrict__ gsum, uint32_t* __restrict__ counts) {
  __shared__ RuleSetLds s;
  __shared__ uint32_t wcount[kRuleSetWaves];
  stage_rules(rules, s);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t base = tile * kLookupTile + threadIdx.x;
    double v[kRuleSetRounds];
    uint64_t m[kRuleSetRounds];
#pragma unroll
    for (int r = 0; r < kRuleSetRounds; ++r) {
      const int64_t i = base + (int64_t)r * kRuleSetBlock;
      v[r] = i < n ? lookup_f64(vals[i]) : 0.0;
      m[r] = 0;
    }
    broken<kRuleSetRounds>(s, v, m);
    // Two rounds' row counts per word: a group has at most 64 * 64 = 4096 rows, 16 bits hold it.
    uint32_t pk[kRuleSetRounds / 2];
#pragma unroll
    for (int q = 0; q < kRuleSetRounds / 2; ++q) {
      uint32_t w = 0;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int r = 2 * q + h;
        const int64_t i = base + (int64_t)r * kRuleSetBlock;
        w |= (i < n ? (uint32_t)__popcll(m[r]) : 0u) << (16 * h);
      }
      for (int d = 32; d >= 1; d >>= 1) w += __shfl_xor(w, d);
      pk[q] = w;
    }
    if (lane == 0) {
      uint32_t c = 0;
#pragma unroll
      for (int r = 0; r < kRuleSetRounds; ++r) {
        const uint32_t g = (pk[r >> 1] >> (16 * (r & 1))) & 0xffffu;
        gsum[tile * kRuleSetGroups + r * kRuleSetWaves + wave] = g;
        c += g;
      }
      wcount[wave] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t c = 0;
      for (int w = 0; w < kRuleSetWaves; ++w) c += wcount[w];
      counts[tile] = c;
    }
    __syncthreads();  // wcount is rewritten for the workgroup's next tile
  }
}

// ---- emit ----------------------------------------------------------------------------------
__global__ __launch_bounds__(kRuleSetBlock) void ruleset_emit_kernel(
    const int64_t* __restrict__ keys, const int64_t* __restrict__ vals,
    const int64_t* __restrict__ ts, int64_t n, const ll2* __restrict__ rules, int64_t ntiles,
    const uint32_t* __restrict__ gsum, const uint32_t* __restrict__ counts,
    const int64_t* __restrict__ offsets, int64_t total, int64_t* __restrict__ out_key,
    int64_t* __restrict__ out_val, int64_t* __restrict__ out_rule, int64_t* __restrict__ out_thr,
    int64_t* __restrict__ out_ts) {
  __shared__ RuleSetLds s;
  __shared__ uint32_t gown[kRuleSetGroups];  // rows of the tile's group j
  __shared__ uint32_t gpre[kRuleSetGroups];  // rows of the tile's earlier groups
  __shared__ uint16_t stage[kRuleSetWaves][kLookupTile];  // a wave's group: (sample, rule) per row
  stage_rules(rules, s);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    if (counts[tile] == 0) continue;  // uniform over the workgroup
    if (wave == 0) {
      const uint32_t own = gsum[tile * kRuleSetGroups + lane];
      uint32_t incl = own;
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(incl, d);
        if (lane >= d) incl += y;
      }
      gown[lane] = own;
      gpre[lane] = incl - own;
    }
    __syncthreads();
    const int64_t off = offsets[tile];
    const int64_t base = tile * kLookupTile + threadIdx.x;
    for (int r = 0; r < kRuleSetRounds; ++r) {
      const int j = r * kRuleSetWaves + wave;
      if (__builtin_amdgcn_readfirstlane(gown[j]) == 0) continue;  // uniform over the wave
      const int64_t i = base + (int64_t)r * kRuleSetBlock;
      const int64_t vb = i < n ? vals[i] : 0;
      const double v[1] = {lookup_f64(vb)};
      uint64_t m[1] = {0};
      broken<1>(s, v, m);
      uint64_t mine = i < n ? m[0] : 0ull;
      const uint32_t own = (uint32_t)__popcll(mine);
      uint32_t incl = own;
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(incl, d);
        if (lane >= d) incl += y;
      }
      // The group's rows as (sample, rule id) pairs in LDS, in row order: every lane lists its
      // own set bits behind the rows of the lanes before it ...
      uint16_t* rows = stage[wave];
      uint32_t slot = incl - own;  // < 4096: a group has at most 64 * 64 rows
      for (; mine != 0; mine &= mine - 1, ++slot)
        rows[slot] = (uint16_t)((lane << 6) | (__ffsll((unsigned long long)mine) - 1));
      wave_lds_sync();
      // ... then lane q writes row q, q + 64, ..: five stores of 64 consecutive rows each.
      const uint32_t nrows = __shfl(incl, 63);
      const int64_t first = off + gpre[j];
      const int64_t i0 = i - lane;
      for (uint32_t q = lane; q < nrows && first + q < total; q += 64) {
        const uint32_t c = rows[q];
        const int64_t src = i0 + (c >> 6), pos = first + q;
        if (src >= n) continue;  // (never: that sample has a row)
        const int id = c & 63;
        out_key[pos] = keys[src];
        out_val[pos] = vals[src];
        out_rule[pos] = id;
        out_thr[pos] = s.by_id[id];
        out_ts[pos] = ts[src];
      }
      wave_lds_sync();  // `rows` is rewritten in the wave's next round
    }
    __syncthreads();  // gown / gpre are refilled for the workgroup's next tile
  }
}

void check_rules(const int64_t* rules, const char* what) {
  if (rules == nullptr || ((uintptr_t)rules & 15u))
    throw std::invalid_argument(std::string(what) + ": the rule table must be 16-byte aligned");
}

}  // namespace

namespace gpu {

void ruleset_count(const int64_t* vals, int64_t n, const int64_t* rules, uint32_t* gsum,
                   uint32_t* counts, intptr_t stream) {
  check_rules(rules, "ruleset_count");
  if (n < 0) throw std::invalid_argument("ruleset_count: negative row count");
  if (n == 0) return;
  const int64_t ntiles = (n + kLookupTile - 1) / kLookupTile;
  hipLaunchKernelGGL(ruleset_count_kernel, dim3(grid_of(ntiles, 1, kRuleSetMaxGrid)),
                     dim3(kRuleSetBlock), 0, (hipStream_t)stream, vals, n,
                     reinterpret_cast<const ll2*>(rules), ntiles, gsum, counts);
  MXS_HIP_CHECK(hipGetLastError());
}

// `gsum`, `counts` and `offsets` must be ruleset_count's and lookup_scan's output for these same
// values and rules and `total` the scan's total: a row past `total` is never written.
void ruleset_emit(const int64_t* keys, const int64_t* vals, const int64_t* ts, int64_t n,
                  const int64_t* rules, const uint32_t* gsum, const uint32_t* counts,
                  const int64_t* offsets, int64_t total, int64_t* out_key, int64_t* out_val,
                  int64_t* out_rule, int64_t* out_thr, int64_t* out_ts, intptr_t stream) {
  check_rules(rules, "ruleset_emit");
  if (n < 0 || total < 0 || (n < (INT64_MAX >> 6) && total > n * kRuleSetMax))
    throw std::invalid_argument("ruleset_emit: bad row counts");
  if (n == 0 || total == 0) return;
  const int64_t ntiles = (n + kLookupTile - 1) / kLookupTile;
  hipLaunchKernelGGL(ruleset_emit_kernel, dim3(grid_of(ntiles, 1, kRuleSetMaxGrid)),
                     dim3(kRuleSetBlock), 0, (hipStream_t)stream, keys, vals, ts, n,
                     reinterpret_cast<const ll2*>(rules), ntiles, gsum, counts, offsets, total,
                     out_key, out_val, out_rule, out_thr, out_ts);
  MXS_HIP_CHECK(hipGetLastError());
}

}  // namespace gpu
}  // namespace mxs
