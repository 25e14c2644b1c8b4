// mxstream — burst alerts on gfx950: N breaches within T per key, as a bounded look-back into
// the key's breach history followed by a segmented wave scan (declarations, the model and the
// summary algebra: csrc/mxs_burst.h; C++ twin: csrc/burst_cpu.cpp).
//
// scan: the batch arrives stably sorted by key and is scanned in the frame of csrc/rule_scan.h
// (rule_heads, rule_owned, rule_before, rule_edge_append, rule_run_goes_on): a wave owns the key runs that
// BEGIN in its 64 sorted rows and walks on a run that leaves the chunk, so a key's ring and row
// have one reading and one writing wave and no atomics touch them. This file adds, between the
// frame's pieces:
//   look-back  A lane's breach ordinal in its run is a popcount of the breach ballot between the
//              run's head lane and the lane. The chunk's breach timestamps are staged in a
//              per-wave LDS strip at their wave-wide breach rank; "the times-th most recent
//              breach at or before me" is strip[rank - times] when it lies in this chunk's part
//              of the run, one 8-byte load of a single slot of the key's stored ring at the head
//              chunk of a run, and a read of the per-wave LDS carry -- the walked run's ring as
//              of the chunk's start -- when the wave is walking on.
//   scan       With `dense` known an element is ID / SET(t) / OFF; a Hillis-Steele segmented
//              scan composes them, the carry is the key's (since, firing), and edges come from
//              a lane's state against its predecessor's.
//   stores     A run that begins and ends in one chunk: its breaches among the last `times`
//              store their slot, after every load of the chunk in program order. A walked run
//              collects them in the LDS carry (filled from the stored ring at the head chunk,
//              before any store to that key) and lanes 0..times-1 store the slots the batch
//              wrote when the run ends. No lane reads from global memory what another lane
//              stored in this launch (the frame's pieces load only the sorted keys and the
//              arrival indices and store only the appended rows, which nothing here loads). The
//              lane that ends a run stores (since, meta).
// sustain_gather (csrc/sustain_hip.hip), the family's gather, turns the appended rows sorted by
// tag into the five columns.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "mxs_burst.h"
#include "rule_scan.h"

namespace mxs {
namespace {

constexpr int kBurstBlock = 256;
constexpr int kBurstWaves = kBurstBlock / 64;
constexpr int kBurstMaxGrid = 8192;

enum { kId = 0, kSet = 1, kOff = 2, kOn = 3 };

// The strip and the carry are written and read by one wave only: LDS operations of a wave
// complete in order, the fence keeps the compiler from moving them across.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(kBurstBlock) void burst_scan_kernel(
    const int64_t* __restrict__ skeys, const int64_t* __restrict__ perm,
    const int64_t* __restrict__ vals, const int64_t* __restrict__ ts, int64_t n, int kind,
    int when, double thr, int times, int64_t within, int64_t* __restrict__ ring,
    ll2* __restrict__ row, int64_t cap, int64_t* __restrict__ out_tag,
    int64_t* __restrict__ out_since, uint32_t* __restrict__ out_n) {
  __shared__ int64_t s_strip[kBurstWaves][64];
  __shared__ int64_t s_carry[kBurstWaves][kBurstMaxTimes];
  const int lane = threadIdx.x & 63;
  int64_t* strip = s_strip[threadIdx.x >> 6];
  int64_t* carry = s_carry[threadIdx.x >> 6];
  const unsigned long long le = (2ull << lane) - 1ull;   // lanes <= lane
  const unsigned long long ge = ~((1ull << lane) - 1ull);  // lanes >= lane
  // Every loop condition is wave-uniform (csrc/rule_scan.h).
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < n;
       base += (int64_t)gridDim.x * blockDim.x) {
    bool cont = false;  // walking on a run that left the wave's own chunk
    // The walked run: its key, its state and ring position at the chunk's start, and the slots
    // the batch has written so far: `bn` of them (at most `times`) from slot `bpos` on.
    int64_t ck = 0, cs = 0;
    int cf = 0, cpos = 0, cheld = 0, bpos = 0, bn = 0;
    for (int64_t b0 = base;; b0 += 64) {
      RuleFrame fr = rule_heads(skeys, n, b0, lane, cont);
      if (fr.leave) break;
      rule_owned(skeys, perm, n, cap, lane, cont, ck, fr);
      const int64_t k = fr.k, src = fr.src;
      const bool head = fr.head, act = fr.act, tail = fr.tail, ok = fr.ok;
      const unsigned long long hm = fr.hm;
      const int64_t t = ok ? ts[src] : 0;
      const bool br = ok && sustain_breach(kind, when, vals[src], thr);
      const unsigned long long tm = __ballot(tail), bm = __ballot(br);
      // The breach ordinal inside the run's part of this chunk, this element included.
      const int hl = cont ? 0 : 63 - __clzll((long long)((hm & le) | 1ull));
      const int rank = __popcll(bm & le);
      const int c = rank - __popcll(bm & ((1ull << hl) - 1ull));
      int held0 = cheld, pos0 = cpos;
      if (!cont) {
        ll2 r;
        r.x = 0, r.y = 0;
        if (ok) r = row[k];  // one 16-byte load; a run's lanes read the same row
        cs = r.x, cf = (int)(r.y & 1);
        held0 = (int)((r.y >> kBurstHeldShift) & 0x7f);
        pos0 = (int)((r.y >> kBurstPosShift) & 0xff);
        pos0 = pos0 < times ? pos0 : 0;  // a ring index stays inside the ring whatever the row holds
      }
      const bool full = held0 + c >= times;
      const int pa = (int)((unsigned)(pos0 + c) % (unsigned)times);  // the slot written next
      if (br) strip[rank - 1] = t;
      wave_sync();
      // recent[0] as of this element: `times` breaches back.
      int64_t old = 0;
      if (ok && full) {
        if (c >= times) old = strip[rank - times];
        else if (cont) old = carry[pa];
        else old = ring[k * times + pa];
      }
      const bool dense = ok && full && t - old <= within;
      // Inclusive segmented wave scan (Hillis-Steele) of the summaries; y is the earlier one.
      int vk = dense ? (br ? kSet : kId) : kOff;
      int64_t vt = old;
      int f = head;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int yk = __shfl_up(vk, o);
        const int64_t yt = __shfl_up(vt, o);
        const int g = __shfl_up(f, o);
        if (lane >= o && !f) {
          if (vk == kId) {
            vk = yk, vt = yt;
          } else if (vk == kSet) {
            if (yk == kOff) vk = kOn;
            else if (yk != kId) vk = yk, vt = yt;
          }
          f = g;
        }
      }
      // The state after this element, and the one before it.
      int64_t s1 = cs;
      int f1 = cf;
      if (vk == kOff) s1 = 0, f1 = 0;
      else if (vk == kOn || (vk == kSet && !cf)) s1 = vt, f1 = 1;
      const int64_t s0 = rule_before(s1, cs, head, lane);
      const int f0 = rule_before(f1, cf, head, lane);
      const bool fire = ok && f1 && !f0;
      const bool resolve = ok && !f1 && f0;
      rule_edge_append(fire, resolve, src, s1, s0, n, out_tag, out_since, out_n, lane);
      // Ring stores: the breaches among the run's last `times` in this chunk.
      const bool ends = act && (tm & ge);  // the lane's run ends in this chunk
      const int tl = ends ? __ffsll((long long)(tm & ge)) - 1 : 63;
      const bool last = br && __popcll(bm & ((2ull << tl) - 1ull)) - rank < times;
      const int ws = pa == 0 ? times - 1 : pa - 1;  // the slot of this lane's breach
      if (!cont && ends && last) ring[k * times + ws] = t;
      const int held1 = held0 + c < times ? held0 + c : times;
      if (tail && ok) {
        ll2 r;
        r.x = f1 ? s1 : 0, r.y = burst_meta(f1, held1, pa);
        row[k] = r;  // one 16-byte store by the lane that ends the run
      }
      const bool goes = rule_run_goes_on(act, tm);
      if (!cont && !goes) break;
      if (!cont) {  // the head chunk of a walk: the key's stored ring, before any store to it
        const int64_t k63 = __shfl(k, 63);
        if (lane < times && (uint64_t)k63 < (uint64_t)cap) carry[lane] = ring[k63 * times + lane];
        bpos = __shfl(pos0, 63);
        bn = 0;
        ck = k63;
        wave_sync();
      }
      if (act && (cont || !ends) && last) carry[ws] = t;
      wave_sync();
      const int xl = goes || !tm ? 63 : __ffsll((long long)tm) - 1;  // the walked run's last lane here
      const int nb = __shfl(c, xl);
      bn = bn + nb < times ? bn + nb : times;
      if (!goes) {  // the walk ends: the slots the batch wrote go to the ring
        int d = lane - bpos;
        d = d < 0 ? d + times : d;
        if (lane < times && (uint64_t)ck < (uint64_t)cap && d < bn)
          ring[ck * times + lane] = carry[lane];
        break;
      }
      cont = true;
      cs = __shfl(s1, 63);
      cf = __shfl(f1, 63);
      cpos = __shfl(pa, 63);
      cheld = __shfl(held1, 63);
    }
  }
}

}  // namespace

namespace gpu {

void burst_scan(const int64_t* skeys, const int64_t* perm, const int64_t* vals, const int64_t* ts,
                int64_t n, int kind, int when, int64_t thr_bits, int times, int64_t within,
                int64_t* ring, int64_t* row, int64_t cap, int64_t* out_tag, int64_t* out_since,
                uint32_t* out_n, intptr_t stream) {
  if (cap < 1 || row == nullptr || ring == nullptr || ((uintptr_t)row & 15u) ||
      ((uintptr_t)ring & 7u))
    throw std::invalid_argument("burst_scan: the row table must be 16-byte aligned, cap >= 1");
  if (n < 0 || n >= ((int64_t)1 << 31)) throw std::invalid_argument("burst_scan: bad row count");
  if (times < 2 || times > kBurstMaxTimes)
    throw std::invalid_argument("burst_scan: times must lie in [2, 16]");
  if (within < 0 || within >= kSustainTsLimit)
    throw std::invalid_argument("burst_scan: within must lie in [0, 2**62)");
  if (when <= kLookupAll || when >= kLookupWhens)
    throw std::invalid_argument("burst_scan: unknown comparison");
  if (kind != kSustainLong && kind != kSustainDouble)
    throw std::invalid_argument("burst_scan: unknown value kind");
  if (out_n == nullptr) throw std::invalid_argument("burst_scan: no row counter");
  hipStream_t s = (hipStream_t)stream;
  MXS_HIP_CHECK(hipMemsetAsync(out_n, 0, sizeof(uint32_t), s));
  if (n == 0) return;
  hipLaunchKernelGGL(burst_scan_kernel, dim3(grid_of(n, kBurstBlock, kBurstMaxGrid)),
                     dim3(kBurstBlock), 0, s, skeys, perm, vals, ts, n, kind, when,
                     lookup_f64(thr_bits), times, within, ring, reinterpret_cast<ll2*>(row), cap,
                     out_tag, out_since, out_n);
  MXS_HIP_CHECK(hipGetLastError());
}

}  // namespace gpu
}  // namespace mxs
