// mxstream — keyed state machines on gfx950: one finite state machine per key, stepped by every
// sample, run as a segmented wave scan of packed functions (declarations, the model and the
// algebra: csrc/mxs_fsm.h; C++ twin: csrc/fsm_cpu.cpp).
//
// scan: the batch arrives stably sorted by key and is scanned in the frame of csrc/rule_scan.h,
// as sustain_scan_kernel does: a wave owns the key runs that begin in its 64 sorted rows and
// walks on a run that leaves them, so a key's 16-byte row has one reader and one writer and no
// atomics touch the state. What is this rule's own: an element is the column of the transition
// table for its class, a function S -> S packed 4 bits per state into one 64-bit register, and a
// stretch of elements is the composition of its functions. The state after an element is nibble
// `carry` of its run's composition so far; `since` is the timestamp of the last element at or
// before it, in its run, that changed the state.
// gather: the appended rows, sorted by tag (arrival << 8 | from << 4 | to), become the five
// output columns.
//
// The rule travels as a kernel argument (FsmRule, 296 bytes): every index into bounds and cols
// is a loop counter that is the same in all 64 lanes, so they are read with scalar loads from
// the argument segment. The one index that differs between lanes, report[from], is a select
// chain over four words (fsm_reported). No LDS, no scratch.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "mxs_fsm.h"
#include "rule_scan.h"

namespace mxs {
namespace {

constexpr int kFsmBlock = 256;
constexpr int kFsmMaxGrid = 8192;

__global__ __launch_bounds__(kFsmBlock) void fsm_scan_kernel(
    const int64_t* __restrict__ skeys, const int64_t* __restrict__ perm,
    const int64_t* __restrict__ vals, const int64_t* __restrict__ ts, int64_t n,
    const FsmRule rule, ll2* __restrict__ state, int64_t cap, int64_t* __restrict__ out_tag,
    int64_t* __restrict__ out_since, uint32_t* __restrict__ out_n) {
  const int lane = threadIdx.x & 63;
  const int states = rule.states;
  const unsigned long long upto = (2ull << lane) - 1ull;  // lanes 0 .. lane (lane 63: all)
  // Every loop condition is wave-uniform (csrc/rule_scan.h).
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < n;
       base += (int64_t)gridDim.x * blockDim.x) {
    bool cont = false;  // walking on a run that left the wave's own chunk
    int64_t ck = 0, cs = kFsmNone;
    int cst = 0;
    for (int64_t b0 = base;; b0 += 64) {
      RuleFrame fr = rule_heads(skeys, n, b0, lane, cont);
      if (fr.leave) break;
      rule_owned(skeys, perm, n, cap, lane, cont, ck, fr);
      const int64_t k = fr.k, src = fr.src;
      const bool ok = fr.ok;
      const int64_t t = ok ? ts[src] : 0;
      // a lane outside the wave's runs maps every state to 0; no owned lane reads it
      uint64_t v = ok ? fsm_function(rule, vals[src]) : 0ull;
      bool fresh = false;  // the run begins here and its key was never seen
      if (!cont) {
        ll2 row;
        row.x = kFsmNone, row.y = 0;
        if (ok) row = state[k];  // one 16-byte load; a run's lanes read the same row
        fresh = ok && row.x == kFsmNone;
        // A key that was never seen enters `initial` at its first element, the run's head: the
        // head's own timestamp is its `since` before, and the lanes behind it take theirs from
        // the head (`mark` below), never from this carry.
        cs = fresh ? t : row.x;
        cst = fresh ? rule.initial : (int)(row.y & 15);
      }
      // Inclusive segmented wave scan (Hillis-Steele) of the functions; y is the earlier one.
      int f = fr.head;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint64_t y = (uint64_t)__shfl_up((long long)v, o);
        const int g = __shfl_up(f, o);
        if (lane >= o && !f) {
          v = fsm_compose(y, v, states);
          f = g;
        }
      }
      // The state after this element, and the one before it.
      const int st1 = fsm_next(v, cst);
      const int st0 = rule_before(st1, cst, fr.head, lane);
      // `since` after: the timestamp of the highest lane at or before this one, in the same
      // run, whose element changed the state (or entered `initial`); else the carry's. A
      // segmented max scan of lane numbers, which two ballots answer without a scan: the run
      // begins at the highest head at or below the lane (lane 0 while walking on).
      const bool mark = ok && (st1 != st0 || (fresh && fr.head));
      const unsigned long long cm = __ballot(mark);
      const unsigned long long hb = fr.hm & upto;
      const int first = hb ? 63 - __clzll((long long)hb) : 0;
      const unsigned long long c = cm & upto & ~((1ull << first) - 1ull);
      const int from_lane = c ? 63 - __clzll((long long)c) : lane;
      const int64_t tc = __shfl(t, from_lane);
      const int64_t s1 = c ? tc : cs;
      const int64_t s0 = rule_before(s1, cs, fr.head, lane);
      const bool emit = ok && fsm_reported(rule, st0, st1);
      rule_row_append(emit, (src << kFsmTagBits) | (int64_t)(st0 << 4 | st1), s0, n, out_tag,
                      out_since, out_n, lane);
      if (fr.tail && ok) {
        ll2 row;
        row.x = s1, row.y = st1;
        state[k] = row;  // one 16-byte store by the lane that ends the run
      }
      if (!rule_run_goes_on(fr.act, __ballot(fr.tail))) break;
      cont = true;
      ck = __shfl(k, 63);
      cs = __shfl(s1, 63);
      cst = __shfl(st1, 63);
    }
  }
}

__global__ __launch_bounds__(kFsmBlock) void fsm_gather_kernel(
    const int64_t* __restrict__ tags, const int64_t* __restrict__ since, int64_t m,
    const int64_t* __restrict__ keys, const int64_t* __restrict__ vals,
    const int64_t* __restrict__ ts, int64_t n, int64_t* __restrict__ out_key,
    int64_t* __restrict__ out_code, int64_t* __restrict__ out_since, int64_t* __restrict__ out_val,
    int64_t* __restrict__ out_ts) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m;
       j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t tag = tags[j];
    const int64_t a = tag >> kFsmTagBits;
    if ((uint64_t)a >= (uint64_t)n) continue;
    out_key[j] = keys[a];
    out_code[j] = tag & ((1 << kFsmTagBits) - 1);
    out_since[j] = since[j];
    out_val[j] = vals[a];
    out_ts[j] = ts[a];
  }
}

}  // namespace

namespace gpu {

void fsm_scan(const int64_t* skeys, const int64_t* perm, const int64_t* vals, const int64_t* ts,
              int64_t n, const FsmRule& rule, int64_t* state, int64_t cap, int64_t* out_tag,
              int64_t* out_since, uint32_t* out_n, intptr_t stream) {
  if (cap < 1 || state == nullptr || ((uintptr_t)state & 15u))
    throw std::invalid_argument("fsm_scan: the table must be 16-byte aligned, cap >= 1");
  if (n < 0 || n >= ((int64_t)1 << 31)) throw std::invalid_argument("fsm_scan: bad row count");
  if (out_n == nullptr) throw std::invalid_argument("fsm_scan: no row counter");
  hipStream_t s = (hipStream_t)stream;
  MXS_HIP_CHECK(hipMemsetAsync(out_n, 0, sizeof(uint32_t), s));
  if (n == 0) return;
  hipLaunchKernelGGL(fsm_scan_kernel, dim3(grid_of(n, kFsmBlock, kFsmMaxGrid)), dim3(kFsmBlock),
                     0, s, skeys, perm, vals, ts, n, rule, reinterpret_cast<ll2*>(state), cap,
                     out_tag, out_since, out_n);
  MXS_HIP_CHECK(hipGetLastError());
}

void fsm_gather(const int64_t* tags, const int64_t* since, int64_t m, const int64_t* keys,
                const int64_t* vals, const int64_t* ts, int64_t n, int64_t* out_key,
                int64_t* out_code, int64_t* out_since, int64_t* out_val, int64_t* out_ts,
                intptr_t stream) {
  if (m < 0 || m > n) throw std::invalid_argument("fsm_gather: bad row count");
  if (m == 0) return;
  hipLaunchKernelGGL(fsm_gather_kernel, dim3(grid_of(m, kFsmBlock, kFsmMaxGrid)),
                     dim3(kFsmBlock), 0, (hipStream_t)stream, tags, since, m, keys, vals, ts, n,
                     out_key, out_code, out_since, out_val, out_ts);
  MXS_HIP_CHECK(hipGetLastError());
}

}  // namespace gpu
}  // namespace mxs
