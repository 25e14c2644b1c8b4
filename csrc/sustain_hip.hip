// mxstream — sustained-condition alerts on gfx950: a per-key state machine over every sample,
// run as a segmented wave scan (declarations, the model and the summary algebra:
// csrc/mxs_sustain.h; C++ twin: csrc/sustain_cpu.cpp).
//
// scan: the batch arrives stably sorted by key and is scanned in the frame of csrc/rule_scan.h:
// a wave owns the key runs that begin in its 64 sorted rows and walks on a run that leaves them,
// so a key's 16-byte row has one reader and one writer and no atomics touch the state; the
// transitions are appended with one reservation per wave and chunk. What is this rule's own is
// the summary and its segmented scan, and the edges it takes from the states.
// gather: the appended rows, sorted by tag, become the five output columns. It is the gather of
// every rule in that frame (burst_update launches it too).
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "mxs_sustain.h"
#include "rule_scan.h"

namespace mxs {
namespace {

constexpr int kSustainBlock = 256;
constexpr int kSustainMaxGrid = 8192;

// A summary: r != 0: reset, (a, b) = the absolute (since, firing) after the stretch;
// r == 0: all-breach, (a, b) = (t_first, t_max).
struct Summary {
  int64_t a, b;
  int r;
};

// An all-breach stretch (t_first, t_max) applied to the state (s, f).
__device__ __forceinline__ void sustain_apply(int64_t t_first, int64_t t_max, int64_t for_ms,
                                              int64_t& s, int64_t& f) {
  if (s != kSustainNone) {
    f = (f || t_max - s >= for_ms) ? 1 : 0;
  } else {
    s = t_first;
    f = t_max - t_first >= for_ms ? 1 : 0;
  }
}

// x, then y.
__device__ __forceinline__ Summary sustain_compose(const Summary& x, const Summary& y,
                                                   int64_t for_ms) {
  if (y.r) return y;
  if (!x.r) return Summary{x.a, x.b > y.b ? x.b : y.b, 0};
  Summary z{x.a, x.b, 1};
  sustain_apply(y.a, y.b, for_ms, z.a, z.b);
  return z;
}

__global__ __launch_bounds__(kSustainBlock) void sustain_scan_kernel(
    const int64_t* __restrict__ skeys, const int64_t* __restrict__ perm,
    const int64_t* __restrict__ vals, const int64_t* __restrict__ ts, int64_t n, int kind,
    int when, double thr, int64_t for_ms, ll2* __restrict__ state, int64_t cap,
    int64_t* __restrict__ out_tag, int64_t* __restrict__ out_since, uint32_t* __restrict__ out_n) {
  const int lane = threadIdx.x & 63;
  // Every loop condition is wave-uniform (csrc/rule_scan.h).
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < n;
       base += (int64_t)gridDim.x * blockDim.x) {
    bool cont = false;  // walking on a run that left the wave's own chunk
    int64_t ck = 0, cs = kSustainNone, cf = 0;
    for (int64_t b0 = base;; b0 += 64) {
      RuleFrame fr = rule_heads(skeys, n, b0, lane, cont);
      if (fr.leave) break;
      rule_owned(skeys, perm, n, cap, lane, cont, ck, fr);
      const int64_t k = fr.k, src = fr.src;
      const bool ok = fr.ok;
      const int64_t t = ok ? ts[src] : 0;
      const bool br = ok && sustain_breach(kind, when, vals[src], thr);
      if (!cont) {
        ll2 row;
        row.x = kSustainNone, row.y = 0;
        if (ok) row = state[k];  // one 16-byte load; a run's lanes read the same row
        cs = row.x, cf = row.y;
      }
      // Inclusive segmented wave scan (Hillis-Steele) of the summaries; y is the earlier one.
      Summary v = br ? Summary{t, t, 0} : Summary{kSustainNone, 0, 1};
      int f = fr.head;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        Summary y;
        y.a = __shfl_up(v.a, o);
        y.b = __shfl_up(v.b, o);
        y.r = __shfl_up(v.r, o);
        const int g = __shfl_up(f, o);
        if (lane >= o && !f) {
          v = sustain_compose(y, v, for_ms);
          f = g;
        }
      }
      // The state after this element, and the one before it.
      int64_t s1 = v.a, f1 = v.b;
      if (!v.r) {
        s1 = cs, f1 = cf;
        sustain_apply(v.a, v.b, for_ms, s1, f1);
      }
      const int64_t s0 = rule_before(s1, cs, fr.head, lane);
      const int64_t f0 = rule_before(f1, cf, fr.head, lane);
      const bool fire = ok && f1 && !f0;
      const bool resolve = ok && !br && f0;
      rule_edge_append(fire, resolve, src, s1, s0, n, out_tag, out_since, out_n, lane);
      if (fr.tail && ok) {
        ll2 row;
        row.x = s1, row.y = f1;
        state[k] = row;  // one 16-byte store by the lane that ends the run
      }
      if (!rule_run_goes_on(fr.act, __ballot(fr.tail))) break;
      cont = true;
      ck = __shfl(k, 63);
      cs = __shfl(s1, 63);
      cf = __shfl(f1, 63);
    }
  }
}

__global__ __launch_bounds__(kSustainBlock) void sustain_gather_kernel(
    const int64_t* __restrict__ tags, const int64_t* __restrict__ since, int64_t m,
    const int64_t* __restrict__ keys, const int64_t* __restrict__ vals,
    const int64_t* __restrict__ ts, int64_t n, int64_t* __restrict__ out_key,
    int64_t* __restrict__ out_code, int64_t* __restrict__ out_since, int64_t* __restrict__ out_val,
    int64_t* __restrict__ out_ts) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m;
       j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t tag = tags[j];
    const int64_t a = tag >> 1;
    if ((uint64_t)a >= (uint64_t)n) continue;
    out_key[j] = keys[a];
    out_code[j] = tag & 1;
    out_since[j] = since[j];
    out_val[j] = vals[a];
    out_ts[j] = ts[a];
  }
}

}  // namespace

namespace gpu {

void sustain_scan(const int64_t* skeys, const int64_t* perm, const int64_t* vals,
                  const int64_t* ts, int64_t n, int kind, int when, int64_t thr_bits,
                  int64_t for_ms, int64_t* state, int64_t cap, int64_t* out_tag,
                  int64_t* out_since, uint32_t* out_n, intptr_t stream) {
  if (cap < 1 || state == nullptr || ((uintptr_t)state & 15u))
    throw std::invalid_argument("sustain_scan: the table must be 16-byte aligned, cap >= 1");
  if (n < 0 || n >= ((int64_t)1 << 31)) throw std::invalid_argument("sustain_scan: bad row count");
  if (for_ms < 0) throw std::invalid_argument("sustain_scan: for_ms must not be negative");
  if (when <= kLookupAll || when >= kLookupWhens)
    throw std::invalid_argument("sustain_scan: unknown comparison");
  if (kind != kSustainLong && kind != kSustainDouble)
    throw std::invalid_argument("sustain_scan: unknown value kind");
  if (out_n == nullptr) throw std::invalid_argument("sustain_scan: no row counter");
  hipStream_t s = (hipStream_t)stream;
  MXS_HIP_CHECK(hipMemsetAsync(out_n, 0, sizeof(uint32_t), s));
  if (n == 0) return;
  hipLaunchKernelGGL(sustain_scan_kernel, dim3(grid_of(n, kSustainBlock, kSustainMaxGrid)),
                     dim3(kSustainBlock), 0, s, skeys, perm, vals, ts, n, kind, when,
                     lookup_f64(thr_bits), for_ms, reinterpret_cast<ll2*>(state), cap, out_tag,
                     out_since, out_n);
  MXS_HIP_CHECK(hipGetLastError());
}

void sustain_gather(const int64_t* tags, const int64_t* since, int64_t m, const int64_t* keys,
                    const int64_t* vals, const int64_t* ts, int64_t n, int64_t* out_key,
                    int64_t* out_code, int64_t* out_since, int64_t* out_val, int64_t* out_ts,
                    intptr_t stream) {
  if (m < 0 || m > n) throw std::invalid_argument("sustain_gather: bad row count");
  if (m == 0) return;
  hipLaunchKernelGGL(sustain_gather_kernel, dim3(grid_of(m, kSustainBlock, kSustainMaxGrid)),
                     dim3(kSustainBlock), 0, (hipStream_t)stream, tags, since, m, keys, vals, ts,
                     n, out_key, out_code, out_since, out_val, out_ts);
  MXS_HIP_CHECK(hipGetLastError());
}

}  // namespace gpu
}  // namespace mxs
