// mxstream — pybind11 bindings of the burst-alert kernel (csrc/burst_hip.hip) and its C++ twin
// (csrc/burst_cpu.cpp). Addresses are passed as integers (tensor data_ptr()); dtypes, sizes and
// contiguity are checked by the Python caller (ops/kernels.py burst_*) before any launch.
#include <pybind11/pybind11.h>

#include "mxs_burst.h"
#include "mxs_runtime.h"

namespace py = pybind11;
using namespace mxs;

namespace {

template <class T>
T* TP(intptr_t p) {
  return reinterpret_cast<T*>(p);
}

}  // namespace

void bind_burst(py::module_& m) {
  m.attr("BURST_MAX_TIMES") = kBurstMaxTimes;
  m.attr("BURST_HELD_SHIFT") = kBurstHeldShift;
  m.attr("BURST_POS_SHIFT") = kBurstPosShift;
  // The device scan takes the batch sorted by key (skeys, perm = arrival index of each sorted
  // row); the twin takes it in arrival order.
  m.def("gpu_burst_scan", [](intptr_t skeys, intptr_t perm, intptr_t vals, intptr_t ts, int64_t n,
                             int kind, int when, int64_t thr_bits, int times, int64_t within,
                             intptr_t ring, intptr_t row, int64_t cap, intptr_t out_tag,
                             intptr_t out_since, intptr_t out_n, intptr_t stream) {
    gpu::burst_scan(TP<const int64_t>(skeys), TP<const int64_t>(perm), TP<const int64_t>(vals),
                    TP<const int64_t>(ts), n, kind, when, thr_bits, times, within,
                    TP<int64_t>(ring), TP<int64_t>(row), cap, TP<int64_t>(out_tag),
                    TP<int64_t>(out_since), TP<uint32_t>(out_n), stream);
  });
  m.def("cpu_burst_update", [](intptr_t keys, intptr_t vals, intptr_t ts, int64_t n, int kind,
                               int when, int64_t thr_bits, int times, int64_t within,
                               intptr_t ring, intptr_t row, int64_t cap, intptr_t out_key,
                               intptr_t out_code, intptr_t out_since, intptr_t out_val,
                               intptr_t out_ts) {
    return cpu::burst_update(TP<const int64_t>(keys), TP<const int64_t>(vals),
                             TP<const int64_t>(ts), n, kind, when, thr_bits, times, within,
                             TP<int64_t>(ring), TP<int64_t>(row), cap, TP<int64_t>(out_key),
                             TP<int64_t>(out_code), TP<int64_t>(out_since),
                             TP<int64_t>(out_val), TP<int64_t>(out_ts));
  });
}
