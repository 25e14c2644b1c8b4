// mxstream — pybind11 bindings of the sustained-alert kernels (csrc/sustain_hip.hip) and their
// C++ twin (csrc/sustain_cpu.cpp). Addresses are passed as integers (tensor data_ptr()); dtypes,
// sizes and contiguity are checked by the Python caller (ops/kernels.py sustain_*) before any
// launch.
#include <pybind11/pybind11.h>

#include "mxs_runtime.h"
#include "mxs_sustain.h"

namespace py = pybind11;
using namespace mxs;

namespace {

template <class T>
T* TP(intptr_t p) {
  return reinterpret_cast<T*>(p);
}

}  // namespace

void bind_sustain(py::module_& m) {
  m.attr("SUSTAIN_NONE") = kSustainNone;
  m.attr("SUSTAIN_TS_LIMIT") = kSustainTsLimit;
  m.attr("SUSTAIN_LONG") = kSustainLong;
  m.attr("SUSTAIN_DOUBLE") = kSustainDouble;
  // The device scan takes the batch sorted by key (skeys, perm = arrival index of each sorted
  // row); the twin takes it in arrival order.
  m.def("gpu_sustain_scan", [](intptr_t skeys, intptr_t perm, intptr_t vals, intptr_t ts,
                               int64_t n, int kind, int when, int64_t thr_bits, int64_t for_ms,
                               intptr_t state, int64_t cap, intptr_t out_tag, intptr_t out_since,
                               intptr_t out_n, intptr_t stream) {
    gpu::sustain_scan(TP<const int64_t>(skeys), TP<const int64_t>(perm), TP<const int64_t>(vals),
                      TP<const int64_t>(ts), n, kind, when, thr_bits, for_ms, TP<int64_t>(state),
                      cap, TP<int64_t>(out_tag), TP<int64_t>(out_since), TP<uint32_t>(out_n),
                      stream);
  });
  m.def("gpu_sustain_gather", [](intptr_t tags, intptr_t since, int64_t rows, intptr_t keys,
                                 intptr_t vals, intptr_t ts, int64_t n, intptr_t out_key,
                                 intptr_t out_code, intptr_t out_since, intptr_t out_val,
                                 intptr_t out_ts, intptr_t stream) {
    gpu::sustain_gather(TP<const int64_t>(tags), TP<const int64_t>(since), rows,
                        TP<const int64_t>(keys), TP<const int64_t>(vals), TP<const int64_t>(ts),
                        n, TP<int64_t>(out_key), TP<int64_t>(out_code), TP<int64_t>(out_since),
                        TP<int64_t>(out_val), TP<int64_t>(out_ts), stream);
  });
  m.def("cpu_sustain_update", [](intptr_t keys, intptr_t vals, intptr_t ts, int64_t n, int kind,
                                 int when, int64_t thr_bits, int64_t for_ms, intptr_t state,
                                 int64_t cap, intptr_t out_key, intptr_t out_code,
                                 intptr_t out_since, intptr_t out_val, intptr_t out_ts) {
    return cpu::sustain_update(TP<const int64_t>(keys), TP<const int64_t>(vals),
                               TP<const int64_t>(ts), n, kind, when, thr_bits, for_ms,
                               TP<int64_t>(state), cap, TP<int64_t>(out_key),
                               TP<int64_t>(out_code), TP<int64_t>(out_since),
                               TP<int64_t>(out_val), TP<int64_t>(out_ts));
  });
}
