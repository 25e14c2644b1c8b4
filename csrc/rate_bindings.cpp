// mxstream — pybind11 bindings of the counter-rate kernels (csrc/rate_hip.hip) and their C++
// twin (csrc/rate_cpu.cpp). Addresses are passed as integers (tensor data_ptr()); dtypes, sizes
// and contiguity are checked by the Python caller (ops/kernels.py rate_*) before any launch. The
// rule's numbers are checked here (rate_rule) on both paths.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <utility>

#include "mxs_rate.h"
#include "mxs_runtime.h"

namespace py = pybind11;
using namespace mxs;

namespace {

template <class T>
T* TP(intptr_t p) {
  return reinterpret_cast<T*>(p);
}

}  // namespace

void bind_rate(py::module_& m) {
  m.attr("RATE_NONE") = kRateNone;
  // The device scan takes the batch sorted by key (skeys, perm = arrival index of each sorted
  // row); the twin takes it in arrival order. `max_gap` 0: none.
  m.def("gpu_rate_scan", [](intptr_t skeys, intptr_t perm, intptr_t vals, intptr_t ts, int64_t n,
                            int kind, intptr_t state, int64_t cap, intptr_t scratch,
                            intptr_t out_ooo, intptr_t stream) {
    gpu::rate_scan(TP<const int64_t>(skeys), TP<const int64_t>(perm), TP<const int64_t>(vals),
                   TP<const int64_t>(ts), n, kind, TP<int64_t>(state), cap, TP<int64_t>(scratch),
                   TP<uint32_t>(out_ooo), stream);
  });
  m.def("gpu_rate_mask", [](intptr_t scratch, int64_t n, int kind, int when, int64_t thr_bits,
                            int64_t per_ms, int64_t max_gap, intptr_t words, intptr_t counts,
                            intptr_t stream) {
    gpu::rate_mask(TP<const int64_t>(scratch), n, rate_rule(kind, when, thr_bits, per_ms, max_gap),
                   TP<uint64_t>(words), TP<uint32_t>(counts), stream);
  });
  m.def("gpu_rate_emit", [](intptr_t scratch, intptr_t keys, intptr_t ts, int64_t n, int kind,
                            int when, int64_t thr_bits, int64_t per_ms, int64_t max_gap,
                            intptr_t words, intptr_t counts, intptr_t offsets, int64_t kept,
                            intptr_t out_key, intptr_t out_rate, intptr_t out_inc,
                            intptr_t out_dt, intptr_t out_ts, intptr_t stream) {
    gpu::rate_emit(TP<const int64_t>(scratch), TP<const int64_t>(keys), TP<const int64_t>(ts), n,
                   rate_rule(kind, when, thr_bits, per_ms, max_gap), TP<const uint64_t>(words),
                   TP<const uint32_t>(counts), TP<const int64_t>(offsets), kept,
                   TP<int64_t>(out_key), TP<int64_t>(out_rate), TP<int64_t>(out_inc),
                   TP<int64_t>(out_dt), TP<int64_t>(out_ts), stream);
  });
  // -> (rows, ignored elements)
  m.def("cpu_rate_update", [](intptr_t keys, intptr_t vals, intptr_t ts, int64_t n, int kind,
                              int when, int64_t thr_bits, int64_t per_ms, int64_t max_gap,
                              intptr_t state, int64_t cap, intptr_t out_key, intptr_t out_rate,
                              intptr_t out_inc, intptr_t out_dt, intptr_t out_ts) {
    int64_t ignored = 0;
    const int64_t rows = cpu::rate_update(
        TP<const int64_t>(keys), TP<const int64_t>(vals), TP<const int64_t>(ts), n,
        rate_rule(kind, when, thr_bits, per_ms, max_gap), TP<int64_t>(state), cap,
        TP<int64_t>(out_key), TP<int64_t>(out_rate), TP<int64_t>(out_inc), TP<int64_t>(out_dt),
        TP<int64_t>(out_ts), &ignored);
    return std::make_pair(rows, ignored);
  });
}
