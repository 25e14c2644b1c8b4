// mxstream — pybind11 bindings of the keyed timer kernels (csrc/timeout_hip.hip) and their C++
// twins (csrc/timeout_cpu.cpp). Addresses are passed as integers (tensor data_ptr()); dtypes,
// sizes and contiguity are checked by the Python caller (ops/kernels.py timeout_*) before any
// launch.
#include <pybind11/pybind11.h>

#include "mxs_runtime.h"
#include "mxs_timeout.h"

namespace py = pybind11;
using namespace mxs;

namespace {

template <class T>
T* TP(intptr_t p) {
  return reinterpret_cast<T*>(p);
}

}  // namespace

void bind_timeout(py::module_& m) {
  m.attr("TIMEOUT_TILE") = kTimeoutTile;
  m.attr("TIMEOUT_WORDS") = kTimeoutWords;
  m.attr("TIMEOUT_NONE") = kTimeoutNone;
  m.def("timeout_tileskip", [] { return timeout_tileskip(); });
  // The device update takes the batch sorted by key (skeys, perm = arrival index of each sorted
  // row); the twin takes it in arrival order.
  m.def("gpu_timeout_update", [](intptr_t skeys, intptr_t perm, intptr_t ts, int64_t n,
                                 int64_t timeout, intptr_t state, intptr_t deadline,
                                 intptr_t tile_min, int64_t cap, intptr_t stream) {
    gpu::timeout_update(TP<const int64_t>(skeys), TP<const int64_t>(perm), TP<const int64_t>(ts),
                        n, timeout, TP<int64_t>(state), TP<int64_t>(deadline),
                        TP<int64_t>(tile_min), cap, stream);
  });
  m.def("cpu_timeout_update", [](intptr_t keys, intptr_t ts, int64_t n, int64_t timeout,
                                 intptr_t state, intptr_t deadline, intptr_t tile_min,
                                 int64_t cap) {
    cpu::timeout_update(TP<const int64_t>(keys), TP<const int64_t>(ts), n, timeout,
                        TP<int64_t>(state), TP<int64_t>(deadline), TP<int64_t>(tile_min), cap);
  });
  m.def("timeout_mask", [](bool cuda, intptr_t deadline, int64_t cap, int64_t w,
                           intptr_t tile_min, intptr_t words, intptr_t counts, intptr_t stream) {
    if (cuda) {
      gpu::timeout_mask(TP<const int64_t>(deadline), cap, w, TP<int64_t>(tile_min),
                        TP<uint64_t>(words), TP<uint32_t>(counts), stream);
    } else {
      py::gil_scoped_release nogil;
      cpu::timeout_mask(TP<const int64_t>(deadline), cap, w, TP<int64_t>(tile_min),
                        TP<uint64_t>(words), TP<uint32_t>(counts));
    }
  });
  m.def("timeout_emit", [](bool cuda, intptr_t state, intptr_t deadline, int64_t cap,
                           intptr_t words, intptr_t counts, intptr_t offsets, int64_t total,
                           intptr_t out_key, intptr_t out_count, intptr_t out_last,
                           intptr_t out_deadline, intptr_t stream) {
    if (cuda) {
      gpu::timeout_emit(TP<const int64_t>(state), TP<int64_t>(deadline), cap,
                        TP<const uint64_t>(words), TP<const uint32_t>(counts),
                        TP<const int64_t>(offsets), total, TP<int64_t>(out_key),
                        TP<int64_t>(out_count), TP<int64_t>(out_last), TP<int64_t>(out_deadline),
                        stream);
    } else {
      py::gil_scoped_release nogil;
      cpu::timeout_emit(TP<const int64_t>(state), TP<int64_t>(deadline), cap,
                        TP<const uint64_t>(words), TP<const uint32_t>(counts), total,
                        TP<int64_t>(out_key), TP<int64_t>(out_count), TP<int64_t>(out_last),
                        TP<int64_t>(out_deadline));
    }
  });
}
