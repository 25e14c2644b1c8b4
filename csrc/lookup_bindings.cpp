// mxstream — pybind11 bindings of the latest-value lookup kernels (csrc/lookup_hip.hip) and their
// C++ twins (csrc/lookup_cpu.cpp). Addresses are passed as integers (tensor data_ptr()); dtypes,
// sizes and contiguity are checked by the Python caller (ops/kernels.py lookup_*) before any
// launch.
#include <pybind11/pybind11.h>

#include "mxs_lookup.h"
#include "mxs_runtime.h"

namespace py = pybind11;
using namespace mxs;

namespace {

template <class T>
T* LP(intptr_t p) {
  return reinterpret_cast<T*>(p);
}

}  // namespace

void bind_lookup(py::module_& m) {
  m.attr("LOOKUP_TILE") = kLookupTile;
  m.attr("LOOKUP_WORDS") = kLookupWords;
  m.attr("LOOKUP_META") = kLookupMeta;
  m.attr("LOOKUP_WHENS") = (int)kLookupWhens;
  // The device upsert takes the batch sorted by key (skeys, perm = arrival index of each sorted
  // row); the twin takes it in arrival order.
  m.def("gpu_lookup_upsert", [](intptr_t skeys, intptr_t perm, intptr_t vals, int64_t n,
                                intptr_t table, int64_t cap, intptr_t stream) {
    gpu::lookup_upsert(LP<const int64_t>(skeys), LP<const int64_t>(perm), LP<const int64_t>(vals),
                       n, LP<int64_t>(table), cap, stream);
  });
  m.def("cpu_lookup_upsert", [](intptr_t keys, intptr_t vals, int64_t n, intptr_t table,
                                int64_t cap) {
    cpu::lookup_upsert(LP<const int64_t>(keys), LP<const int64_t>(vals), n, LP<int64_t>(table),
                       cap);
  });
  m.def("lookup_mask", [](bool cuda, intptr_t keys, intptr_t vals, int64_t n, intptr_t table,
                          int64_t cap, int when, bool has_default, int64_t default_bits,
                          intptr_t words, intptr_t counts, intptr_t stream) {
    if (cuda) {
      gpu::lookup_mask(LP<const int64_t>(keys), LP<const int64_t>(vals), n,
                       LP<const int64_t>(table), cap, when, has_default, default_bits,
                       LP<uint64_t>(words), LP<uint32_t>(counts), stream);
    } else {
      py::gil_scoped_release nogil;
      cpu::lookup_mask(LP<const int64_t>(keys), LP<const int64_t>(vals), n,
                       LP<const int64_t>(table), cap, when, has_default, default_bits,
                       LP<uint64_t>(words), LP<uint32_t>(counts));
    }
  });
  m.def("lookup_scan", [](bool cuda, intptr_t counts, int64_t ntiles, intptr_t offsets,
                          intptr_t meta, intptr_t stream) {
    if (cuda)
      gpu::lookup_scan(LP<const uint32_t>(counts), ntiles, LP<int64_t>(offsets), LP<int64_t>(meta),
                       stream);
    else
      cpu::lookup_scan(LP<const uint32_t>(counts), ntiles, LP<int64_t>(offsets),
                       LP<int64_t>(meta));
  });
  m.def("lookup_emit", [](bool cuda, intptr_t keys, intptr_t vals, intptr_t ts, int64_t n,
                          intptr_t table, int64_t cap, bool has_default, int64_t default_bits,
                          intptr_t words, intptr_t counts, intptr_t offsets, int64_t kept,
                          intptr_t out_key, intptr_t out_val, intptr_t out_t, intptr_t out_ts,
                          intptr_t stream) {
    if (cuda) {
      gpu::lookup_emit(LP<const int64_t>(keys), LP<const int64_t>(vals), LP<const int64_t>(ts), n,
                       LP<const int64_t>(table), cap, has_default, default_bits,
                       LP<const uint64_t>(words), LP<const uint32_t>(counts),
                       LP<const int64_t>(offsets), kept, LP<int64_t>(out_key),
                       LP<int64_t>(out_val), LP<int64_t>(out_t), LP<int64_t>(out_ts), stream);
    } else {
      py::gil_scoped_release nogil;
      cpu::lookup_emit(LP<const int64_t>(keys), LP<const int64_t>(vals), LP<const int64_t>(ts), n,
                       LP<const int64_t>(table), cap, has_default, default_bits,
                       LP<const uint64_t>(words), kept, LP<int64_t>(out_key), LP<int64_t>(out_val),
                       LP<int64_t>(out_t), LP<int64_t>(out_ts));
    }
  });
  m.def("lookup_gather", [](bool cuda, intptr_t keys, intptr_t vals, intptr_t ts, int64_t n,
                            intptr_t table, int64_t cap, int64_t default_bits, intptr_t out_key,
                            intptr_t out_val, intptr_t out_t, intptr_t out_ts, intptr_t stream) {
    if (cuda) {
      gpu::lookup_gather(LP<const int64_t>(keys), LP<const int64_t>(vals), LP<const int64_t>(ts),
                         n, LP<const int64_t>(table), cap, default_bits, LP<int64_t>(out_key),
                         LP<int64_t>(out_val), LP<int64_t>(out_t), LP<int64_t>(out_ts), stream);
    } else {
      py::gil_scoped_release nogil;
      cpu::lookup_gather(LP<const int64_t>(keys), LP<const int64_t>(vals), LP<const int64_t>(ts),
                         n, LP<const int64_t>(table), cap, default_bits, LP<int64_t>(out_key),
                         LP<int64_t>(out_val), LP<int64_t>(out_t), LP<int64_t>(out_ts));
    }
  });
}
