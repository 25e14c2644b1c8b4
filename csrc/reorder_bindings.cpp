// mxstream — pybind11 bindings of the reorder-buffer kernels (csrc/reorder_hip.hip) and their C++
// twins (csrc/reorder_cpu.cpp). Addresses are passed as integers (tensor data_ptr()); dtypes,
// sizes and contiguity are checked by the Python caller (ops/kernels.py reorder_*) before any
// launch.
#include <pybind11/pybind11.h>

#include "mxs_reorder.h"
#include "mxs_runtime.h"

namespace py = pybind11;
using namespace mxs;

namespace {

template <class T>
T* TP(intptr_t p) {
  return reinterpret_cast<T*>(p);
}

}  // namespace

void bind_reorder(py::module_& m) {
  m.attr("REORDER_TILE") = kReorderTile;
  m.attr("REORDER_MAX_CHUNKS") = kReorderMaxChunks;
  m.def("gpu_reorder_cut", [](intptr_t ts, int64_t n_arena, intptr_t begin, intptr_t end,
                              int64_t k, int64_t w, intptr_t cut, intptr_t stream) {
    gpu::reorder_cut(TP<const int64_t>(ts), n_arena, TP<const int64_t>(begin),
                     TP<const int64_t>(end), k, w, TP<int64_t>(cut), stream);
  });
  m.def("gpu_reorder_collect", [](intptr_t ts, int64_t n_arena, intptr_t begin, intptr_t dest,
                                  int64_t k, int64_t total, int64_t lo, intptr_t out_key,
                                  intptr_t out_src, intptr_t err, intptr_t stream) {
    gpu::reorder_collect(TP<const int64_t>(ts), n_arena, TP<const int64_t>(begin),
                         TP<const int64_t>(dest), k, total, lo, TP<int64_t>(out_key),
                         TP<int64_t>(out_src), TP<uint32_t>(err), stream);
  });
  m.def("gpu_reorder_gather", [](intptr_t perm, int64_t n, intptr_t src_key, intptr_t src_ts,
                                 intptr_t src_bits, int64_t n_src, intptr_t dst_key,
                                 intptr_t dst_ts, intptr_t dst_bits, intptr_t err,
                                 intptr_t stream) {
    gpu::reorder_gather(TP<const int64_t>(perm), n, TP<const int64_t>(src_key),
                        TP<const int64_t>(src_ts), TP<const int64_t>(src_bits), n_src,
                        TP<int64_t>(dst_key), TP<int64_t>(dst_ts), TP<int64_t>(dst_bits),
                        TP<uint32_t>(err), stream);
  });
  m.def("cpu_reorder_cut", [](intptr_t ts, int64_t n_arena, intptr_t begin, intptr_t end,
                              int64_t k, int64_t w, intptr_t cut) {
    cpu::reorder_cut(TP<const int64_t>(ts), n_arena, TP<const int64_t>(begin),
                     TP<const int64_t>(end), k, w, TP<int64_t>(cut));
  });
  m.def("cpu_reorder_collect", [](intptr_t ts, int64_t n_arena, intptr_t begin, intptr_t dest,
                                  int64_t k, int64_t total, int64_t lo, intptr_t out_key,
                                  intptr_t out_src) {
    cpu::reorder_collect(TP<const int64_t>(ts), n_arena, TP<const int64_t>(begin),
                         TP<const int64_t>(dest), k, total, lo, TP<int64_t>(out_key),
                         TP<int64_t>(out_src));
  });
  m.def("cpu_reorder_gather", [](intptr_t perm, int64_t n, intptr_t src_key, intptr_t src_ts,
                                 intptr_t src_bits, int64_t n_src, intptr_t dst_key,
                                 intptr_t dst_ts, intptr_t dst_bits) {
    cpu::reorder_gather(TP<const int64_t>(perm), n, TP<const int64_t>(src_key),
                        TP<const int64_t>(src_ts), TP<const int64_t>(src_bits), n_src,
                        TP<int64_t>(dst_key), TP<int64_t>(dst_ts), TP<int64_t>(dst_bits));
  });
}
