// mxstream — pybind11 bindings of the window-join kernels (csrc/join_hip.hip) and their C++
// twins (csrc/join_cpu.cpp). Addresses are passed as integers (tensor data_ptr()); dtypes, sizes
// and contiguity are checked by the Python caller (ops/kernels.py join_*) before any launch.
#include <pybind11/pybind11.h>

#include <stdexcept>

#include "mxs_join.h"
#include "mxs_runtime.h"

namespace py = pybind11;
using namespace mxs;

namespace {

template <class T>
T* JP(intptr_t p) {
  return reinterpret_cast<T*>(p);
}

JoinSide side(intptr_t keys, intptr_t heads, int64_t nseg, int64_t total) {
  if (nseg < 0 || total < 0) throw std::invalid_argument("join: negative segment count / total");
  return JoinSide{JP<const int64_t>(keys), JP<const int64_t>(heads), nseg, total};
}

}  // namespace

void bind_join(py::module_& m) {
  m.attr("JOIN_MAX_PAIRS") = kJoinMaxPairs;
  m.attr("JOIN_PLAN_COLS") = kJoinPlanCols;
  m.attr("JOIN_META") = kJoinMeta;
  m.attr("JOIN_TILE") = kJoinTile;
  m.def("join_match", [](bool cuda, intptr_t lkeys, intptr_t lheads, int64_t kl, int64_t ltotal,
                         intptr_t rkeys, intptr_t rheads, int64_t kr, int64_t rtotal,
                         intptr_t match, intptr_t cnt, intptr_t stream) {
    const JoinSide l = side(lkeys, lheads, kl, ltotal), r = side(rkeys, rheads, kr, rtotal);
    if (cuda)
      gpu::join_match(l, r, JP<int64_t>(match), JP<uint64_t>(cnt), stream);
    else
      cpu::join_match(l, r, JP<int64_t>(match), JP<uint64_t>(cnt));
  });
  m.def("join_scan_scratch_bytes", &gpu::join_scan_scratch_bytes);
  m.def("join_scan", [](bool cuda, intptr_t lkeys, intptr_t lheads, int64_t kl, int64_t ltotal,
                        intptr_t rkeys, intptr_t rheads, int64_t kr, int64_t rtotal,
                        intptr_t match, intptr_t cnt, intptr_t scratch, intptr_t pair_off,
                        intptr_t plan, intptr_t meta, intptr_t stream) {
    const JoinSide l = side(lkeys, lheads, kl, ltotal), r = side(rkeys, rheads, kr, rtotal);
    if (cuda)
      gpu::join_scan(l, r, JP<int64_t>(match), JP<uint64_t>(cnt), JP<void>(scratch),
                     JP<int64_t>(pair_off), JP<int64_t>(plan), JP<int64_t>(meta), stream);
    else
      cpu::join_scan(l, r, JP<int64_t>(match), JP<uint64_t>(cnt), JP<int64_t>(pair_off),
                     JP<int64_t>(plan), JP<int64_t>(meta));
  });
  m.def("gpu_join_expand", [](intptr_t plan, int64_t kl, int64_t nmatched, int64_t P,
                              intptr_t lord, intptr_t rord, int64_t p0, int64_t p1,
                              intptr_t out_key, intptr_t out_l, intptr_t out_r, intptr_t stream) {
    gpu::join_expand(JP<int64_t>(plan), kl, nmatched, P, JP<uint64_t>(lord), JP<uint64_t>(rord),
                     p0, p1, JP<int64_t>(out_key), JP<int64_t>(out_l), JP<int64_t>(out_r), stream);
  });
  m.def("cpu_join_expand", [](intptr_t lkeys, intptr_t lheads, int64_t kl, int64_t ltotal,
                              intptr_t rkeys, intptr_t rheads, int64_t kr, int64_t rtotal,
                              intptr_t match, intptr_t pair_off, intptr_t lord, intptr_t rord,
                              int64_t p0, int64_t p1, intptr_t out_key, intptr_t out_l,
                              intptr_t out_r) {
    const JoinSide l = side(lkeys, lheads, kl, ltotal), r = side(rkeys, rheads, kr, rtotal);
    py::gil_scoped_release nogil;
    cpu::join_expand(l, r, JP<int64_t>(match), JP<int64_t>(pair_off), JP<uint64_t>(lord),
                     JP<uint64_t>(rord), p0, p1, JP<int64_t>(out_key), JP<int64_t>(out_l),
                     JP<int64_t>(out_r));
  });
}
