// mxstream — pybind11 bindings of the interval-join kernels (csrc/ijoin_hip.hip) and their C++
// twins (csrc/ijoin_cpu.cpp). Addresses are passed as integers (tensor data_ptr()); dtypes, sizes
// and contiguity are checked by the Python caller (ops/kernels.py ijoin_*) before any launch.
#include <pybind11/pybind11.h>

#include <stdexcept>

#include "mxs_ijoin.h"
#include "mxs_runtime.h"

namespace py = pybind11;
using namespace mxs;

namespace {

template <class T>
T* IP(intptr_t p) {
  return reinterpret_cast<T*>(p);
}

IJoinCols cols(intptr_t key, intptr_t ts, intptr_t val, int64_t n) {
  if (n < 0) throw std::invalid_argument("ijoin: negative row count");
  return IJoinCols{IP<const int64_t>(key), IP<const int64_t>(ts), IP<const int64_t>(val), n};
}

}  // namespace

void bind_ijoin(py::module_& m) {
  m.attr("IJOIN_PLAN_COLS") = kIJoinPlanCols;
  m.attr("IJOIN_META") = kIJoinMeta;
  m.def("ijoin_probe", [](bool cuda, intptr_t bkey, intptr_t bts, int64_t nb, intptr_t okey,
                          intptr_t ots, int64_t no, int64_t rlo, int64_t rhi, int64_t cutoff,
                          intptr_t lb, intptr_t cnt, intptr_t stream) {
    const IJoinCols b = cols(bkey, bts, 0, nb), o = cols(okey, ots, 0, no);
    if (cuda) {
      gpu::ijoin_probe(b, o, rlo, rhi, cutoff, IP<int64_t>(lb), IP<uint64_t>(cnt), stream);
    } else {
      py::gil_scoped_release nogil;
      cpu::ijoin_probe(b, o, rlo, rhi, cutoff, IP<int64_t>(lb), IP<uint64_t>(cnt));
    }
  });
  m.def("ijoin_scan_scratch_bytes", &gpu::ijoin_scan_scratch_bytes);
  m.def("ijoin_scan", [](bool cuda, intptr_t cnt, intptr_t lb, int64_t n, intptr_t scratch,
                         intptr_t plan, intptr_t meta, intptr_t stream) {
    if (cuda)
      gpu::ijoin_scan(IP<uint64_t>(cnt), IP<int64_t>(lb), n, IP<void>(scratch), IP<int64_t>(plan),
                      IP<int64_t>(meta), stream);
    else
      cpu::ijoin_scan(IP<uint64_t>(cnt), IP<int64_t>(lb), n, IP<int64_t>(plan),
                      IP<int64_t>(meta));
  });
  // The plan must be ijoin_scan's of ijoin_probe's output for these same batch and other columns
  // (see gpu::ijoin_expand): go through ops/kernels.py ijoin_plan / ijoin_expand.
  m.def("gpu_ijoin_expand", [](intptr_t plan, int64_t n, int64_t nrows, int64_t P, intptr_t bkey,
                               intptr_t bts, intptr_t bval, intptr_t ots, intptr_t oval,
                               int64_t no, int side, int64_t p0, int64_t p1, intptr_t out_key,
                               intptr_t out_l, intptr_t out_r, intptr_t out_ts, intptr_t stream) {
    gpu::ijoin_expand(IP<int64_t>(plan), n, nrows, P, cols(bkey, bts, bval, n),
                      cols(0, ots, oval, no), side, p0, p1, IP<int64_t>(out_key),
                      IP<int64_t>(out_l), IP<int64_t>(out_r), IP<int64_t>(out_ts), stream);
  });
  m.def("cpu_ijoin_expand", [](intptr_t cnt, intptr_t lb, intptr_t bkey, intptr_t bts,
                               intptr_t bval, int64_t n, intptr_t ots, intptr_t oval, int64_t no,
                               int side, int64_t p0, int64_t p1, intptr_t out_key, intptr_t out_l,
                               intptr_t out_r, intptr_t out_ts) {
    py::gil_scoped_release nogil;
    cpu::ijoin_expand(IP<uint64_t>(cnt), IP<int64_t>(lb), cols(bkey, bts, bval, n),
                      cols(0, ots, oval, no), side, p0, p1, IP<int64_t>(out_key),
                      IP<int64_t>(out_l), IP<int64_t>(out_r), IP<int64_t>(out_ts));
  });
  m.def("ijoin_merge", [](bool cuda, intptr_t okey, intptr_t ots, intptr_t oval, int64_t no,
                          intptr_t bkey, intptr_t bts, intptr_t bval, int64_t nb,
                          intptr_t out_key, intptr_t out_ts, intptr_t out_val, intptr_t stream) {
    const IJoinCols o = cols(okey, ots, oval, no), b = cols(bkey, bts, bval, nb);
    if (cuda) {
      gpu::ijoin_merge(o, b, IP<int64_t>(out_key), IP<int64_t>(out_ts), IP<int64_t>(out_val),
                       stream);
    } else {
      py::gil_scoped_release nogil;
      cpu::ijoin_merge(o, b, IP<int64_t>(out_key), IP<int64_t>(out_ts), IP<int64_t>(out_val));
    }
  });
  m.def("gpu_ijoin_keep", [](intptr_t ts, int64_t n, int64_t cutoff, intptr_t cnt,
                             intptr_t stream) {
    gpu::ijoin_keep(IP<int64_t>(ts), n, cutoff, IP<uint64_t>(cnt), stream);
  });
  m.def("gpu_ijoin_gather", [](intptr_t plan, int64_t n, int64_t nrows, intptr_t skey,
                               intptr_t sts, intptr_t sval, intptr_t out_key, intptr_t out_ts,
                               intptr_t out_val, intptr_t stream) {
    gpu::ijoin_gather(IP<int64_t>(plan), n, nrows, cols(skey, sts, sval, n), IP<int64_t>(out_key),
                      IP<int64_t>(out_ts), IP<int64_t>(out_val), stream);
  });
  m.def("cpu_ijoin_purge", [](intptr_t skey, intptr_t sts, intptr_t sval, int64_t n,
                              int64_t cutoff, intptr_t out_key, intptr_t out_ts,
                              intptr_t out_val) {
    return cpu::ijoin_purge(cols(skey, sts, sval, n), cutoff, IP<int64_t>(out_key),
                            IP<int64_t>(out_ts), IP<int64_t>(out_val));
  });
}
