// mxstream — pybind11 bindings of the rule-set kernels (csrc/ruleset_hip.hip) and their C++ twins
// (csrc/ruleset_cpu.cpp). Addresses are passed as integers (tensor data_ptr()); dtypes, sizes and
// contiguity are checked by the Python caller (ops/kernels.py ruleset_*) before any launch.
#include <pybind11/pybind11.h>

#include "mxs_ruleset.h"
#include "mxs_runtime.h"

namespace py = pybind11;
using namespace mxs;

namespace {

template <class T>
T* RP(intptr_t p) {
  return reinterpret_cast<T*>(p);
}

}  // namespace

void bind_ruleset(py::module_& m) {
  m.attr("RULESET_MAX") = kRuleSetMax;
  m.attr("RULESET_GROUPS") = kRuleSetGroups;
  m.def("ruleset_count", [](bool cuda, intptr_t vals, int64_t n, intptr_t rules, intptr_t gsum,
                            intptr_t counts, intptr_t stream) {
    if (cuda) {
      gpu::ruleset_count(RP<const int64_t>(vals), n, RP<const int64_t>(rules), RP<uint32_t>(gsum),
                         RP<uint32_t>(counts), stream);
    } else {
      py::gil_scoped_release nogil;
      cpu::ruleset_count(RP<const int64_t>(vals), n, RP<const int64_t>(rules), RP<uint32_t>(gsum),
                         RP<uint32_t>(counts));
    }
  });
  m.def("ruleset_emit", [](bool cuda, intptr_t keys, intptr_t vals, intptr_t ts, int64_t n,
                           intptr_t rules, intptr_t gsum, intptr_t counts, intptr_t offsets,
                           int64_t total, intptr_t out_key, intptr_t out_val, intptr_t out_rule,
                           intptr_t out_thr, intptr_t out_ts, intptr_t stream) {
    if (cuda) {
      gpu::ruleset_emit(RP<const int64_t>(keys), RP<const int64_t>(vals), RP<const int64_t>(ts), n,
                        RP<const int64_t>(rules), RP<const uint32_t>(gsum),
                        RP<const uint32_t>(counts), RP<const int64_t>(offsets), total,
                        RP<int64_t>(out_key), RP<int64_t>(out_val), RP<int64_t>(out_rule),
                        RP<int64_t>(out_thr), RP<int64_t>(out_ts), stream);
    } else {
      py::gil_scoped_release nogil;
      cpu::ruleset_emit(RP<const int64_t>(keys), RP<const int64_t>(vals), RP<const int64_t>(ts), n,
                        RP<const int64_t>(rules), total, RP<int64_t>(out_key),
                        RP<int64_t>(out_val), RP<int64_t>(out_rule), RP<int64_t>(out_thr),
                        RP<int64_t>(out_ts));
    }
  });
}
