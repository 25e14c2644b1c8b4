// mxstream — pybind11 bindings of the keyed state-machine kernels (csrc/fsm_hip.hip) and their
// C++ twin (csrc/fsm_cpu.cpp). Addresses are passed as integers (tensor data_ptr()); dtypes,
// sizes and contiguity are checked by the Python caller (ops/kernels.py fsm_*) before any
// launch. The rule arrives as three short sequences and is checked here (fsm_rule) on both
// paths.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <vector>

#include "mxs_fsm.h"
#include "mxs_runtime.h"

namespace py = pybind11;
using namespace mxs;

namespace {

template <class T>
T* TP(intptr_t p) {
  return reinterpret_cast<T*>(p);
}

FsmRule rule_of(const std::vector<double>& bounds, const std::vector<uint64_t>& cols,
                const std::vector<uint32_t>& report, int initial, int kind) {
  if (cols.empty() || cols.size() > (size_t)kFsmMaxClasses || bounds.size() + 1 != cols.size())
    throw std::invalid_argument("fsm: 1 to 16 table columns, one more than bounds");
  if (report.empty() || report.size() > (size_t)kFsmMaxStates)
    throw std::invalid_argument("fsm: 1 to 16 report masks, one per state");
  return fsm_rule(bounds.data(), cols.data(), report.data(), (int)report.size(),
                  (int)cols.size(), initial, kind);
}

}  // namespace

void bind_fsm(py::module_& m) {
  m.attr("FSM_NONE") = kFsmNone;
  m.attr("FSM_MAX_STATES") = kFsmMaxStates;
  m.attr("FSM_MAX_CLASSES") = kFsmMaxClasses;
  m.attr("FSM_TAG_BITS") = kFsmTagBits;
  // The device scan takes the batch sorted by key (skeys, perm = arrival index of each sorted
  // row); the twin takes it in arrival order.
  m.def("gpu_fsm_scan", [](intptr_t skeys, intptr_t perm, intptr_t vals, intptr_t ts, int64_t n,
                           const std::vector<double>& bounds, const std::vector<uint64_t>& cols,
                           const std::vector<uint32_t>& report, int initial, int kind,
                           intptr_t state, int64_t cap, intptr_t out_tag, intptr_t out_since,
                           intptr_t out_n, intptr_t stream) {
    gpu::fsm_scan(TP<const int64_t>(skeys), TP<const int64_t>(perm), TP<const int64_t>(vals),
                  TP<const int64_t>(ts), n, rule_of(bounds, cols, report, initial, kind),
                  TP<int64_t>(state), cap, TP<int64_t>(out_tag), TP<int64_t>(out_since),
                  TP<uint32_t>(out_n), stream);
  });
  m.def("gpu_fsm_gather", [](intptr_t tags, intptr_t since, int64_t rows, intptr_t keys,
                             intptr_t vals, intptr_t ts, int64_t n, intptr_t out_key,
                             intptr_t out_code, intptr_t out_since, intptr_t out_val,
                             intptr_t out_ts, intptr_t stream) {
    gpu::fsm_gather(TP<const int64_t>(tags), TP<const int64_t>(since), rows,
                    TP<const int64_t>(keys), TP<const int64_t>(vals), TP<const int64_t>(ts), n,
                    TP<int64_t>(out_key), TP<int64_t>(out_code), TP<int64_t>(out_since),
                    TP<int64_t>(out_val), TP<int64_t>(out_ts), stream);
  });
  m.def("cpu_fsm_update", [](intptr_t keys, intptr_t vals, intptr_t ts, int64_t n,
                             const std::vector<double>& bounds, const std::vector<uint64_t>& cols,
                             const std::vector<uint32_t>& report, int initial, int kind,
                             intptr_t state, int64_t cap, intptr_t out_key, intptr_t out_code,
                             intptr_t out_since, intptr_t out_val, intptr_t out_ts) {
    return cpu::fsm_update(TP<const int64_t>(keys), TP<const int64_t>(vals),
                           TP<const int64_t>(ts), n, rule_of(bounds, cols, report, initial, kind),
                           TP<int64_t>(state), cap, TP<int64_t>(out_key), TP<int64_t>(out_code),
                           TP<int64_t>(out_since), TP<int64_t>(out_val), TP<int64_t>(out_ts));
  });
}
