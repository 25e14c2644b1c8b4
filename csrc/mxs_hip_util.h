// mxstream — the small host-side helpers every .hip unit needs: the HIP error check, the 16-byte
// store type and the grid size of a striding kernel. Included from .hip files only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

namespace mxs {

#define MXS_HIP_CHECK(x)                                                                    \
  do {                                                                                      \
    hipError_t e_ = (x);                                                                    \
    if (e_ != hipSuccess)                                                                   \
      throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(e_) + " at " + \
                               __FILE__ + ":" + std::to_string(__LINE__));                  \
  } while (0)

typedef long long ll2 __attribute__((ext_vector_type(2)));

// Workgroups for n items at `per_block` each: at least 1, at most `cap` (the kernels stride).
inline int grid_of(int64_t n, int per_block, int cap) {
  int64_t g = (n + per_block - 1) / per_block;
  if (g < 1) g = 1;
  return (int)(g < cap ? g : cap);
}

}  // namespace mxs
