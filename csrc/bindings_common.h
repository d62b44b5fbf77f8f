// xdot — the small host helpers the torch binding translation units (bindings*.cpp) share.
#pragma once
#include <torch/library.h>
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include "kernels.h"

#include <rocprofiler-sdk-roctx/roctx.h>

#include <cstdlib>

namespace xdot {
namespace bind {

// roctx ranges around every op (visible in rocprofv3 --marker-trace timelines); enabled by
// XDOT_ROCTX=1 so the default path pays one predictable branch.
inline bool roctx_on() {
  static const bool v = [] {
    const char* e = std::getenv("XDOT_ROCTX");
    return e && e[0] == '1';
  }();
  return v;
}
struct Range {
  bool on;
  explicit Range(const char* name) : on(roctx_on()) { if (on) roctxRangePushA(name); }
  ~Range() { if (on) roctxRangePop(); }
};

inline int dt_code(at::ScalarType t) {
  switch (t) {
    case at::kFloat: return xdot::DT_F32;
    case at::kBFloat16: return xdot::DT_BF16;
    case at::kHalf: return xdot::DT_F16;
    default: TORCH_CHECK(false, "xdot: unsupported dtype ", t);
  }
  return -1;
}

inline hipStream_t cur_stream(const at::Tensor& t) { return c10::hip::getCurrentHIPStream(t.device().index()).stream(); }

// elements addressable from t.data_ptr() to the end of its storage
inline int64_t avail_elems(const at::Tensor& t) {
  const int64_t bytes = (int64_t)t.storage().nbytes() - t.storage_offset() * (int64_t)t.element_size();
  return bytes / (int64_t)t.element_size();
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline void check_launch(hipError_t e, const char* what) {
  TORCH_CHECK(e == hipSuccess, "xdot: ", what, " launch failed: ", hipGetErrorString(e));
}

// the launcher took the configuration (else "xdot.<op>: <why>") and the launch itself succeeded
inline void launched(int rc, const char* op, const char* why = "config") {
  TORCH_CHECK(rc == 0, "xdot.", op, ": ", why);
  check_launch(hipGetLastError(), op);
}

}  // namespace bind
}  // namespace xdot
