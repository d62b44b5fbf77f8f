// xdot — the small host helpers the torch binding translation units (bindings*.cpp) share.
#pragma once
#include <torch/library.h>
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "row_view.h"

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

// a contiguous fp32 (B, H, R) tensor (lse, lse2, delta) on the launch's device
inline void check_bhr(const at::Tensor& t, int64_t B, int64_t H, int64_t R, const at::Device& dev, const char* what) {
  TORCH_CHECK(t.is_contiguous() && t.scalar_type() == at::kFloat && t.numel() == B * H * R && t.device() == dev, what);
}

// one (B, R, C) operand of a row-wise op (row_view.h): on like's GPU, of like's dtype, unit inner stride,
// non-negative row / batch strides, inside its storage; `written`: its rows may not overlap either
inline RowView row_view(const at::Tensor& t, int64_t B, int64_t R, int64_t C, const at::Tensor& like, bool written,
                        const char* op, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device() && t.scalar_type() == like.scalar_type() && t.dim() == 3 &&
                  t.size(0) == B && t.size(1) == R && t.size(2) == C,
              "xdot.", op, ": ", name, " must be a (", B, ", ", R, ", ", C, ") tensor of the op's dtype on the same GPU");
  RowView v;
  const auto err = xdot::row_view(B, R, C, t.strides().data(), avail_elems(t), (int64_t)t.element_size(),
                                  reinterpret_cast<uintptr_t>(t.data_ptr()), written, &v);
  TORCH_CHECK(err != RowViewErr::inner_stride, "xdot.", op, ": the last dimension of ", name, " must have stride 1");
  TORCH_CHECK(err != RowViewErr::negative_stride, "xdot.", op, ": negative strides in ", name);
  TORCH_CHECK(err != RowViewErr::rows_overlap, "xdot.", op, ": the rows of ", name, " overlap");
  TORCH_CHECK(err != RowViewErr::out_of_bounds, "xdot.", op, ": view ", name, " out of bounds");
  return v;
}

// the rotation table of a row-wise op: cos and sin both (-> true) or neither (-> false), contiguous fp32
// (R, D/2) on `dev`
inline bool rot_table(const c10::optional<at::Tensor>& cosb, const c10::optional<at::Tensor>& sinb, int64_t R, int64_t D,
                      const at::Device& dev, const char* op) {
  const bool hc = cosb.has_value() && cosb->defined(), hs = sinb.has_value() && sinb->defined();
  TORCH_CHECK(hc == hs, "xdot.", op, ": cos and sin go together");
  if (!hc) return false;
  TORCH_CHECK(D % 2 == 0, "xdot.", op, ": the rotation needs an even head dim, got ", D);
  TORCH_CHECK(cosb->is_cuda() && cosb->device() == dev && sinb->device() == dev && cosb->scalar_type() == at::kFloat &&
                  sinb->scalar_type() == at::kFloat && cosb->is_contiguous() && sinb->is_contiguous() &&
                  cosb->dim() == 2 && cosb->size(0) == R && cosb->size(1) == D / 2 && sinb->sizes() == cosb->sizes(),
              "xdot.", op, ": cos / sin must be contiguous fp32 (R, D/2) on the same GPU");
  return true;
}

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
