// xdot — host side of the flash kernel files: one handle per kernel instantiation that both the
// launcher and the grid planner go through, the runtime -> compile-time dispatch of head dim and
// dtype, and the pass order of a score-buffer column launch.  No device code.
#pragma once
#include "flash_common.h"

namespace xdot {
namespace fa {

// Resident 256-thread workgroups per CU of ONE kernel instantiation with LDS bytes of dynamic LDS.
// One static per (kernel, LDS): the answer never depends on which kernel was asked about first.
template <auto Kernel, int LDS> int resident_wgs() {
  static const int v = [] {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(Kernel), 256, LDS) != hipSuccess || n < 1)
      n = 1;
    return n;
  }();
  return v;
}

// A flash kernel (256 threads, one args struct by value) together with its dynamic LDS size: what a
// launch and an occupancy query both need.  Empty = the configuration has no kernel; the selectors of
// the family files return it and their callers refuse the launch / the plan.
template <class Args> struct Kern {
  void (*fn)(Args) = nullptr;
  int lds = 0;
  int (*occ)() = nullptr;
  explicit operator bool() const { return fn != nullptr; }
  void launch(dim3 grid, hipStream_t st, const Args& a) const {
    void* args[] = {const_cast<Args*>(&a)};
    (void)hipLaunchKernel(reinterpret_cast<const void*>(fn), grid, dim3(256), args, (size_t)lds, st);
  }
  int wgs_per_cu() const { return occ ? occ() : 0; }
  int slots() const { return wgs_per_cu() * xdot_num_cus(); }  // resident workgroups of the whole GPU
};
template <class A> A kern_args(void (*)(A));
// the handle of Kernel at LDS bytes; empty where that exceeds the 160 KiB of a CU (no such launch)
template <auto Kernel, int LDS> auto kern() {
  using K = Kern<decltype(kern_args(Kernel))>;
  if constexpr (LDS > 160 * 1024) return K{};
  else return K{Kernel, LDS, &resident_wgs<Kernel, LDS>};
}

// ---- runtime value -> template argument ---------------------------------------------------------
// f(Ic<D>{}) for the head dim D of the set, `none` for any other
template <class R, class F> R for_head_dim(int D, R none, F&& f) {
  switch (D) {
    case 32: return f(Ic<32>{});
    case 64: return f(Ic<64>{});
    case 96: return f(Ic<96>{});
    case 128: return f(Ic<128>{});
    default: return none;
  }
}
// the wide heads of flash_wide.hip
template <class R, class F> R for_wide_head_dim(int D, R none, F&& f) {
  switch (D) {
    case 160: return f(Ic<160>{});
    case 192: return f(Ic<192>{});
    case 256: return f(Ic<256>{});
    case 384: return f(Ic<384>{});
    default: return none;
  }
}
// f(Ic<DT>{}, Ic<D>{}) for a 16-bit dtype and a head dim <= 128 ...
template <class R, class F> R for_dtype16_head_dim(int dt, int D, R none, F&& f) {
  switch (dt) {
    case DT_BF16: return for_head_dim(D, none, [&](auto d) -> R { return f(Ic<DT_BF16>{}, d); });
    case DT_F16: return for_head_dim(D, none, [&](auto d) -> R { return f(Ic<DT_F16>{}, d); });
    default: return none;
  }
}
// ... and with the wide heads as well (the helpers templated on D alone: prep, combine, partial sums)
template <class R, class F> R for_dtype16_any_head_dim(int dt, int D, R none, F&& f) {
  if (D <= 128) return for_dtype16_head_dim(dt, D, none, f);
  switch (dt) {
    case DT_BF16: return for_wide_head_dim(D, none, [&](auto d) -> R { return f(Ic<DT_BF16>{}, d); });
    case DT_F16: return for_wide_head_dim(D, none, [&](auto d) -> R { return f(Ic<DT_F16>{}, d); });
    default: return none;
  }
}

// ---- column launch of the score-buffer families (exact fp32, split-bf16, wide) ------------------
// What a D <= 128 fp32 column launch does, from the mode fields of its args (kernels.h): recompute S;
// recompute S and store dS for the row kernel; read S in two passes (dQ: S -> dS, and dV); or the
// fused pass over S (exact fp32 only: `has_fused`).
enum class ColsMode { recompute, ds_only, from_s, fused };
inline ColsMode cols_mode(const BwdArgs& a, bool has_fused) {
  if (a.sbuf) return has_fused && a.sb_passes == 4 ? ColsMode::fused : ColsMode::from_s;
  return a.dsbuf ? ColsMode::ds_only : ColsMode::recompute;
}

// The order of a column launch's kernels and partial sums.
// two_pass (from_s, and every wide launch): dQ and dV come from two kernels, sb_passes says which run
// (bit 0 the dV pass, bit 1 the dQ pass, 0: both).  In place the dQ pass overwrites S with dS, so the
// dV pass goes first; with a dS buffer the dQ pass goes first (the dV pass can then overlap the row
// kernel).  Each pass is followed by the sum of its split partials.
// !two_pass: ONE launch (dq) writes both gradients (recompute, dS-only and fused kernels), then both sums.
template <class LQ, class LV, class SQ, class SV>
void run_cols_passes(bool two_pass, int sb_passes, bool ds_buffer, LQ&& dq, LV&& dv, SQ&& sum_q, SV&& sum_v) {
  if (!two_pass) {
    dq();
    sum_q();
    sum_v();
    return;
  }
  const int ps = sb_passes ? sb_passes : 3;
  const bool dv_first = !ds_buffer;
  if ((ps & 1) && dv_first) {
    dv();
    sum_v();
  }
  if (ps & 2) {
    dq();
    sum_q();
  }
  if ((ps & 1) && !dv_first) {
    dv();
    sum_v();
  }
}

}  // namespace fa
}  // namespace xdot
