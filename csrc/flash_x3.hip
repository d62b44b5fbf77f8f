// xdot — fp32 flash attention on the bf16 matrix pipe ("split-bf16", opt-in fp32 mode).
//
// The exact-fp32 family (csrc/flash_f32.hip) runs every product on v_mfma_f32_32x32x2_f32:
// 64 FLOP/clk/SIMD, 1/16 of the bf16 rate, so an fp32 step costs ~10x a bf16 one.  Here every
// fp32 operand x is split into two bf16 values, hi = bf16(x) and lo = bf16(x - hi) (x = hi + lo
// up to ~2^-17 |x|), and a product a·b is three bf16 MFMAs accumulated in fp32:
//     a·b ≈ a_lo·b_hi + a_hi·b_lo + a_hi·b_hi      (a_lo·b_lo ~ 2^-16 |a·b| dropped)
// = 3 x 32x32x16 bf16 MFMAs per 16-deep K step instead of 8 x 32x32x2 f32 ones: 5.3x fewer
// matrix-pipe cycles.  Softmax, LSE, δ and every accumulation stay fp32; measured against fp64
// the relative error is 6e-6..9e-6 (exact fp32: 3e-7..6e-7), profiles/r3_fp32_split.md.  Opt-in:
// ``XDOT_FP32_MODE=split``, per call ``fp32_mode=1``; the default ``exact`` keeps flash_f32.hip.
// ``split3`` (``fp32_mode=2``) is the same kernels with three parts per operand and six MFMAs per
// product (fp32-level error): the device code, templated on the split count, is flash_x3.h; this
// file instantiates the two-way kernels and holds the selectors, launchers and planners of both,
// flash_x6.hip instantiates the three-way ones.
//
// Same decomposition, layouts, masks and partial/combine protocol as flash_f32.hip (same
// reference semantics, distributed_dot_product/module.py:60-71): 4 waves x 32 rows (columns
// for the gathered-side kernel), 32-row tiles staged global -> VGPR (one tile ahead) -> LDS.
// The staging step splits each fp32 tile ONCE per workgroup into the bf16 images the MFMAs
// read:
//   * row-major  [row][d] hi / lo, stride D + 8 (16-byte pad: the 16-lane ds_read_b128 groups
//     hit 16 distinct bank quads) — A operand of products over the head dim;
//   * transposed [d][slot] hi / lo, stride 40 — A operand of products over the tile index,
//     slots permuted so that lane half h of K step j reads tile rows tidx(8j + t, h), t = 0..7,
//     i.e. the accumulator registers 8j..8j+7 of the previous product (B operand straight from
//     the accumulator, split in registers).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "flash_x3.h"

namespace {
namespace fa = xdot::fa;
namespace fa3 = xdot::fa3;
using fa::ColsMode;
using fa::Kern;
using fa::kern;

// ---- kernel selectors: the one place each (kernel, LDS) pair of this family is written; the
// launchers and the planners below both ask them (empty: no such kernel).  mode: BwdArgs /
// FwdArgs::fp32_mode, 1 two-way, 2 three-way (no S-buffer kernels: empty) ----
Kern<fa::FwdArgs> fwd_kern(int mode, int D, bool sbuf) {
  if (mode == 2) return sbuf ? Kern<fa::FwdArgs>{} : fa3::fwd_kern3(D);
  return fa::for_head_dim(D, Kern<fa::FwdArgs>{}, [&](auto d) {
    constexpr int DV = decltype(d)::value;
    return sbuf ? kern<fa3::fwd_kernel<DV, true>, fa3::FwdL<DV>::LDS_SB>() : kern<fa3::fwd_kernel<DV, false>, fa3::FwdL<DV>::LDS>();
  });
}
// reads_ds: the score-buffer modes (dS from the column kernel, Q image only)
Kern<fa::BwdArgs> rows_kern(int mode, int D, bool reads_ds) {
  if (mode == 2) return fa3::rows_kern3(D, reads_ds);
  return fa::for_head_dim(D, Kern<fa::BwdArgs>{}, [&](auto d) {
    constexpr int DV = decltype(d)::value;
    return reads_ds ? kern<fa3::bwd_rows_ds_kernel<DV>, fa3::RowsDsL<DV>::LDS>() : kern<fa3::bwd_rows_kernel<DV>, fa3::RowsL<DV>::LDS>();
  });
}
// the dQ pass over S / the single pass of the other modes.  dS-only at D = 128: the recompute
// kernel's two-image stages plus the transpose tiles exceed the 160 KiB of LDS (empty)
Kern<fa::BwdArgs> cols_kern(int fm, int D, ColsMode mode) {
  if (fm == 2) return mode == ColsMode::from_s ? Kern<fa::BwdArgs>{} : fa3::cols_kern3(D, mode == ColsMode::ds_only);
  return fa::for_head_dim(D, Kern<fa::BwdArgs>{}, [&](auto d) {
    constexpr int DV = decltype(d)::value;
    switch (mode) {
      case ColsMode::from_s: return kern<fa3::bwd_cols_kernel<DV, true>, fa3::ColsL<DV, true>::LDS>();
      case ColsMode::ds_only: return kern<fa3::bwd_cols_kernel<DV, false, true>, fa3::ColsL<DV, false, true>::LDS>();
      default: return kern<fa3::bwd_cols_kernel<DV, false>, fa3::ColsL<DV, false>::LDS>();
    }
  });
}
Kern<fa::BwdArgs> dv_kern(int D) {
  return fa::for_head_dim(D, Kern<fa::BwdArgs>{}, [&](auto d) {
    constexpr int DV = decltype(d)::value;
    return kern<fa3::bwd_cols_dv_kernel<DV>, fa3::DvL<DV>::LDS>();
  });
}
}  // namespace

extern "C" int xdot_flash_fwd_x3_launch(const xdot::fa::FwdArgs* a, int D, hipStream_t st) {
  if (a->R == 0 || a->B == 0 || a->H == 0 || a->prescaled) return a->prescaled ? -1 : 0;
  const auto k = fwd_kern(a->fp32_mode, D, a->sbuf != nullptr);
  if (!k) return -1;
  k.launch(dim3(((a->R + 127) / 128) * a->B * a->H * a->nsplit), st, *a);
  return 0;
}

extern "C" int xdot_flash_bwd_rows_x3_launch(const xdot::fa::BwdArgs* a, int D, hipStream_t st) {
  if (a->R == 0 || a->B == 0 || a->H == 0 || a->T == 0) return 0;
  const auto k = rows_kern(a->fp32_mode, D, a->sbuf || a->dsbuf);
  if (a->prescaled || !k) return -1;
  k.launch(dim3(((a->R + 127) / 128) * a->B * a->H * a->nsplit), st, *a);
  return 0;
}

extern "C" int xdot_flash_bwd_cols_x3_launch(const xdot::fa::BwdArgs* a, int D, hipStream_t st) {
  if (a->R == 0 || a->B == 0 || a->H == 0 || a->T == 0) return 0;
  if (a->prescaled || a->dkv16) return -1;
  const int W = ((a->T + 127) / 128) * a->B * a->H, sq = a->csq > 1 ? a->csq : 1, sv = a->csv > 1 ? a->csv : 1;
  if ((sq > 1 && (!a->cpq || (!a->sbuf && !a->cpv))) || (sv > 1 && !a->cpv) || (D & 3)) return -1;
  const ColsMode mode = fa::cols_mode(*a, false);
  const auto kq = cols_kern(a->fp32_mode, D, mode), kv = dv_kern(D);
  if (!kq || !kv) return -1;
  // split partials of a pass summed into its grad half (BwdArgs::csq / csv); a single-pass kernel
  // writes both halves in sq pieces
  const bool two_pass = mode == ColsMode::from_s;
  const int64_t rows = (int64_t)a->B * a->T;
  const int C = a->H * D, nv = two_pass ? sv : sq;
  fa::run_cols_passes(
      two_pass, a->sb_passes, a->dsbuf != nullptr, [&] { kq.launch(dim3(W * sq), st, *a); },
      [&] { kv.launch(dim3(W * sv), st, *a); },
      [&] {
        if (sq > 1) xdot_flash_cols_sum_launch(a->cpq, a->dkc, sq, rows, C, a->ldg, xdot::DT_F32, st);
      },
      [&] {
        if (nv > 1) xdot_flash_cols_sum_launch(a->cpv, a->dvc, nv, rows, C, a->ldg, xdot::DT_F32, st);
      });
  return 0;
}

extern "C" int xdot_flash_cols_splits_x3(const xdot::fa::BwdArgs* a, int D, int* sq, int* sv) {
  *sq = *sv = 1;
  const int e = fa::env_int("XDOT_CSPLIT", 1, 4);  // as in flash_f32.hip, <= 4
  if (e >= 0) {
    *sq = *sv = (a->R + 31) / 32 / e >= 1 ? e : 1;
    return 0;
  }
  const ColsMode mode = fa::cols_mode(*a, false);
  const auto kq = cols_kern(a->fp32_mode, D, mode), kv = dv_kern(D);
  if (!kq || !kv) return -1;
  const int64_t W = (int64_t)((a->T + 127) / 128) * a->B * a->H;
  const int NRT = (a->R + 31) / 32;
  *sq = fa::csplit_cols(W, NRT, kq.slots());
  *sv = mode == ColsMode::from_s ? fa::csplit_cols(W, NRT, kv.slots()) : *sq;
  return 0;
}

// column splits of the split-bf16 forward (kernel 0) / row-side backward (1) of family `mode` (1 two-way,
// 2 three-way), see kernels.h
extern "C" int xdot_flash_f32_row_splits_x3(int kernel, int mode, int D, bool sbuf, int64_t W, int64_t T) {
  const int slots = kernel == 0 ? fwd_kern(mode, D, sbuf).slots() : rows_kern(mode, D, sbuf).slots();
  if (!slots) return 0;
  return fa::csplit_f32_rows(W, (int)((T + 31) / 32), slots);
}
