// xdot — fp32 flash attention on the bf16 matrix pipe with fp32-level error ("split3", opt-in:
// ``XDOT_FP32_MODE=split3``, per call ``fp32_mode=2``).
//
// The kernels of flash_x3.h with three bf16 parts per fp32 operand, x = h + m + l (all 24 mantissa
// bits), and six bf16 MFMAs per product, smallest terms first:
//     a·b ≈ a_l·b_h + a_h·b_l + a_m·b_m + a_m·b_h + a_h·b_m + a_h·b_h     (m·l, l·m, l·l <= 2^-25 dropped)
// (products over the head dim keep the five small terms in an accumulator of their own, added once at
// the end: flash_x3.h rowprod)
// = 6 x 32x32x16 bf16 MFMAs per 16-deep K step where the exact family (flash_f32.hip) runs
// 8 x 32x32x2 f32 ones at 1/16 the rate.  What is dropped lies below the rounding of the fp32
// accumulation, so the error against fp64 is that of the exact family (profiles/split3.md), not the
// 6e-6..9e-6 of the two-way split.
//
// Instantiated here: the kernels of the family's default schedule.  The forward without a score
// store, the recompute column kernel with and without the dS store, the recompute row kernel and
// the row kernel that reads dS.  There is no S buffer in this mode (the bindings refuse one): the
// S-buffer kernels of flash_x3.hip have no three-way form.
//
// Sizes (LDS = 2 stages of 3 planes per image; registers per lane from the compiler's resource
// report, profiles/split3.md; nothing spills to scratch):
//   forward        D <= 96: 72 KiB, two workgroups per CU;  D = 128: 120 KiB, one
//   column kernel  one workgroup per CU at every D: the resident q and v fragments are
//                  2 x 3 x D/16 x 4 VGPRs (192 at D = 128) beside 2 x D/32 x 16 pinned accumulator
//                  AGPRs; + 16 KiB of transpose tiles with the dS store (D = 128: 136.5 KiB)
//   row kernel     D <= 64 two per CU, above one (k and dO fragments resident, dK pinned)
//   dS row kernel  one image: 2 x 3 planes, two per CU
// This file alone is compiled without packed fp32 VALU instructions (xdot/build.py).
#include "flash_x3.h"

namespace xdot {
namespace fa3 {

fa::Kern<fa::FwdArgs> fwd_kern3(int D) {
  return fa::for_head_dim(D, fa::Kern<fa::FwdArgs>{}, [&](auto d) {
    constexpr int DV = decltype(d)::value;
    return fa::kern<fwd_kernel<DV, false, 3>, FwdL<DV, 3>::LDS>();
  });
}

fa::Kern<fa::BwdArgs> rows_kern3(int D, bool reads_ds) {
  return fa::for_head_dim(D, fa::Kern<fa::BwdArgs>{}, [&](auto d) {
    constexpr int DV = decltype(d)::value;
    return reads_ds ? fa::kern<bwd_rows_ds_kernel<DV, 3>, RowsDsL<DV, 3>::LDS>() : fa::kern<bwd_rows_kernel<DV, 3>, RowsL<DV, 3>::LDS>();
  });
}

fa::Kern<fa::BwdArgs> cols_kern3(int D, bool stores_ds) {
  return fa::for_head_dim(D, fa::Kern<fa::BwdArgs>{}, [&](auto d) {
    constexpr int DV = decltype(d)::value;
    return stores_ds ? fa::kern<bwd_cols_kernel<DV, false, true, 3>, ColsL<DV, false, true, 3>::LDS>()
                     : fa::kern<bwd_cols_kernel<DV, false, false, 3>, ColsL<DV, false, false, 3>::LDS>();
  });
}

}  // namespace fa3
}  // namespace xdot
