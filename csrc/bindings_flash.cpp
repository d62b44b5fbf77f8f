// xdot — torch bindings of the flash-attention kernels (schemas: TORCH_LIBRARY in bindings.cpp).
//
// How many splits a launch takes and whether it runs on the head-heavy grid is decided by plan_fwd /
// plan_rows / plan_cols, from the host-only models of flash_plan.h and the occupancy of the very kernel
// the launcher would pick (the kernel selectors of the family files, flash_launch.h); the flash_*_plan
// ops return those functions' answers without launching anything.
#include "bindings_common.h"
#include "flash_plan.h"

#include <vector>

namespace {

using namespace xdot::bind;
using namespace xdot::fa;
using OptT = c10::optional<at::Tensor>;

// C: row-side columns H*D; Cg: gathered-side columns Hg*D (Hg = H / G gathered heads, G row heads each)
struct FlashGeom { int64_t B, R, C, T, D, ld, Cg, G; };

// rows: contiguous (B, R, C).  kc / vc: (B, T, C) views with unit inner stride and a common
// row stride `ld` (C for separate tensors, 2C for the two halves of a packed [q | v]).
// `bits`: the kt-major (B, NKT, R) words, or with colmajor the (B, NRT, Tpad) words of the
// backward column kernel (mask_pack's third output).  Hg: gathered heads (0: H); Hg < H is grouped-query
// attention, row head h reads gathered head h / (H / Hg)
FlashGeom flash_check(const at::Tensor& rows, const at::Tensor& kc, const at::Tensor& vc, int64_t H, const OptT& bits,
                      const OptT& flags, bool colmajor = false, int64_t Hg = 0) {
  TORCH_CHECK(rows.is_cuda() && kc.is_cuda() && vc.is_cuda(), "xdot.flash: GPU tensors required");
  TORCH_CHECK(rows.is_contiguous(), "xdot.flash: rows must be contiguous");
  TORCH_CHECK(rows.scalar_type() == kc.scalar_type() && rows.scalar_type() == vc.scalar_type(), "xdot.flash: dtype mismatch");
  TORCH_CHECK(rows.scalar_type() == at::kBFloat16 || rows.scalar_type() == at::kHalf || rows.scalar_type() == at::kFloat,
              "xdot.flash: bf16/fp16/fp32 only");
  TORCH_CHECK(rows.dim() == 3 && kc.dim() == 3 && vc.sizes() == kc.sizes(), "xdot.flash: rows (B,R,C), cols (B,T,C)");
  FlashGeom g{rows.size(0), rows.size(1), rows.size(2), kc.size(1), 0, kc.stride(1), 0, 1};
  TORCH_CHECK(H > 0 && g.C % H == 0, "xdot.flash: C not divisible by heads");
  const int64_t hg = Hg > 0 ? Hg : H;
  TORCH_CHECK(hg <= H && H % hg == 0, "xdot.flash: the heads H = ", H, " must be a multiple of the gathered heads Hg = ", hg);
  g.D = g.C / H;
  g.Cg = hg * g.D;
  g.G = H / hg;
  TORCH_CHECK(kc.size(0) == g.B, "xdot.flash: batch mismatch");
  TORCH_CHECK(kc.size(2) == g.Cg, "xdot.flash: the gathered side must have Hg * D = ", g.Cg, " columns (Hg = ", hg,
              ", D = ", g.D, "), got ", kc.size(2));
  TORCH_CHECK(g.G == 1 || H <= 1024, "xdot.flash: grouped gathered heads take at most 1024 heads");
  TORCH_CHECK(g.G == 1 || (rows.scalar_type() != at::kFloat && g.D <= 128),
              "xdot.flash: grouped gathered heads (Hg < H) run in the 16-bit kernels with head dim <= 128 only");
  TORCH_CHECK(g.T > 0, "xdot.flash: empty key side");
  for (const at::Tensor* t : {&kc, &vc}) {
    TORCH_CHECK(t->stride(2) == 1 && t->stride(1) == g.ld && (g.B == 1 || t->stride(0) == g.T * g.ld),
                "xdot.flash: key/value side must be (B, T, C) rows with a common row stride");
    TORCH_CHECK((g.B - 1) * g.T * g.ld + (g.T - 1) * g.ld + g.Cg <= avail_elems(*t), "xdot.flash: key/value out of bounds");
  }
  TORCH_CHECK(g.ld % 8 == 0 && g.ld >= g.Cg, "xdot.flash: row stride must be a multiple of 8 elements");
  TORCH_CHECK(g.D == 32 || g.D == 64 || g.D == 96 || g.D == 128 || g.D == 160 || g.D == 192 || g.D == 256 ||
                  g.D == 384,
              "xdot.flash: head dim must be 32/64/96/128 or (flash_wide.hip) 160/192/256/384");
  TORCH_CHECK(g.T < (1LL << 31) && g.R < (1LL << 31) && g.B * H * ((g.R + 127) / 128) * 8 < (1LL << 31), "xdot.flash: too large");
  TORCH_CHECK(aligned16(rows.data_ptr()) && aligned16(kc.data_ptr()) && aligned16(vc.data_ptr()), "xdot.flash: 16-byte alignment");
  const bool hb = bits.has_value() && bits->defined(), hf = flags.has_value() && flags->defined();
  TORCH_CHECK(hb == hf, "xdot.flash: mask bits and flags go together");
  if (hb) {
    const int64_t NKT = (g.T + 63) / 64;
    const int64_t nwords = colmajor ? g.B * ((g.R + 63) / 64) * ((g.T + 127) / 128 * 128) : g.B * g.R * NKT;
    TORCH_CHECK(bits->is_contiguous() && bits->numel() == nwords && bits->element_size() == 8,
                colmajor ? "xdot.flash_bwd_cols: mask needs the column-major bits (mask_pack output 3)"
                         : "xdot.flash: mask bits shape");
    TORCH_CHECK(flags->is_contiguous() && flags->numel() == g.B * ((g.R + 31) / 32) * ((NKT + 3) & ~3),
                "xdot.flash: mask flags shape");
    TORCH_CHECK((reinterpret_cast<uintptr_t>(flags->data_ptr()) & 3) == 0, "xdot.flash: flags alignment");
  }
  return g;
}

// the geometry of a plan query: no tensors
FlashGeom query_geom(int64_t B, int64_t R, int64_t T, int64_t H, int64_t D) {
  TORCH_CHECK(B > 0 && R > 0 && T > 0 && H > 0 && D > 0 && T < (1LL << 31) && R < (1LL << 31), "xdot.flash: plan query shape");
  return FlashGeom{B, R, H * D, T, D, H * D, H * D, 1};
}

// fp32 score buffer (flash_f32.hip exact, flash_x3.hip split): (B*H, ceil(R/32), ceil(T/32)) blocks
// of 1024 floats.  ds: the dS buffer, which split3 (fp32_mode 2) takes too; it keeps no S buffer
float* sbuf_ptr(const OptT& sbuf, const FlashGeom& g, int64_t H, const at::Tensor& rows, int64_t fp32_mode,
                const char* what, bool ds = false) {
  if (!sbuf.has_value() || !sbuf->defined()) return nullptr;
  const auto& t = *sbuf;
  TORCH_CHECK(rows.scalar_type() == at::kFloat && fp32_mode >= 0 && fp32_mode <= 2, what,
              ": the score buffer is an fp32 (exact, split or split3) feature");
  TORCH_CHECK(ds || fp32_mode != 2, what,
              ": fp32_mode 2 (split3) keeps no S buffer (sbuf); it takes a dS buffer (dsbuf) or recomputes");
  const int64_t need = (g.B * H * ((g.R + 31) / 32) * ((g.T + 31) / 32) + 1) * 1024;  // + the dump block
  TORCH_CHECK(t.is_cuda() && t.device() == rows.device() && t.scalar_type() == at::kFloat && t.is_contiguous() &&
                  t.numel() == need && aligned16(t.data_ptr()),
              what, ": score buffer must be a contiguous fp32 device tensor of ", need, " elements");
  return t.data_ptr<float>();
}

// ---- grid planning -----------------------------------------------------------------------
// nsplit column splits of `blocks` row blocks; heavy: per XCD `whole` row blocks run unsplit, only the
// last `rem` in nsplit pieces
struct FwdPlan { int nsplit; bool heavy; int whole, rem; int64_t blocks; };

// Column splits / grid of a forward launch.  Precedence: a forced nsplit; else the 16-bit model
// (head-heavy where it wins), overridden for fp32 by the occupancy model (exact fp32: head-heavy
// where it beats that split) and for D > 128 by the wide model.
FwdPlan plan_fwd(const FlashGeom& g, int64_t H, at::ScalarType dtype, int64_t fp32_mode, bool has_sbuf, int64_t nsplit) {
  const int rpw = xdot_flash_fwd_rows_per_wg();
  const int64_t NB = ((g.R + rpw - 1) / rpw) * g.B * H, nkt = (g.T + 63) / 64;
  // forced: clamped through the forward's block count and 512 slots (the row side passes 1 and 1)
  if (nsplit != 0) return {pick_split(NB, g.T, 512, nsplit), false, 0, 0, NB};
  FwdPlan p{1, false, 0, 0, NB};
  int hs = 0;
  p.heavy = dtype != at::kFloat && g.D <= 128 &&
            head_heavy_plan(NB, nkt, 64, pick_split(NB, g.T, 8 * 64, 0), &p.whole, &p.rem, &hs);
  p.nsplit = p.heavy ? hs : pick_split(NB, g.T, 512, 0);
  if (dtype == at::kFloat) {  // fp32 kernels: their own occupancy / tile model
    const int f = xdot_flash_f32_row_splits(0, (int)fp32_mode, (int)g.D, has_sbuf, NB, g.T);
    if (f > 0) p.nsplit = f;
    // exact fp32 (D <= 128): the head-heavy grid when the round model prefers it over that split
    const int occ = fp32_mode == 0 && g.D <= 128 && f32_heavy() ? xdot_flash_f32_fwd_occ((int)g.D, has_sbuf) : 0;
    if (occ > 0 && head_heavy_plan(NB, nkt, (int64_t)occ * (xdot_num_cus() / 8), p.nsplit, &p.whole, &p.rem, &hs)) {
      p.heavy = true;
      p.nsplit = hs;
    }
  }
  if (g.D > 128) {  // wide kernels (one workgroup per CU): their own occupancy, told of the score buffer
    const int f = xdot_flash_wide_splits(0, dt_code(dtype), (int)g.D, has_sbuf, NB, (g.T + 31) / 32);
    if (f > 0) p.nsplit = f;
  }
  return p;
}

// Column splits of a row-side backward launch: a forced nsplit; else rows_split, overridden for
// fp32 by the occupancy model and for D > 128 by the wide model.
int plan_rows(const FlashGeom& g, int64_t H, at::ScalarType dtype, int64_t fp32_mode, bool has_score_or_ds_buf,
              bool has_sbuf, int64_t nsplit) {
  // forced: clamped through 1 block and 1 slot (the forward passes its block count and 512)
  if (nsplit > 0) return pick_split(1, g.T, 1, nsplit);
  int ns = rows_split(g.B, g.R, g.T, H);
  if (nsplit != 0) return ns;
  const int64_t W = ((g.R + 127) / 128) * g.B * H;
  if (dtype == at::kFloat) {
    // the fp32 model is told of either buffer (score or dS) ...
    const int f = xdot_flash_f32_row_splits(1, (int)fp32_mode, (int)g.D, has_score_or_ds_buf, W, g.T);
    if (f > 0) ns = f;
  }
  if (g.D > 128) {
    // ... the wide model only with the score buffer
    const int f = xdot_flash_wide_splits(1, dt_code(dtype), (int)g.D, has_sbuf, W, (g.T + 31) / 32);
    if (f > 0) ns = f;
  }
  return ns;
}

// row splits of the dQ / recompute pass and of the dV pass; heavy: per XCD `whole` column blocks
// unsplit, the last `rem` in `split` row pieces
struct ColsPlan { int sq = 1, sv = 1; bool heavy = false; int whole = 0, rem = 0, split = 0; };

// Row splits / grid of a column launch from the geometry and mode fields (set_cols_mode) of `a`: splits
// against the last-round tail (fp32, wide and pipelined 16-bit kernels, else 1) or the head-heavy grid
ColsPlan plan_cols(const xdot::fa::BwdArgs& a, int dt, int D) {
  ColsPlan p;
  if (dt == xdot::DT_F32 && D <= 128 && (a.prescaled || a.dkv16)) return p;
  TORCH_CHECK(xdot_flash_cols_splits(&a, dt, D, &p.sq, &p.sv) == 0, "xdot.flash_bwd_cols: split config");
  p.heavy = dt == xdot::DT_F32 && xdot_flash_f32_cols_heavy(&a, D, p.sq, &p.whole, &p.rem, &p.split);
  return p;
}

// ---- argument structs ---------------------------------------------------------------------
// the fields FwdArgs and BwdArgs share
template <class A>
A flash_args(const FlashGeom& g, const at::Tensor& rows, const at::Tensor& kc, const at::Tensor& vc, const OptT& bits,
             const OptT& flags, int64_t H, double scale, bool prescaled, int64_t fp32_mode) {
  A a{};
  a.rows = rows.data_ptr(); a.kc = kc.data_ptr(); a.vc = vc.data_ptr();
  const bool hb = bits.has_value() && bits->defined();
  a.mbits = hb ? reinterpret_cast<const uint64_t*>(bits->data_ptr()) : nullptr;
  a.mflags = hb ? flags->data_ptr<uint8_t>() : nullptr;
  a.B = (int)g.B; a.H = (int)H; a.R = (int)g.R; a.T = (int)g.T; a.scale = (float)scale;
  a.ldkv = g.ld;
  a.G = g.G > 1 ? (int)g.G : 0;
  a.gmul = g.G > 1 ? (int)(((1 << 20) + g.G - 1) / g.G) : 0;
  TORCH_CHECK(fp32_mode >= 0 && fp32_mode <= 2, "xdot.flash: fp32_mode must be 0 (exact), 1 (split) or 2 (split3), got ", fp32_mode);
  a.prescaled = prescaled ? 1 : 0; a.fp32_mode = (int)fp32_mode;
  return a;
}

constexpr auto fwd_args = flash_args<xdot::fa::FwdArgs>;

xdot::fa::BwdArgs bwd_args(const FlashGeom& g, const at::Tensor& dout, const at::Tensor& rows, const at::Tensor& kc,
                           const at::Tensor& vc, const at::Tensor& lse, const OptT& bits, const OptT& flags, int64_t H,
                           double scale, bool prescaled, int64_t fp32_mode) {
  TORCH_CHECK(dout.sizes() == rows.sizes() && dout.is_contiguous() && dout.scalar_type() == rows.scalar_type(),
              "xdot.flash_bwd: dout shape/dtype");
  check_bhr(lse, g.B, H, g.R, rows.device(), "xdot.flash_bwd: lse");
  auto a = flash_args<xdot::fa::BwdArgs>(g, rows, kc, vc, bits, flags, H, scale, prescaled, fp32_mode);
  a.dout = dout.data_ptr(); a.lse = lse.data_ptr<float>(); a.nsplit = 1;
  return a;
}

// the mode fields of a column launch (what plan_cols reads beside the geometry); returns the passes run
int64_t set_cols_mode(xdot::fa::BwdArgs& a, at::ScalarType dtype, int64_t D, float* sb, float* dsb, int64_t passes,
                      bool fp32_out) {
  // passes 4: the fused exact-fp32 column pass (dQ and dV in one kernel); other families run both (3)
  if (passes == 4 && (!sb || a.fp32_mode != 0 || D > 128 || dtype != at::kFloat)) passes = 3;
  TORCH_CHECK(passes >= 1 && passes <= 4 && (passes >= 3 || (sb && dsb)),
              "xdot.flash_bwd_cols: single passes (1 = dV, 2 = dQ) need the score and dS buffers");
  a.dkv16 = (fp32_out || dtype == at::kFloat) ? 0 : 1;
  a.sbuf = sb; a.dsbuf = dsb; a.sb_passes = (int)passes;
  return passes;
}

void check_part(const at::Tensor& t, int64_t slots_needed, int64_t per_slot, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == at::kFloat && t.dim() >= 1 &&
                  t.size(0) >= slots_needed && t.numel() == t.size(0) * per_slot,
              "xdot: partial buffer ", what, " has the wrong shape/dtype");
}

// δ = rowsum(dO ⊙ O) and, given lse, lse2 = lse * log2 e (else undefined): fp32 (B, H, R), one pass
std::tuple<at::Tensor, at::Tensor> bwd_prep(const at::Tensor& dout, const at::Tensor& out, const at::Tensor* lse, int64_t H,
                                            const char* op) {
  TORCH_CHECK(dout.is_cuda() && dout.dim() == 3 && dout.is_contiguous() && out.sizes() == dout.sizes() &&
                  out.is_contiguous() && out.scalar_type() == dout.scalar_type() && out.device() == dout.device(),
              "xdot.", op, ": dout/out must be matching contiguous (B, R, H*D) device tensors");
  TORCH_CHECK(H > 0 && dout.size(2) % H == 0, "xdot.", op, ": H");
  xdot::fa::BwdArgs a{};
  a.dout = dout.data_ptr(); a.B = (int)dout.size(0); a.R = (int)dout.size(1); a.H = (int)H;
  auto delta = at::empty({dout.size(0), H, dout.size(1)}, dout.options().dtype(at::kFloat));
  at::Tensor lse2;
  if (lse) {
    check_bhr(*lse, dout.size(0), H, dout.size(1), dout.device(), "xdot.flash_bwd_prep: lse (B, H, R) fp32");
    lse2 = at::empty_like(delta);
    a.lse = lse->data_ptr<float>();
    a.lse2 = lse2.data_ptr<float>();
  }
  c10::DeviceGuard guard(dout.device());
  launched(xdot_flash_bwd_delta_launch(&a, out.data_ptr(), delta.data_ptr<float>(), dt_code(dout.scalar_type()),
                                       (int)(dout.size(2) / H), cur_stream(dout)),
           op, "unsupported dtype/head dim");
  return {delta, lse2};
}

// ---- ops ------------------------------------------------------------------------------------
std::tuple<at::Tensor, at::Tensor> flash_fwd(const at::Tensor& rows, const at::Tensor& kc, const at::Tensor& vc,
                                             const OptT& bits, const OptT& flags, int64_t H, double scale, int64_t nsplit,
                                             bool prescaled, int64_t fp32_mode, const OptT& sbuf, int64_t Hg) {
  Range rr_("xdot.flash_fwd");
  const FlashGeom g = flash_check(rows, kc, vc, H, bits, flags, false, Hg);
  float* sb = sbuf_ptr(sbuf, g, H, rows, fp32_mode, "xdot.flash_fwd");
  auto out = at::empty_like(rows);
  const auto f32 = rows.options().dtype(at::kFloat);
  auto lse = at::empty({g.B, H, g.R}, f32);
  const FwdPlan p = plan_fwd(g, H, rows.scalar_type(), fp32_mode, sb != nullptr, nsplit);
  auto a = fwd_args(g, rows, kc, vc, bits, flags, H, scale, prescaled, fp32_mode);
  at::Tensor opart, lpart;
  if (p.heavy) {  // compact partials of the split tail blocks only
    opart = at::empty({(int64_t)p.nsplit * 8 * p.rem * 128 * g.D}, f32);
    lpart = at::empty({(int64_t)p.nsplit * 8 * p.rem * 128}, f32);
    a.xrbs = (int)(p.blocks / 8); a.xwhole = p.whole; a.xrem = p.rem;
  } else if (p.nsplit > 1) {
    opart = at::empty({p.nsplit, g.B, g.R, g.C}, f32);
    lpart = at::empty({p.nsplit, g.B, H, g.R}, f32);
  }
  a.out = out.data_ptr(); a.lse = lse.data_ptr<float>(); a.nsplit = p.nsplit;
  a.opart = p.nsplit > 1 ? opart.data_ptr<float>() : nullptr;
  a.lpart = p.nsplit > 1 ? lpart.data_ptr<float>() : nullptr;
  a.sbuf = sb;
  c10::DeviceGuard guard(rows.device());
  launched(xdot_flash_fwd_launch(&a, dt_code(rows.scalar_type()), (int)g.D, cur_stream(rows)), "flash_fwd");
  return {out, lse};
}

// [nsplit, heavy, whole, rem]: what flash_fwd would choose for this shape on the current device
std::vector<int64_t> flash_fwd_plan(int64_t B, int64_t R, int64_t T, int64_t H, int64_t D, at::ScalarType dtype,
                                    int64_t fp32_mode, bool sbuf, int64_t nsplit) {
  const FwdPlan p = plan_fwd(query_geom(B, R, T, H, D), H, dtype, fp32_mode, sbuf, nsplit);
  return {p.nsplit, p.heavy, p.whole, p.rem};
}

// [nsplit, workgroups per CU, rounds]: what flash_bwd_rows would choose for this shape on the current
// device without a score or dS buffer (workgroups per CU: XDOT_ROWS_WPC, read per call; 0 and no rounds
// outside the 16-bit D <= 128 family)
std::vector<int64_t> flash_rows_plan(int64_t B, int64_t R, int64_t T, int64_t H, int64_t D, at::ScalarType dtype,
                                     int64_t fp32_mode, bool prescaled, int64_t nsplit) {
  const int ns = plan_rows(query_geom(B, R, T, H, D), H, dtype, fp32_mode, false, false, nsplit);
  xdot::fa::BwdArgs a{};
  a.B = (int)B; a.R = (int)R; a.T = (int)T; a.H = (int)H; a.nsplit = ns; a.prescaled = prescaled ? 1 : 0;
  const int wpc = xdot_flash_bwd_rows_wpc(&a, dt_code(dtype), (int)D);
  return {ns, wpc, wpc > 0 ? rows_rounds(B, R, H, ns, wpc, xdot_num_cus()) : 0};
}

// gathered-side grads, packed fp32 (B, T, 2C) = [dq | dv] partials for ONE reduce-scatter,
// + δ = rowsum(dO·O)
std::tuple<at::Tensor, at::Tensor> flash_bwd_cols(const at::Tensor& dout, const at::Tensor& rows, const at::Tensor& kc,
                                                  const at::Tensor& vc, const at::Tensor& out, const at::Tensor& lse,
                                                  const OptT& bits, const OptT& flags, int64_t H, double scale,
                                                  const OptT& delta_in, bool fp32_out, bool prescaled, const OptT& lse2_in,
                                                  int64_t fp32_mode, const OptT& sbuf, const OptT& dsbuf, int64_t passes,
                                                  const OptT& dkv_out, int64_t Hg) {
  Range rr_("xdot.flash_bwd_cols");
  const FlashGeom g = flash_check(rows, kc, vc, H, bits, flags, /*colmajor=*/true, Hg);
  float* sb = sbuf_ptr(sbuf, g, H, rows, fp32_mode, "xdot.flash_bwd_cols");
  float* dsb = sbuf_ptr(dsbuf, g, H, rows, fp32_mode, "xdot.flash_bwd_cols (dS buffer)", true);
  // a dS buffer alone: dS-only mode (the recomputing column kernel stores dS, D <= 128)
  TORCH_CHECK(!dsb || sb || g.D <= 128, "xdot.flash_bwd_cols: a dS buffer without the score buffer needs D <= 128");
  TORCH_CHECK(out.sizes() == rows.sizes() && out.is_contiguous() && out.scalar_type() == rows.scalar_type(),
              "xdot.flash_bwd_cols: out shape/dtype");
  auto a = bwd_args(g, dout, rows, kc, vc, lse, bits, flags, H, scale, prescaled, fp32_mode);
  passes = set_cols_mode(a, rows.scalar_type(), g.D, sb, dsb, passes, fp32_out);
  const auto f32 = rows.options().dtype(at::kFloat);
  // dkv_out: the other pass's output, completed in place
  at::Tensor dkv = dkv_out.has_value() && dkv_out->defined() ? *dkv_out
                       : at::empty({g.B, g.T, 2 * g.Cg}, fp32_out ? kc.options().dtype(at::kFloat) : kc.options());
  TORCH_CHECK(dkv.is_contiguous() && dkv.sizes() == at::IntArrayRef({g.B, g.T, 2 * g.Cg}) &&
                  dkv.scalar_type() == (fp32_out ? at::kFloat : kc.scalar_type()) && dkv.device() == rows.device(),
              "xdot.flash_bwd_cols: dkv_out must be (B, T, 2 * Hg * D) = (", g.B, ", ", g.T, ", ", 2 * g.Cg,
              ") in the output dtype");
  const bool have_delta = delta_in.has_value() && delta_in->defined();
  if (have_delta) check_bhr(*delta_in, g.B, H, g.R, rows.device(), "xdot.flash_bwd_cols: delta");
  at::Tensor delta = have_delta ? *delta_in : at::empty({g.B, H, g.R}, f32);
  a.dkc = dkv.data_ptr(); a.dvc = static_cast<char*>(dkv.data_ptr()) + g.Cg * dkv.element_size(); a.ldg = 2 * g.Cg;
  a.delta = delta.data_ptr<float>();
  // lse2 = lse * log2 e: given (from flash_bwd_prep, together with δ), or one prep pass here
  const bool have_lse2 = have_delta && lse2_in.has_value() && lse2_in->defined();
  if (have_lse2) check_bhr(*lse2_in, g.B, H, g.R, rows.device(), "xdot.flash_bwd_cols: lse2");
  at::Tensor lse2 = have_lse2 ? *lse2_in : at::empty({g.B, H, g.R}, f32);
  a.lse2 = lse2.data_ptr<float>();
  c10::DeviceGuard guard(rows.device());
  const int dt = dt_code(rows.scalar_type());
  // prep: lse2 (+ δ unless given)
  if (!have_lse2)
    TORCH_CHECK(xdot_flash_bwd_delta_launch(&a, out.data_ptr(), have_delta ? nullptr : delta.data_ptr<float>(), dt,
                                            (int)g.D, cur_stream(rows)) == 0,
                "xdot.flash_bwd_cols: config");
  // fp32 partials of the split launches, summed in the launcher
  const ColsPlan p = plan_cols(a, dt, (int)g.D);
  // (the single-pass recompute kernels use sq for both halves: sv == sq there)
  const bool run_q = !sb || passes == 4 || (passes & 2), run_v = !sb || passes == 4 || (passes & 1);
  at::Tensor cpq, cpv;
  if (p.heavy) {  // compact partials of the XCDs' tail blocks only
    cpq = at::empty({(int64_t)p.split * 8 * p.rem * 128 * g.D}, f32);
    cpv = at::empty_like(cpq);
    a.csq = a.csv = p.split;
    a.xcb = (int)(((g.T + 127) / 128) * g.B * H / 8); a.xwhole = p.whole; a.xrem = p.rem;
  } else {
    a.csq = run_q && p.sq > 1 ? p.sq : 0;
    a.csv = run_v && p.sv > 1 ? p.sv : 0;
    if (a.csq) cpq = at::empty({a.csq, g.B, g.T, g.Cg}, f32);
    if (a.csv) cpv = at::empty({a.csv, g.B, g.T, g.Cg}, f32);
  }
  a.cpq = cpq.defined() ? cpq.data_ptr<float>() : nullptr;
  a.cpv = cpv.defined() ? cpv.data_ptr<float>() : nullptr;
  launched(xdot_flash_bwd_cols_launch(&a, dt, (int)g.D, cur_stream(rows)), "flash_bwd_cols");
  return {dkv, delta};
}

// [sq, sv, heavy, whole, rem, split]: what flash_bwd_cols would choose for this shape on the current device
std::vector<int64_t> flash_cols_plan(int64_t B, int64_t R, int64_t T, int64_t H, int64_t D, at::ScalarType dtype,
                                     int64_t fp32_mode, bool sbuf, bool dsbuf, int64_t passes, bool prescaled,
                                     bool fp32_out, int64_t Hg) {
  const FlashGeom g = query_geom(B, R, T, H, D);
  TORCH_CHECK(Hg >= 0 && (Hg == 0 || H % Hg == 0), "xdot.flash_cols_plan: H must be a multiple of Hg");
  static float present;  // the planner only asks whether the buffers exist
  xdot::fa::BwdArgs a{};
  a.B = (int)B; a.H = (int)H; a.R = (int)R; a.T = (int)T;
  a.prescaled = prescaled ? 1 : 0; a.fp32_mode = (int)fp32_mode;
  a.G = Hg > 0 && Hg < H ? (int)(H / Hg) : 0;
  set_cols_mode(a, dtype, D, sbuf ? &present : nullptr, dsbuf ? &present : nullptr, passes, fp32_out);
  const ColsPlan p = plan_cols(a, dt_code(dtype), (int)g.D);
  return {p.sq, p.sv, p.heavy, p.whole, p.rem, p.split};
}

// out (n elements, any kernel dtype) = Σ_s part[s] over the leading (split) dim of fp32 partials, one pass
void sum_into(const at::Tensor& part, at::Tensor& out, const char* op, const char* why) {
  TORCH_CHECK(part.is_cuda() && part.is_contiguous() && part.scalar_type() == at::kFloat && part.dim() >= 2, "xdot.", op,
              ": contiguous fp32 (S, ...) device tensor");
  const int64_t n = out.numel();
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() && n * part.size(0) == part.numel(), "xdot.", op,
              ": out must be a contiguous fp32 slot");
  TORCH_CHECK(n % 4 == 0 && aligned16(part.data_ptr()) && aligned16(out.data_ptr()), "xdot.", op,
              ": numel % 4 and 16-byte alignment");
  c10::DeviceGuard guard(part.device());
  TORCH_CHECK(xdot_sum_partials_launch(part.data_ptr<float>(), out.data_ptr(), (int)part.size(0), n,
                                       dt_code(out.scalar_type()), cur_stream(part)) == 0, "xdot.", op, why);
  check_launch(hipGetLastError(), op);
}

// Σ_s part[s] cast to out_dtype
at::Tensor sum_partials(const at::Tensor& part, at::ScalarType out_dtype) {
  Range rr_("xdot.sum_partials");
  auto out = at::empty(part.sizes().slice(part.dim() ? 1 : 0), part.options().dtype(out_dtype));
  sum_into(part, out, "sum_partials", ": unsupported dtype");
  return out;
}

// out = Σ_s part[s] in fp32; out may be part[0] (running sums: each element is read and
// written by one thread)
void sum_partials_into(const at::Tensor& part, at::Tensor& out) {
  Range rr_("xdot.sum_partials_into");
  TORCH_CHECK(out.scalar_type() == at::kFloat, "xdot.sum_partials_into: out must be a contiguous fp32 slot");
  sum_into(part, out, "sum_partials_into", "");
}

// row side of the flash kernels pre-multiplied by scale * log2(e), in the input dtype
at::Tensor flash_prescale(const at::Tensor& x, double scale) {
  Range rr_("xdot.flash_prescale");
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && (x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kHalf) &&
                  x.numel() % 8 == 0 && aligned16(x.data_ptr()),
              "xdot.flash_prescale: contiguous 16-byte aligned bf16/fp16 device tensor, numel % 8 == 0");
  auto out = at::empty_like(x);
  c10::DeviceGuard guard(x.device());
  launched(xdot_prescale_rows_launch(x.data_ptr(), out.data_ptr(), x.numel(), (float)scale, dt_code(x.scalar_type()),
                                     cur_stream(x)),
           "flash_prescale", "dtype");
  return out;
}

// δ = rowsum(dO ⊙ O) per (b, h, row), fp32 (B, H, R)
at::Tensor flash_bwd_delta(const at::Tensor& dout, const at::Tensor& out, int64_t H) {
  Range rr_("xdot.flash_bwd_delta");
  return std::get<0>(bwd_prep(dout, out, nullptr, H, "flash_bwd_delta"));
}

// δ = rowsum(dO ⊙ O) and lse2 = lse * log2 e, both fp32 (B, H, R), in ONE pass: the fused
// backward's prep (flash_bwd_cols then takes both and launches no prep of its own)
std::tuple<at::Tensor, at::Tensor> flash_bwd_prep(const at::Tensor& dout, const at::Tensor& out, const at::Tensor& lse,
                                                  int64_t H) {
  Range rr_("xdot.flash_bwd_prep");
  return bwd_prep(dout, out, &lse, H, "flash_bwd_prep");
}

// row-side grad (this rank's rows), column-split when the row count is small
at::Tensor flash_bwd_rows(const at::Tensor& dout, const at::Tensor& rows, const at::Tensor& kc, const at::Tensor& vc,
                          const at::Tensor& lse, const at::Tensor& delta, const OptT& bits, const OptT& flags, int64_t H,
                          double scale, int64_t nsplit, bool prescaled, int64_t fp32_mode, const OptT& sbuf,
                          const OptT& dsbuf, int64_t Hg) {
  Range rr_("xdot.flash_bwd_rows");
  const FlashGeom g = flash_check(rows, kc, vc, H, bits, flags, false, Hg);
  float* sb = sbuf_ptr(sbuf, g, H, rows, fp32_mode, "xdot.flash_bwd_rows");
  float* dsb = sbuf_ptr(dsbuf, g, H, rows, fp32_mode, "xdot.flash_bwd_rows (dS buffer)", true);
  TORCH_CHECK(!dsb || sb || g.D <= 128, "xdot.flash_bwd_rows: a dS buffer without the score buffer needs D <= 128");
  check_bhr(delta, g.B, H, g.R, rows.device(), "xdot.flash_bwd_rows: delta");
  auto a = bwd_args(g, dout, rows, kc, vc, lse, bits, flags, H, scale, prescaled, fp32_mode);
  auto drows = at::empty_like(rows);
  const int ns = plan_rows(g, H, rows.scalar_type(), fp32_mode, sb || dsb, sb != nullptr, nsplit);
  at::Tensor dpart;
  if (ns > 1) dpart = at::empty({ns, g.B, g.R, g.C}, rows.options().dtype(at::kFloat));
  a.delta = delta.data_ptr<float>(); a.drows = drows.data_ptr();
  a.nsplit = ns; a.dpart = ns > 1 ? dpart.data_ptr<float>() : nullptr;
  a.sbuf = sb; a.dsbuf = dsb;
  c10::DeviceGuard guard(rows.device());
  launched(xdot_flash_bwd_rows_launch(&a, dt_code(rows.scalar_type()), (int)g.D, cur_stream(rows)), "flash_bwd_rows");
  return drows;
}

// ---- decode (csrc/flash_decode.hip) ----------------------------------------------------
// Rn new rows at positions pos0, pos0 + 1, ... against one rank's cache qc / vc (B, Tcap, Hg*D) whose slot
// positions are col_pos (B, Tcap) int32, -1 = empty: -> (out (B, Rn, H*D) in the rows' dtype, or fp32 with
// out_fp32: the wire format of the cross-rank merge; lse (B, H, Rn)).  nsplit 0: plan_decode
// qscale / vscale set: the cache is fp8 (e4m3fn bytes, row stride in bytes) with fp32 (B, Hg, Tcap) scale
// views (csrc/flash_decode8.hip; with `extend`, csrc/flash_extend8.hip); every other check is the 16-bit call's.
std::tuple<at::Tensor, at::Tensor> decode_call(const char* op, const at::Tensor& rows, const at::Tensor& qc, const at::Tensor& vc,
                                               const at::Tensor* qscale, const at::Tensor* vscale, const at::Tensor& col_pos,
                                               int64_t pos0, int64_t window, int64_t H, double scale, int64_t Hg,
                                               int64_t nsplit, bool out_fp32, bool extend = false) {
  const bool fp8 = qscale != nullptr;
  TORCH_CHECK(rows.is_cuda() && qc.is_cuda() && vc.is_cuda() && col_pos.is_cuda() && qc.device() == rows.device() &&
                  vc.device() == rows.device() && col_pos.device() == rows.device(),
              op, "rows, qc, vc and col_pos must be tensors on one GPU");
  TORCH_CHECK(rows.scalar_type() == at::kBFloat16 || rows.scalar_type() == at::kHalf, op, "bf16 / fp16 only, got ",
              rows.scalar_type());
  if (fp8) {
    TORCH_CHECK(qc.scalar_type() == at::kFloat8_e4m3fn && vc.scalar_type() == at::kFloat8_e4m3fn, op,
                "qc and vc must be float8_e4m3fn, got ", qc.scalar_type(), " and ", vc.scalar_type());
  } else {
    TORCH_CHECK(qc.scalar_type() == rows.scalar_type() && vc.scalar_type() == rows.scalar_type(), op,
                "rows, qc and vc must have one dtype");
  }
  TORCH_CHECK(rows.dim() == 3 && rows.is_contiguous(), op, "rows must be a contiguous (B, Rn, H*D) tensor");
  const int64_t B = rows.size(0), Rn = rows.size(1), C = rows.size(2), hg = Hg > 0 ? Hg : H;
  TORCH_CHECK(H > 0 && C % H == 0 && hg <= H && H % hg == 0, op, "H = ", H, " must divide the row width ", C,
              " and be a multiple of Hg = ", hg);
  const int64_t D = C / H, G = H / hg;
  TORCH_CHECK(D == 32 || D == 64 || D == 96 || D == 128, op, "head dim must be 32 / 64 / 96 / 128, got ", D);
  if (extend) {
    TORCH_CHECK(B > 0 && Rn > 0 && G * Rn > DEC_MAX_ROWS && G <= EXT_MAX_GROUP, op, "G * Rn = ", G * Rn,
                " rows per gathered head with G = ", G, ", the kernel takes more than ", DEC_MAX_ROWS, " with G <= ", EXT_MAX_GROUP);
  } else {
    TORCH_CHECK(B > 0 && Rn > 0 && decode_row_tiles(G, Rn) > 0, op, "G * Rn = ", G * Rn, " rows per gathered head, the kernel takes 1..",
                DEC_MAX_ROWS);
  }
  TORCH_CHECK(qc.dim() == 3 && qc.size(0) == B && qc.size(2) == hg * D && vc.sizes() == qc.sizes() && qc.size(1) > 0,
              op, "qc and vc must be (B, Tcap, Hg*D) = (", B, ", Tcap, ", hg * D, ")");
  const int64_t Tcap = qc.size(1), ld = qc.stride(1), ldq = fp8 ? 16 : 8;  // rows on the 16-byte grid
  for (const at::Tensor* t : {&qc, &vc}) {
    TORCH_CHECK(t->stride(2) == 1 && t->stride(1) == ld && ld >= hg * D && ld % ldq == 0 && (B == 1 || t->stride(0) == Tcap * ld),
                op, "qc and vc must be rows of unit inner stride with one row stride (a multiple of ", ldq,
                ") and batch stride Tcap * row stride");
    TORCH_CHECK((B - 1) * Tcap * ld + (Tcap - 1) * ld + hg * D <= avail_elems(*t), op, "cache view out of bounds");
  }
  TORCH_CHECK(aligned16(rows.data_ptr()) && aligned16(qc.data_ptr()) && aligned16(vc.data_ptr()), op, "16-byte alignment");
  TORCH_CHECK(col_pos.scalar_type() == at::kInt && col_pos.dim() == 2 && col_pos.size(0) == B && col_pos.size(1) == Tcap &&
                  col_pos.is_contiguous(),
              op, "col_pos must be a contiguous int32 (B, Tcap) = (", B, ", ", Tcap, ") tensor, got ", col_pos.scalar_type(),
              " ", col_pos.sizes());
  TORCH_CHECK(pos0 >= 0 && pos0 + Rn < (1LL << 31) && window >= 0 && window < (1LL << 31), op,
              "pos0 and window must be >= 0 and positions stay below 2^31");
  TORCH_CHECK(Tcap < (1LL << 31) - DEC_TILE && B * Tcap * ld < (1LL << 40), op, "cache too large");
  if (fp8) {
    for (const at::Tensor* t : {qscale, vscale}) {
      TORCH_CHECK(t->is_cuda() && t->device() == rows.device() && t->scalar_type() == at::kFloat && t->dim() == 3 &&
                      t->size(0) == B && t->size(1) == hg && t->size(2) == Tcap && t->stride(2) == 1 &&
                      t->strides() == qscale->strides() && t->stride(1) >= Tcap && (B == 1 || t->stride(0) >= hg * t->stride(1)),
                  op, "qscale and vscale must be fp32 (B, Hg, Tcap) = (", B, ", ", hg, ", ", Tcap,
                  ") views on the rows' GPU with unit inner stride and the same strides");
      TORCH_CHECK((B - 1) * t->stride(0) + (hg - 1) * t->stride(1) + Tcap <= avail_elems(*t), op, "scale view out of bounds");
    }
  }
  c10::DeviceGuard guard(rows.device());
  const int64_t ntiles = (Tcap + DEC_TILE - 1) / DEC_TILE;
  TORCH_CHECK(nsplit >= 0, op, "nsplit must be >= 0");
  const int nrt = decode_row_tiles(G, Rn), cus = xdot_num_cus();
  const int rb = extend ? extend_block_rows(G, (int)D) : 0;
  const int64_t nblk = extend ? (Rn + rb - 1) / rb : 1;
  const int ns = nsplit > 0 ? (int)std::min(nsplit, ntiles)
                 : extend   ? (fp8 ? plan_extend_fp8(B, hg, G, Rn, (int)D, Tcap, cus) : plan_extend(B, hg, G, Rn, (int)D, Tcap, cus))
                 : fp8      ? plan_decode_fp8(B, hg, nrt, (int)D, Tcap, cus)
                            : plan_decode(B, hg, nrt, Tcap, cus);
  TORCH_CHECK((int64_t)ns * nblk * B * hg < (1LL << 31), op, "too many workgroups");
  const auto f32 = rows.options().dtype(at::kFloat);
  const bool parts = !extend || ns > 1;  // one span of the row-blocked sweep writes out / lse itself
  at::Tensor opart, lpart;
  if (parts) opart = at::empty({ns, B, Rn, C}, f32), lpart = at::empty({ns, B, H, Rn}, f32);
  auto out = at::empty({B, Rn, C}, out_fp32 ? f32 : rows.options()), lse = at::empty({B, H, Rn}, f32);
  DecodeArgs a{};
  a.rows = rows.data_ptr(); a.qc = qc.data_ptr(); a.vc = vc.data_ptr(); a.col_pos = col_pos.data_ptr<int32_t>();
  a.opart = parts ? opart.data_ptr<float>() : nullptr; a.lpart = parts ? lpart.data_ptr<float>() : nullptr;
  a.out = out.data_ptr(); a.lse = lse.data_ptr<float>();
  a.B = (int)B; a.H = (int)H; a.Hg = (int)hg; a.Rn = (int)Rn; a.Tcap = (int)Tcap; a.ldkv = ld;
  a.pos0 = (int)pos0; a.window = (int)window; a.scale = (float)scale;
  a.nspan = ns; a.span_tiles = decode_span_tiles(Tcap, ns); a.out32 = out_fp32 ? 1 : 0;
  if (fp8) {
    a.qscale = qscale->data_ptr<float>(); a.vscale = vscale->data_ptr<float>();
    a.sc_head = hg > 1 ? qscale->stride(1) : 0; a.sc_batch = B > 1 ? qscale->stride(0) : 0;
  }
  if (extend) {
    ExtendArgs ea{a, rb, (int)nblk};
    if (fp8) launched(xdot_flash_extend8_launch(&ea, dt_code(rows.scalar_type()), (int)D, cur_stream(rows)), "flash_extend_fp8");
    else launched(xdot_flash_extend_launch(&ea, dt_code(rows.scalar_type()), (int)D, cur_stream(rows)), "flash_extend");
  } else if (fp8) {
    launched(xdot_flash_decode8_launch(&a, dt_code(rows.scalar_type()), (int)D, cur_stream(rows)), "flash_decode_fp8");
  } else {
    launched(xdot_flash_decode_launch(&a, dt_code(rows.scalar_type()), (int)D, cur_stream(rows)), "flash_decode");
  }
  return {out, lse};
}

std::tuple<at::Tensor, at::Tensor> flash_decode(const at::Tensor& rows, const at::Tensor& qc, const at::Tensor& vc,
                                                const at::Tensor& col_pos, int64_t pos0, int64_t window, int64_t H,
                                                double scale, int64_t Hg, int64_t nsplit, bool out_fp32) {
  Range rr_("xdot.flash_decode");
  return decode_call("xdot.flash_decode: ", rows, qc, vc, nullptr, nullptr, col_pos, pos0, window, H, scale, Hg, nsplit, out_fp32);
}

std::tuple<at::Tensor, at::Tensor> flash_decode_fp8(const at::Tensor& rows, const at::Tensor& qc, const at::Tensor& vc,
                                                    const at::Tensor& qscale, const at::Tensor& vscale, const at::Tensor& col_pos,
                                                    int64_t pos0, int64_t window, int64_t H, double scale, int64_t Hg,
                                                    int64_t nsplit, bool out_fp32) {
  Range rr_("xdot.flash_decode_fp8");
  return decode_call("xdot.flash_decode_fp8: ", rows, qc, vc, &qscale, &vscale, col_pos, pos0, window, H, scale, Hg, nsplit, out_fp32);
}

// the same call with G * Rn > 64 rows per gathered head: the row-blocked sweep (csrc/flash_extend.hip), a
// 16-bit cache; nsplit 0: plan_extend
std::tuple<at::Tensor, at::Tensor> flash_extend(const at::Tensor& rows, const at::Tensor& qc, const at::Tensor& vc,
                                                const at::Tensor& col_pos, int64_t pos0, int64_t window, int64_t H,
                                                double scale, int64_t Hg, int64_t nsplit, bool out_fp32) {
  Range rr_("xdot.flash_extend");
  return decode_call("xdot.flash_extend: ", rows, qc, vc, nullptr, nullptr, col_pos, pos0, window, H, scale, Hg, nsplit, out_fp32,
                     true);
}

// the same over an fp8 cache with (B, Hg, Tcap) scale views (csrc/flash_extend8.hip); nsplit 0: plan_extend_fp8
std::tuple<at::Tensor, at::Tensor> flash_extend_fp8(const at::Tensor& rows, const at::Tensor& qc, const at::Tensor& vc,
                                                    const at::Tensor& qscale, const at::Tensor& vscale, const at::Tensor& col_pos,
                                                    int64_t pos0, int64_t window, int64_t H, double scale, int64_t Hg,
                                                    int64_t nsplit, bool out_fp32) {
  Range rr_("xdot.flash_extend_fp8");
  return decode_call("xdot.flash_extend_fp8: ", rows, qc, vc, &qscale, &vscale, col_pos, pos0, window, H, scale, Hg, nsplit, out_fp32,
                     true);
}

// ---- paged decode (csrc/flash_paged.hip) ---------------------------------------------------------
// The decode call for a ragged batch over a pool of pages: qpool / vpool (P, S, Hg*D) the two halves of the
// pool's slots, pool_pos (P, S) int32 their positions, table (B, maxp) int32 the page of each logical block
// (-1: a hole), npages (B,) int32 the entries in use, pos0 (B,) int32 the position of each sequence's first
// new row (negative: inactive).  The three last are read by the kernel: nothing here waits for the device.
// max_pages: the most pages any sequence holds, if the caller knows better than maxp (it only sizes the grid).
struct PagedGeom {
  int64_t B, Rn, C, hg, D, G, P, S, maxp, ld;
};

PagedGeom paged_check(const char* op, const at::Tensor& rows, const at::Tensor& qpool, const at::Tensor& vpool,
                      const at::Tensor& pool_pos, const at::Tensor& table, const at::Tensor& npages, const at::Tensor& pos0,
                      int64_t window, int64_t H, int64_t Hg, bool fp8 = false) {
  for (const at::Tensor* t : {&rows, &qpool, &vpool, &pool_pos, &table, &npages, &pos0})
    TORCH_CHECK(t->is_cuda() && t->device() == rows.device(), op, "every tensor must be on the rows' GPU");
  TORCH_CHECK(rows.scalar_type() == at::kBFloat16 || rows.scalar_type() == at::kHalf, op, "bf16 / fp16 only, got ",
              rows.scalar_type());
  if (fp8) {
    TORCH_CHECK(qpool.scalar_type() == at::kFloat8_e4m3fn && vpool.scalar_type() == at::kFloat8_e4m3fn, op,
                "qpool and vpool must be float8_e4m3fn, got ", qpool.scalar_type(), " and ", vpool.scalar_type());
  } else {
    TORCH_CHECK(qpool.scalar_type() == rows.scalar_type() && vpool.scalar_type() == rows.scalar_type(), op,
                "rows, qpool and vpool must have one dtype");
  }
  TORCH_CHECK(rows.dim() == 3 && rows.is_contiguous(), op, "rows must be a contiguous (B, Rn, H*D) tensor");
  PagedGeom g{};
  g.B = rows.size(0); g.Rn = rows.size(1); g.C = rows.size(2); g.hg = Hg > 0 ? Hg : H;
  TORCH_CHECK(H > 0 && g.C % H == 0 && g.hg <= H && H % g.hg == 0, op, "H = ", H, " must divide the row width ", g.C,
              " and be a multiple of Hg = ", g.hg);
  g.D = g.C / H; g.G = H / g.hg;
  TORCH_CHECK(g.D == 32 || g.D == 64 || g.D == 96 || g.D == 128, op, "head dim must be 32 / 64 / 96 / 128, got ", g.D);
  TORCH_CHECK(g.B > 0 && g.Rn > 0 && decode_row_tiles(g.G, g.Rn) > 0, op, "G * Rn = ", g.G * g.Rn,
              " rows per gathered head, the kernel takes 1..", DEC_MAX_ROWS);
  TORCH_CHECK(qpool.dim() == 3 && qpool.size(0) > 0 && qpool.size(2) == g.hg * g.D && vpool.sizes() == qpool.sizes(), op,
              "qpool and vpool must be (P, S, Hg*D) = (P, S, ", g.hg * g.D, ")");
  g.P = qpool.size(0); g.S = qpool.size(1); g.ld = qpool.stride(1);
  TORCH_CHECK(paged_page_size_ok(g.S), op, "the page size must be 32, 64, 128 or 256 slots, got ", g.S);
  const int64_t ldq = fp8 ? 16 : 8;  // slots on the 16-byte grid
  for (const at::Tensor* t : {&qpool, &vpool}) {
    TORCH_CHECK(t->stride(2) == 1 && t->stride(1) == g.ld && g.ld >= g.hg * g.D && g.ld % ldq == 0 && (g.P == 1 || t->stride(0) == g.S * g.ld),
                op, "qpool and vpool must be slots of unit inner stride with one slot stride (a multiple of ", ldq,
                ") and page stride S * slot stride");
    TORCH_CHECK((g.P * g.S - 1) * g.ld + g.hg * g.D <= avail_elems(*t), op, "pool view out of bounds");
  }
  TORCH_CHECK(aligned16(rows.data_ptr()) && aligned16(qpool.data_ptr()) && aligned16(vpool.data_ptr()), op, "16-byte alignment");
  TORCH_CHECK(g.P * g.S < (1LL << 31) && g.P * g.S * g.ld < (1LL << 40), op, "pool too large");
  TORCH_CHECK(pool_pos.scalar_type() == at::kInt && pool_pos.dim() == 2 && pool_pos.size(0) == g.P && pool_pos.size(1) == g.S &&
                  pool_pos.is_contiguous(),
              op, "pool_pos must be a contiguous int32 (P, S) = (", g.P, ", ", g.S, ") tensor, got ", pool_pos.scalar_type(), " ",
              pool_pos.sizes());
  TORCH_CHECK(table.scalar_type() == at::kInt && table.dim() == 2 && table.size(0) == g.B && table.size(1) > 0 && table.is_contiguous(),
              op, "table must be a contiguous int32 (B, maxp) = (", g.B, ", maxp) tensor, got ", table.scalar_type(), " ", table.sizes());
  g.maxp = table.size(1);
  TORCH_CHECK(g.maxp * g.S < (1LL << 31), op, "table too wide");
  for (const at::Tensor* t : {&npages, &pos0})
    TORCH_CHECK(t->scalar_type() == at::kInt && t->dim() == 1 && t->size(0) == g.B && t->is_contiguous(), op,
                "npages and pos0 must be contiguous int32 (B,) = (", g.B, ",) tensors, got ", t->scalar_type(), " ", t->sizes());
  TORCH_CHECK(window >= 0 && window < (1LL << 31), op, "window must be >= 0 and below 2^31");
  return g;
}

// qscale / vscale set: the pool is fp8 (e4m3fn bytes, slot stride in bytes) with fp32 (P, Hg, S) scale views, the
// two halves of one (P, 2*Hg, S) buffer (csrc/flash_paged8.hip); every other check is the 16-bit call's.
std::tuple<at::Tensor, at::Tensor> paged_call(const char* op, const char* what, const at::Tensor& rows, const at::Tensor& qpool,
                                              const at::Tensor& vpool, const at::Tensor* qscale, const at::Tensor* vscale,
                                              const at::Tensor& pool_pos, const at::Tensor& table, const at::Tensor& npages,
                                              const at::Tensor& pos0, int64_t window, int64_t H, double scale, int64_t Hg,
                                              int64_t nsplit, bool out_fp32, int64_t max_pages) {
  const bool fp8 = qscale != nullptr;
  const PagedGeom g = paged_check(op, rows, qpool, vpool, pool_pos, table, npages, pos0, window, H, Hg, fp8);
  TORCH_CHECK(nsplit >= 0 && max_pages >= 0, op, "nsplit and max_pages must be >= 0");
  if (fp8) {
    for (const at::Tensor* t : {qscale, vscale}) {
      TORCH_CHECK(t->is_cuda() && t->device() == rows.device() && t->scalar_type() == at::kFloat && t->dim() == 3 &&
                      t->size(0) == g.P && t->size(1) == g.hg && t->size(2) == g.S && t->stride(2) == 1 && t->stride(1) == g.S &&
                      t->strides() == qscale->strides() && t->stride(0) >= g.hg * g.S && t->stride(0) % 4 == 0 &&
                      aligned16(t->data_ptr()),
                  op, "qscale and vscale must be fp32 (P, Hg, S) = (", g.P, ", ", g.hg, ", ", g.S,
                  ") views on the rows' GPU with unit inner stride, head stride S, one 16-byte aligned page stride");
      TORCH_CHECK((g.P - 1) * t->stride(0) + g.hg * g.S <= avail_elems(*t), op, "scale view out of bounds");
    }
    TORCH_CHECK(g.P * qscale->stride(0) < (1LL << 40), op, "pool too large");
  }
  c10::DeviceGuard guard(rows.device());
  const int64_t mp = max_pages > 0 ? std::min(max_pages, g.maxp) : g.maxp, ntiles = mp * (g.S / DEC_TILE);
  const int nrt = decode_row_tiles(g.G, g.Rn), cus = xdot_num_cus();
  const int ns = nsplit > 0 ? (int)std::min(nsplit, ntiles)
                 : fp8      ? plan_decode_paged_fp8(g.B, g.hg, nrt, (int)g.D, mp, g.S, cus)
                            : plan_decode_paged(g.B, g.hg, nrt, mp, g.S, cus);
  TORCH_CHECK((int64_t)ns * g.B * g.hg < (1LL << 31), op, "too many workgroups");
  const auto f32 = rows.options().dtype(at::kFloat);
  auto opart = at::empty({ns, g.B, g.Rn, g.C}, f32), lpart = at::empty({ns, g.B, H, g.Rn}, f32);
  auto out = at::empty({g.B, g.Rn, g.C}, out_fp32 ? f32 : rows.options()), lse = at::empty({g.B, H, g.Rn}, f32);
  PagedArgs a{};
  a.d.rows = rows.data_ptr(); a.d.qc = qpool.data_ptr(); a.d.vc = vpool.data_ptr(); a.d.col_pos = pool_pos.data_ptr<int32_t>();
  a.d.opart = opart.data_ptr<float>(); a.d.lpart = lpart.data_ptr<float>(); a.d.out = out.data_ptr(); a.d.lse = lse.data_ptr<float>();
  a.d.B = (int)g.B; a.d.H = (int)H; a.d.Hg = (int)g.hg; a.d.Rn = (int)g.Rn; a.d.ldkv = g.ld;
  a.d.window = (int)window; a.d.scale = (float)scale; a.d.nspan = ns; a.d.out32 = out_fp32 ? 1 : 0;
  a.table = table.data_ptr<int32_t>(); a.npages = npages.data_ptr<int32_t>(); a.pos0v = pos0.data_ptr<int32_t>();
  a.P = (int)g.P; a.S = (int)g.S; a.maxp = (int)g.maxp;
  if (fp8) {
    a.d.qscale = qscale->data_ptr<float>(); a.d.vscale = vscale->data_ptr<float>();
    a.d.sc_head = g.S; a.d.sc_batch = qscale->stride(0);
    launched(xdot_flash_paged8_launch(&a, dt_code(rows.scalar_type()), (int)g.D, cur_stream(rows)), what);
  } else {
    launched(xdot_flash_paged_launch(&a, dt_code(rows.scalar_type()), (int)g.D, cur_stream(rows)), what);
  }
  return {out, lse};
}

std::tuple<at::Tensor, at::Tensor> flash_decode_paged(const at::Tensor& rows, const at::Tensor& qpool, const at::Tensor& vpool,
                                                      const at::Tensor& pool_pos, const at::Tensor& table, const at::Tensor& npages,
                                                      const at::Tensor& pos0, int64_t window, int64_t H, double scale, int64_t Hg,
                                                      int64_t nsplit, bool out_fp32, int64_t max_pages) {
  Range rr_("xdot.flash_decode_paged");
  return paged_call("xdot.flash_decode_paged: ", "flash_decode_paged", rows, qpool, vpool, nullptr, nullptr, pool_pos, table, npages,
                    pos0, window, H, scale, Hg, nsplit, out_fp32, max_pages);
}

std::tuple<at::Tensor, at::Tensor> flash_decode_paged_fp8(const at::Tensor& rows, const at::Tensor& qpool, const at::Tensor& vpool,
                                                          const at::Tensor& qscale, const at::Tensor& vscale,
                                                          const at::Tensor& pool_pos, const at::Tensor& table,
                                                          const at::Tensor& npages, const at::Tensor& pos0, int64_t window,
                                                          int64_t H, double scale, int64_t Hg, int64_t nsplit, bool out_fp32,
                                                          int64_t max_pages) {
  Range rr_("xdot.flash_decode_paged_fp8");
  return paged_call("xdot.flash_decode_paged_fp8: ", "flash_decode_paged_fp8", rows, qpool, vpool, &qscale, &vscale, pool_pos, table,
                    npages, pos0, window, H, scale, Hg, nsplit, out_fp32, max_pages);
}

// spans plan_decode_paged gives this shape on the current device
int64_t flash_decode_paged_plan(int64_t B, int64_t Hg, int64_t G, int64_t Rn, int64_t max_pages, int64_t S) {
  const int nt = decode_row_tiles(G, Rn);
  TORCH_CHECK(nt > 0 && B > 0 && Hg > 0 && max_pages > 0 && paged_page_size_ok(S), "xdot.flash_decode_paged_plan: shape");
  return plan_decode_paged(B, Hg, nt, max_pages, S, xdot_num_cus());
}

// the same for an fp8 pool of head dim D (plan_decode_paged_fp8)
int64_t flash_decode_paged_fp8_plan(int64_t B, int64_t Hg, int64_t G, int64_t Rn, int64_t D, int64_t max_pages, int64_t S) {
  const int nt = decode_row_tiles(G, Rn);
  TORCH_CHECK(nt > 0 && B > 0 && Hg > 0 && D > 0 && max_pages > 0 && paged_page_size_ok(S), "xdot.flash_decode_paged_fp8_plan: shape");
  return plan_decode_paged_fp8(B, Hg, nt, (int)D, max_pages, S, xdot_num_cus());
}

// rows (B, n, 2*Hg*D) 16-bit, a row view of row_view.h -> e4m3 bytes and per-chunk scales in slots
// [at, at + n) of an fp8 cache: qv8 (B, cap, 2*Hg*D) float8_e4m3fn, scales (B, 2*Hg, cap) fp32, both contiguous
void cache_quant(const at::Tensor& rows, at::Tensor& qv8, at::Tensor& scales, int64_t at_, int64_t Hg) {
  Range rr_("xdot.cache_quant");
  const char* op = "xdot.cache_quant: ";
  TORCH_CHECK(rows.is_cuda() && rows.dim() == 3 && (rows.scalar_type() == at::kBFloat16 || rows.scalar_type() == at::kHalf), op,
              "rows must be a bf16 / fp16 (B, n, 2*Hg*D) tensor on a GPU");
  const int64_t B = rows.size(0), n = rows.size(1), C = rows.size(2);
  TORCH_CHECK(Hg > 0 && C % (2 * Hg) == 0, op, "the row width ", C, " must be a multiple of 2*Hg = ", 2 * Hg);
  const int64_t D = C / (2 * Hg);
  TORCH_CHECK(D == 32 || D == 64 || D == 96 || D == 128, op, "head dim must be 32 / 64 / 96 / 128, got ", D);
  const auto v = row_view(rows, B, n, C, rows, false, "cache_quant", "rows");
  TORCH_CHECK(v.vec, op, "rows must start and step on 16-byte boundaries");
  TORCH_CHECK(qv8.is_cuda() && qv8.device() == rows.device() && qv8.scalar_type() == at::kFloat8_e4m3fn && qv8.dim() == 3 &&
                  qv8.size(0) == B && qv8.size(2) == C && qv8.is_contiguous() && aligned16(qv8.data_ptr()),
              op, "qv8 must be a contiguous float8_e4m3fn (B, capacity, 2*Hg*D) = (", B, ", capacity, ", C, ") tensor on the rows' GPU");
  const int64_t cap = qv8.size(1);
  TORCH_CHECK(scales.is_cuda() && scales.device() == rows.device() && scales.scalar_type() == at::kFloat && scales.dim() == 3 &&
                  scales.size(0) == B && scales.size(1) == 2 * Hg && scales.size(2) == cap && scales.is_contiguous(),
              op, "scales must be a contiguous fp32 (B, 2*Hg, capacity) = (", B, ", ", 2 * Hg, ", ", cap, ") tensor on the rows' GPU");
  TORCH_CHECK(at_ >= 0 && at_ + n <= cap, op, "slots [", at_, ", ", at_ + n, ") outside the capacity ", cap);
  TORCH_CHECK(cap < (1LL << 31) && n < (1LL << 31) && B < (1LL << 31), op, "cache too large");
  if (B == 0 || n == 0) return;
  QuantArgs a{};
  a.rows = rows.data_ptr(); a.qv8 = qv8.data_ptr(); a.scales = scales.data_ptr<float>();
  a.sb = v.sb; a.sr = v.sr; a.B = (int)B; a.n = (int)n; a.chunks = (int)(2 * Hg); a.cap = (int)cap; a.at = (int)at_;
  c10::DeviceGuard guard(rows.device());
  launched(xdot_cache_quant_launch(&a, dt_code(rows.scalar_type()), (int)D, cur_stream(rows)), "cache_quant");
}

// rows (N, 2*Hg*D) 16-bit of unit inner stride, starting and stepping on 16-byte boundaries -> e4m3 bytes, per-chunk
// scales and positions at the flat slots `slots` (N,) int32 (page * S + slot; outside the pool: skipped) of an fp8
// pool: qv8 (P, S, 2*Hg*D) float8_e4m3fn, scales (P, 2*Hg, S) fp32, pool_pos (P, S) int32, all contiguous;
// positions (N,) int32
void cache_quant_paged(const at::Tensor& rows, at::Tensor& qv8, at::Tensor& scales, at::Tensor& pool_pos, const at::Tensor& slots,
                       const at::Tensor& positions, int64_t Hg) {
  Range rr_("xdot.cache_quant_paged");
  const char* op = "xdot.cache_quant_paged: ";
  TORCH_CHECK(rows.is_cuda() && rows.dim() == 2 && (rows.scalar_type() == at::kBFloat16 || rows.scalar_type() == at::kHalf), op,
              "rows must be a bf16 / fp16 (N, 2*Hg*D) tensor on a GPU");
  const int64_t N = rows.size(0), C = rows.size(1);
  TORCH_CHECK(Hg > 0 && C % (2 * Hg) == 0, op, "the row width ", C, " must be a multiple of 2*Hg = ", 2 * Hg);
  const int64_t D = C / (2 * Hg);
  TORCH_CHECK(D == 32 || D == 64 || D == 96 || D == 128, op, "head dim must be 32 / 64 / 96 / 128, got ", D);
  TORCH_CHECK(N <= 1 || (rows.stride(0) >= C && rows.stride(0) % 8 == 0), op, "rows must step on 16-byte boundaries without overlap");
  TORCH_CHECK(rows.stride(1) == 1 && aligned16(rows.data_ptr()), op, "rows must have unit inner stride and start on a 16-byte boundary");
  const int64_t sr = N > 1 ? rows.stride(0) : C;
  TORCH_CHECK(N == 0 || (N - 1) * sr + C <= avail_elems(rows), op, "row view out of bounds");
  for (const at::Tensor* t : {(const at::Tensor*)&qv8, (const at::Tensor*)&scales, (const at::Tensor*)&pool_pos, &slots, &positions})
    TORCH_CHECK(t->is_cuda() && t->device() == rows.device() && t->is_contiguous(), op, "every tensor must be contiguous on the rows' GPU");
  TORCH_CHECK(qv8.scalar_type() == at::kFloat8_e4m3fn && qv8.dim() == 3 && qv8.size(0) > 0 && qv8.size(2) == C && aligned16(qv8.data_ptr()),
              op, "qv8 must be a float8_e4m3fn (P, S, 2*Hg*D) = (P, S, ", C, ") tensor");
  const int64_t P = qv8.size(0), S = qv8.size(1);
  TORCH_CHECK(paged_page_size_ok(S), op, "the page size must be 32, 64, 128 or 256 slots, got ", S);
  TORCH_CHECK(scales.scalar_type() == at::kFloat && scales.dim() == 3 && scales.size(0) == P && scales.size(1) == 2 * Hg && scales.size(2) == S,
              op, "scales must be an fp32 (P, 2*Hg, S) = (", P, ", ", 2 * Hg, ", ", S, ") tensor");
  TORCH_CHECK(pool_pos.scalar_type() == at::kInt && pool_pos.dim() == 2 && pool_pos.size(0) == P && pool_pos.size(1) == S, op,
              "pool_pos must be an int32 (P, S) = (", P, ", ", S, ") tensor");
  for (const at::Tensor* t : {&slots, &positions})
    TORCH_CHECK(t->scalar_type() == at::kInt && t->dim() == 1 && t->size(0) == N, op, "slots and positions must be int32 (N,) = (", N,
                ",) tensors, got ", t->scalar_type(), " ", t->sizes());
  TORCH_CHECK(P * S < (1LL << 31) && N < (1LL << 31), op, "pool too large");
  if (N == 0) return;
  QuantPagedArgs a{};
  a.rows = rows.data_ptr(); a.qv8 = qv8.data_ptr(); a.scales = scales.data_ptr<float>(); a.pool_pos = pool_pos.data_ptr<int32_t>();
  a.slots = slots.data_ptr<int32_t>(); a.positions = positions.data_ptr<int32_t>();
  a.sr = sr; a.N = (int)N; a.chunks = (int)(2 * Hg); a.S = (int)S; a.nslots = (int)(P * S);
  c10::DeviceGuard guard(rows.device());
  launched(xdot_cache_quant_paged_launch(&a, dt_code(rows.scalar_type()), (int)D, cur_stream(rows)), "cache_quant_paged");
}

// spans plan_decode gives this shape on the current device
int64_t flash_decode_plan(int64_t B, int64_t Hg, int64_t G, int64_t Rn, int64_t Tcap) {
  const int nt = decode_row_tiles(G, Rn);
  TORCH_CHECK(nt > 0 && B > 0 && Hg > 0 && Tcap > 0, "xdot.flash_decode_plan: shape");
  return plan_decode(B, Hg, nt, Tcap, xdot_num_cus());
}
// the same for an fp8 cache of head dim D (plan_decode_fp8)
int64_t flash_decode_fp8_plan(int64_t B, int64_t Hg, int64_t G, int64_t Rn, int64_t D, int64_t Tcap) {
  const int nt = decode_row_tiles(G, Rn);
  TORCH_CHECK(nt > 0 && B > 0 && Hg > 0 && Tcap > 0 && D > 0, "xdot.flash_decode_fp8_plan: shape");
  return plan_decode_fp8(B, Hg, nt, (int)D, Tcap, xdot_num_cus());
}
// spans plan_extend gives this shape (head dim D) on the current device
int64_t flash_extend_plan(int64_t B, int64_t Hg, int64_t G, int64_t Rn, int64_t D, int64_t Tcap) {
  TORCH_CHECK(B > 0 && Hg > 0 && Rn > 0 && Tcap > 0 && D > 0 && extend_block_rows(G, (int)D) > 0, "xdot.flash_extend_plan: shape");
  return plan_extend(B, Hg, G, Rn, (int)D, Tcap, xdot_num_cus());
}
// the same over an fp8 cache (plan_extend_fp8)
int64_t flash_extend_fp8_plan(int64_t B, int64_t Hg, int64_t G, int64_t Rn, int64_t D, int64_t Tcap) {
  TORCH_CHECK(B > 0 && Hg > 0 && Rn > 0 && Tcap > 0 && D > 0 && extend_block_rows(G, (int)D) > 0, "xdot.flash_extend_fp8_plan: shape");
  return plan_extend_fp8(B, Hg, G, Rn, (int)D, Tcap, xdot_num_cus());
}

// ---- chunked launches (gather / reduce-scatter pipelining) ----------------------------
// column splits the row-block kernels would use for (R rows, T columns) under the 16-bit model —
// the partial / ring paths size their buffers with it
int64_t flash_splits(int64_t B, int64_t R, int64_t T, int64_t H, bool rows_kernel) {
  if (rows_kernel) return rows_split(B, R, T, H);
  return pick_split(((R + 127) / 128) * B * H, T, 512, 0);
}

// forward over this column chunk into partial slots [sp0, sp0 + nsplit) of opart / lpart
void flash_fwd_partial(const at::Tensor& rows, const at::Tensor& kc, const at::Tensor& vc, const OptT& bits,
                       const OptT& flags, int64_t H, double scale, at::Tensor& opart, at::Tensor& lpart, int64_t sp0,
                       int64_t nsplit, bool prescaled, int64_t fp32_mode, int64_t Hg) {
  Range rr_("xdot.flash_fwd_partial");
  const FlashGeom g = flash_check(rows, kc, vc, H, bits, flags, false, Hg);
  TORCH_CHECK(sp0 >= 0 && nsplit >= 1, "xdot.flash_fwd_partial: slots");
  const int ns = pick_split(1, g.T, 1, nsplit);  // clamps nsplit to the column tiles
  check_part(opart, sp0 + ns, g.B * g.R * g.C, "opart");
  check_part(lpart, sp0 + ns, g.B * H * g.R, "lpart");
  auto a = fwd_args(g, rows, kc, vc, bits, flags, H, scale, prescaled, fp32_mode);
  a.nsplit = ns; a.sp0 = (int)sp0; a.force_partial = 1;
  a.opart = opart.data_ptr<float>(); a.lpart = lpart.data_ptr<float>();
  c10::DeviceGuard guard(rows.device());
  launched(xdot_flash_fwd_launch(&a, dt_code(rows.scalar_type()), (int)g.D, cur_stream(rows)), "flash_fwd_partial");
}

// merge all S slots of opart (S, B, R, C) / lpart into a.out (dtype dt) or a.out32, and a.lse
void combine(xdot::fa::FwdArgs& a, const at::Tensor& opart, const at::Tensor& lpart, int64_t B, int64_t H, int64_t R,
             int64_t C, int dt, const char* op) {
  const int64_t S = opart.size(0);
  check_part(opart, S, B * R * C, "opart");
  check_part(lpart, S, B * H * R, "lpart");
  a.B = (int)B; a.H = (int)H; a.R = (int)R; a.nsplit = (int)S;
  a.opart = opart.data_ptr<float>(); a.lpart = lpart.data_ptr<float>();
  c10::DeviceGuard guard(opart.device());
  launched(xdot_flash_fwd_combine_launch(&a, dt, (int)(C / H), cur_stream(opart)), op);
}

// merge all slots of opart / lpart -> (out in like's dtype, lse)
std::tuple<at::Tensor, at::Tensor> flash_fwd_combine(const at::Tensor& opart, const at::Tensor& lpart, int64_t H,
                                                     const at::Tensor& like) {
  Range rr_("xdot.flash_fwd_combine");
  TORCH_CHECK(like.dim() == 3 && like.is_cuda(), "xdot.flash_fwd_combine: like (B, R, C)");
  TORCH_CHECK(H > 0 && like.size(2) % H == 0, "xdot.flash_fwd_combine: H");
  auto out = at::empty_like(like);
  auto lse = at::empty({like.size(0), H, like.size(1)}, like.options().dtype(at::kFloat));
  xdot::fa::FwdArgs a{};
  a.out = out.data_ptr(); a.lse = lse.data_ptr<float>();
  combine(a, opart, lpart, like.size(0), H, like.size(1), like.size(2), dt_code(like.scalar_type()), "flash_fwd_combine");
  return {out, lse};
}

// merge all slots of opart / lpart into slot 0 in fp32 (the running partial of the ring
// forward: two slots of memory per block instead of one per ring step).  O is merged in place
// (each element is read and written by one thread); the merged LSE goes to lrun (lpart slot 0
// is still read by the other threads of its row) and is copied back by the caller.
void flash_fwd_merge(at::Tensor& opart, const at::Tensor& lpart, at::Tensor& lrun, int64_t H) {
  Range rr_("xdot.flash_fwd_merge");
  TORCH_CHECK(opart.dim() == 4 && opart.is_cuda(), "xdot.flash_fwd_merge: opart (S, B, R, C)");
  const int64_t B = opart.size(1), R = opart.size(2), C = opart.size(3);
  TORCH_CHECK(H > 0 && C % H == 0 && (C / H) % 32 == 0, "xdot.flash_fwd_merge: H");
  TORCH_CHECK(lrun.is_cuda() && lrun.is_contiguous() && lrun.scalar_type() == at::kFloat && lrun.numel() == B * H * R,
              "xdot.flash_fwd_merge: lrun (B, H, R) fp32");
  xdot::fa::FwdArgs a{};
  a.out32 = opart.data_ptr<float>(); a.lse = lrun.data_ptr<float>();
  combine(a, opart, lpart, B, H, R, C, xdot::DT_BF16, "flash_fwd_merge");  // dtype only selects the (unused) 16-bit output path
}

// row-side grads of this column chunk into partial slots [sp0, sp0 + nsplit) of dpart
void flash_bwd_rows_partial(const at::Tensor& dout, const at::Tensor& rows, const at::Tensor& kc, const at::Tensor& vc,
                            const at::Tensor& lse, const at::Tensor& delta, const OptT& bits, const OptT& flags, int64_t H,
                            double scale, at::Tensor& dpart, int64_t sp0, int64_t nsplit, bool prescaled,
                            int64_t fp32_mode, int64_t Hg) {
  Range rr_("xdot.flash_bwd_rows_partial");
  const FlashGeom g = flash_check(rows, kc, vc, H, bits, flags, false, Hg);
  check_bhr(delta, g.B, H, g.R, rows.device(), "xdot.flash_bwd_rows_partial: delta");
  TORCH_CHECK(sp0 >= 0 && nsplit >= 1, "xdot.flash_bwd_rows_partial: slots");
  const int ns = pick_split(1, g.T, 1, nsplit);
  check_part(dpart, sp0 + ns, g.B * g.R * g.C, "dpart");
  auto a = bwd_args(g, dout, rows, kc, vc, lse, bits, flags, H, scale, prescaled, fp32_mode);
  a.delta = delta.data_ptr<float>();
  a.nsplit = ns; a.sp0 = (int)sp0; a.force_partial = 1; a.dpart = dpart.data_ptr<float>();
  c10::DeviceGuard guard(rows.device());
  launched(xdot_flash_bwd_rows_launch(&a, dt_code(rows.scalar_type()), (int)g.D, cur_stream(rows)),
           "flash_bwd_rows_partial");
}

// Σ of all dpart slots -> (B, R, C) in like's dtype
at::Tensor flash_bwd_rows_sum(const at::Tensor& dpart, int64_t H, const at::Tensor& like) {
  Range rr_("xdot.flash_bwd_rows_sum");
  const int64_t B = like.size(0), R = like.size(1), C = like.size(2), S = dpart.size(0);
  check_part(dpart, S, B * R * C, "dpart");
  auto out = at::empty_like(like);
  xdot::fa::BwdArgs a{};
  a.drows = out.data_ptr(); a.dpart = dpart.data_ptr<float>();
  a.B = (int)B; a.H = (int)H; a.R = (int)R; a.nsplit = (int)S;
  c10::DeviceGuard guard(like.device());
  launched(xdot_flash_bwd_rows_sum_launch(&a, dt_code(like.scalar_type()), (int)(C / H), cur_stream(like)),
           "flash_bwd_rows_sum");
  return out;
}

}  // namespace

TORCH_LIBRARY_IMPL(xdot, CompositeExplicitAutograd, m) {
  m.impl("flash_splits", &flash_splits);
  m.impl("flash_fwd_plan", &flash_fwd_plan);
  m.impl("flash_cols_plan", &flash_cols_plan);
  m.impl("flash_rows_plan", &flash_rows_plan);
  m.impl("flash_decode_plan", &flash_decode_plan);
  m.impl("flash_decode_fp8_plan", &flash_decode_fp8_plan);
  m.impl("flash_decode_paged_plan", &flash_decode_paged_plan);
  m.impl("flash_decode_paged_fp8_plan", &flash_decode_paged_fp8_plan);
  m.impl("flash_extend_plan", &flash_extend_plan);
  m.impl("flash_extend_fp8_plan", &flash_extend_fp8_plan);
}

TORCH_LIBRARY_IMPL(xdot, CUDA, m) {
  m.impl("flash_fwd", &flash_fwd);
  m.impl("flash_decode", &flash_decode);
  m.impl("flash_decode_fp8", &flash_decode_fp8);
  m.impl("flash_decode_paged", &flash_decode_paged);
  m.impl("flash_decode_paged_fp8", &flash_decode_paged_fp8);
  m.impl("flash_extend", &flash_extend);
  m.impl("flash_extend_fp8", &flash_extend_fp8);
  m.impl("cache_quant", &cache_quant);
  m.impl("cache_quant_paged", &cache_quant_paged);
  m.impl("flash_bwd_cols", &flash_bwd_cols);
  m.impl("flash_bwd_rows", &flash_bwd_rows);
  m.impl("flash_bwd_delta", &flash_bwd_delta);
  m.impl("flash_bwd_prep", &flash_bwd_prep);
  m.impl("sum_partials", &sum_partials);
  m.impl("sum_partials_into", &sum_partials_into);
  m.impl("flash_prescale", &flash_prescale);
  m.impl("flash_fwd_partial", &flash_fwd_partial);
  m.impl("flash_fwd_combine", &flash_fwd_combine);
  m.impl("flash_fwd_merge", &flash_fwd_merge);
  m.impl("flash_bwd_rows_partial", &flash_bwd_rows_partial);
  m.impl("flash_bwd_rows_sum", &flash_bwd_rows_sum);
}
