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
// of 1024 floats
float* sbuf_ptr(const OptT& sbuf, const FlashGeom& g, int64_t H, const at::Tensor& rows, int64_t fp32_mode,
                const char* what) {
  if (!sbuf.has_value() || !sbuf->defined()) return nullptr;
  const auto& t = *sbuf;
  TORCH_CHECK(rows.scalar_type() == at::kFloat && (fp32_mode == 0 || fp32_mode == 1), what,
              ": the score buffer is an fp32 (exact or split) feature");
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
  float* dsb = sbuf_ptr(dsbuf, g, H, rows, fp32_mode, "xdot.flash_bwd_cols (dS buffer)");
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
  float* dsb = sbuf_ptr(dsbuf, g, H, rows, fp32_mode, "xdot.flash_bwd_rows (dS buffer)");
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
}

TORCH_LIBRARY_IMPL(xdot, CUDA, m) {
  m.impl("flash_fwd", &flash_fwd);
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
