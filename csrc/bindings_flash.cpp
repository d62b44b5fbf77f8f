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

// a contiguous fp32 (B, H, R) tensor (lse, lse2, delta) on the launch's device
void check_bhr(const at::Tensor& t, int64_t B, int64_t H, int64_t R, const at::Device& dev, const char* what) {
  TORCH_CHECK(t.is_contiguous() && t.scalar_type() == at::kFloat && t.numel() == B * H * R && t.device() == dev, what);
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

// rotary table: cos / sin (R, D/2) fp32 of double(offset + row) * inv_freq[i] (csrc/rope.hip)
std::tuple<at::Tensor, at::Tensor> rope_table(int64_t R, int64_t D, int64_t offset, const at::Tensor& inv_freq) {
  Range rr_("xdot.rope_table");
  TORCH_CHECK(D >= 2 && D % 2 == 0 && D < (1LL << 31), "xdot.rope_table: head dim must be even, got ", D);
  TORCH_CHECK(R >= 0 && offset >= 0 && offset + R <= 2147483647LL, "xdot.rope_table: positions must stay below 2^31");
  TORCH_CHECK(inv_freq.is_cuda() && inv_freq.scalar_type() == at::kDouble && inv_freq.is_contiguous() &&
                  inv_freq.numel() == D / 2,
              "xdot.rope_table: inv_freq must be a contiguous fp64 device tensor of D/2 entries");
  auto cosb = at::empty({R, D / 2}, inv_freq.options().dtype(at::kFloat));
  auto sinb = at::empty_like(cosb);
  c10::DeviceGuard guard(inv_freq.device());
  launched(xdot_rope_table_launch(cosb.data_ptr<float>(), sinb.data_ptr<float>(), inv_freq.data_ptr<double>(), (int)R,
                                  (int)(D / 2), offset, cur_stream(inv_freq)),
           "rope_table", "shape");
  return {cosb, sinb};
}

// out = alpha * rotate(x): x, out (B, R, H*D) with unit inner stride and any row / batch strides
// (the q half of a packed [q|v] buffer, a rank slot of the gather buffer); out may be x itself
void rope_apply(const at::Tensor& x, const at::Tensor& cosb, const at::Tensor& sinb, int64_t H, bool inverse,
                double alpha, at::Tensor& out) {
  Range rr_("xdot.rope_apply");
  TORCH_CHECK(x.is_cuda() && out.is_cuda() && cosb.is_cuda() && sinb.is_cuda() && out.device() == x.device() &&
                  cosb.device() == x.device() && sinb.device() == x.device(),
              "xdot.rope_apply: tensors of one GPU required");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kHalf || x.scalar_type() == at::kFloat,
              "xdot.rope_apply: bf16/fp16/fp32 only");
  TORCH_CHECK(x.dim() == 3 && out.sizes() == x.sizes() && out.scalar_type() == x.scalar_type(),
              "xdot.rope_apply: x and out must be (B, R, H*D) of one dtype");
  const int64_t B = x.size(0), R = x.size(1), C = x.size(2);
  TORCH_CHECK(H > 0 && C % H == 0 && (C / H) % 2 == 0, "xdot.rope_apply: H*D with an even head dim D, got C=", C, " H=", H);
  TORCH_CHECK(B < (1LL << 31) && R < (1LL << 31) && C < (1LL << 31) && B * H < (1LL << 31), "xdot.rope_apply: too large");
  const int64_t D = C / H;
  TORCH_CHECK(cosb.scalar_type() == at::kFloat && sinb.scalar_type() == at::kFloat && cosb.is_contiguous() &&
                  sinb.is_contiguous() && cosb.dim() == 2 && cosb.size(0) == R && cosb.size(1) == D / 2 &&
                  sinb.sizes() == cosb.sizes(),
              "xdot.rope_apply: cos / sin must be contiguous fp32 (R, D/2)");
  if (x.numel() == 0) return;
  const int64_t V = 16 / (int64_t)x.element_size();
  int64_t st[4];  // x batch, x row, out batch, out row (a stride of a size-1 dim is never used)
  bool vec = aligned16(x.data_ptr()) && aligned16(out.data_ptr()) && aligned16(cosb.data_ptr()) && aligned16(sinb.data_ptr());
  int k = 0;
  for (const at::Tensor* t : {&x, static_cast<const at::Tensor*>(&out)}) {
    TORCH_CHECK(t->stride(2) == 1 || C == 1, "xdot.rope_apply: the last dimension must have stride 1");
    const int64_t sb = B > 1 ? t->stride(0) : 0, sr = R > 1 ? t->stride(1) : 0;
    TORCH_CHECK(sb >= 0 && sr >= 0, "xdot.rope_apply: negative strides");
    TORCH_CHECK((B - 1) * sb + (R - 1) * sr + C <= avail_elems(*t), "xdot.rope_apply: view out of bounds");
    vec = vec && sb % V == 0 && sr % V == 0;
    st[k++] = sb;
    st[k++] = sr;
  }
  // in place (the same view) or disjoint: a lane reads only the pairs it writes
  if (x.data_ptr() == out.data_ptr()) {
    TORCH_CHECK(st[0] == st[2] && st[1] == st[3], "xdot.rope_apply: an in-place out must be the same view as x");
  } else {
    const char* xb = static_cast<const char*>(x.data_ptr());
    const char* ob = static_cast<const char*>(out.data_ptr());
    const int64_t es = (int64_t)x.element_size();
    const int64_t xe = ((B - 1) * st[0] + (R - 1) * st[1] + C) * es, oe = ((B - 1) * st[2] + (R - 1) * st[3] + C) * es;
    TORCH_CHECK(xb + xe <= ob || ob + oe <= xb, "xdot.rope_apply: x and out overlap");
  }
  xdot::RopeArgs a{};
  a.x = x.data_ptr(); a.out = out.data_ptr();
  a.cos = cosb.data_ptr<float>(); a.sin = sinb.data_ptr<float>();
  a.B = (int)B; a.R = (int)R; a.H = (int)H; a.D = (int)D;
  a.xs_b = st[0]; a.xs_r = st[1]; a.os_b = st[2]; a.os_r = st[3];
  a.alpha = (float)alpha; a.inverse = inverse ? 1 : 0;
  const int64_t half = D / 2;
  const int mode = !vec ? 0 : (half % V == 0 ? 1 : (half > V ? 2 : 0));
  c10::DeviceGuard guard(x.device());
  launched(xdot_rope_apply_launch(&a, dt_code(x.scalar_type()), mode, cur_stream(x)), "rope_apply", "shape");
}

// ---- per-head RMSNorm fused with the rotation (csrc/headnorm.hip) ----
// the (B, R, C) views of one headnorm call: unit inner stride, any non-negative row / batch strides,
// inside their storage (as rope_apply).  Returns batch / row strides per view and whether every
// view is on the 16-byte grid
struct HnViews { int64_t st[3][2]; bool vec; };

HnViews hn_views(std::initializer_list<const at::Tensor*> ts, int64_t B, int64_t R, int64_t C, const char* op) {
  HnViews v{};
  v.vec = true;
  const at::Tensor& first = **ts.begin();
  const int64_t V = 16 / (int64_t)first.element_size();
  int k = 0;
  for (const at::Tensor* t : ts) {
    TORCH_CHECK(t->is_cuda() && t->device() == first.device(), "xdot.", op, ": tensors of one GPU required");
    TORCH_CHECK(t->dim() == 3 && t->size(0) == B && t->size(1) == R && t->size(2) == C &&
                    t->scalar_type() == first.scalar_type(),
                "xdot.", op, ": the views must be (B, R, H*D) of one dtype");
    TORCH_CHECK(t->stride(2) == 1 || C == 1, "xdot.", op, ": the last dimension must have stride 1");
    const int64_t sb = B > 1 ? t->stride(0) : 0, sr = R > 1 ? t->stride(1) : 0;
    TORCH_CHECK(sb >= 0 && sr >= 0, "xdot.", op, ": negative strides");
    TORCH_CHECK((B - 1) * sb + (R - 1) * sr + C <= avail_elems(*t), "xdot.", op, ": view out of bounds");
    v.vec = v.vec && aligned16(t->data_ptr()) && sb % V == 0 && sr % V == 0;
    v.st[k][0] = sb;
    v.st[k][1] = sr;
    ++k;
  }
  return v;
}

// `dst` is written while `src` is read: the same view (in place) or disjoint memory
void hn_no_overlap(const at::Tensor& src, const int64_t* ss, const at::Tensor& dst, const int64_t* ds, int64_t B,
                   int64_t R, int64_t C, const char* op) {
  if (src.data_ptr() == dst.data_ptr()) {
    TORCH_CHECK(ss[0] == ds[0] && ss[1] == ds[1], "xdot.", op, ": an in-place output must be the same view as its input");
    return;
  }
  const char* sb = static_cast<const char*>(src.data_ptr());
  const char* db = static_cast<const char*>(dst.data_ptr());
  const int64_t es = (int64_t)src.element_size();
  const int64_t se = ((B - 1) * ss[0] + (R - 1) * ss[1] + C) * es, de = ((B - 1) * ds[0] + (R - 1) * ds[1] + C) * es;
  TORCH_CHECK(sb + se <= db || db + de <= sb, "xdot.", op, ": input and output overlap");
}

// weight (D,) in x's dtype or fp32; cos / sin both or neither, contiguous fp32 (R, D/2)
void hn_params(const at::Tensor& x, const at::Tensor& weight, const OptT& cosb, const OptT& sinb, int64_t R, int64_t D,
               const char* op) {
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kHalf || x.scalar_type() == at::kFloat,
              "xdot.", op, ": bf16/fp16/fp32 only");
  TORCH_CHECK(weight.is_cuda() && weight.device() == x.device() && weight.dim() == 1 && weight.size(0) == D &&
                  weight.is_contiguous() &&
                  (weight.scalar_type() == x.scalar_type() || weight.scalar_type() == at::kFloat),
              "xdot.", op, ": weight must be a contiguous (D,) = (", D, ",) tensor of x's dtype or fp32");
  const bool hc = cosb.has_value() && cosb->defined(), hs = sinb.has_value() && sinb->defined();
  TORCH_CHECK(hc == hs, "xdot.", op, ": cos and sin go together");
  if (hc) {
    TORCH_CHECK(D % 2 == 0, "xdot.", op, ": the rotation needs an even head dim, got ", D);
    TORCH_CHECK(cosb->is_cuda() && sinb->is_cuda() && cosb->device() == x.device() && sinb->device() == x.device() &&
                    cosb->scalar_type() == at::kFloat && sinb->scalar_type() == at::kFloat && cosb->is_contiguous() &&
                    sinb->is_contiguous() && cosb->dim() == 2 && cosb->size(0) == R && cosb->size(1) == D / 2 &&
                    sinb->sizes() == cosb->sizes(),
                "xdot.", op, ": cos / sin must be contiguous fp32 (R, D/2)");
  }
}

xdot::HeadNormPlan hn_plan(int64_t B, int64_t R, int64_t H, int64_t D, int64_t esize, const char* op) {
  xdot::HeadNormPlan p{};
  TORCH_CHECK(B < (1LL << 31) && R < (1LL << 31) && H * D < (1LL << 31) && B * H < (1LL << 31), "xdot.", op, ": too large");
  TORCH_CHECK(xdot_headnorm_plan((int)B, (int)R, (int)H, (int)D, (int)esize, &p) == 0, "xdot.", op,
              ": head dim ", D, " is too wide (one wave reduces a head row: D <= ", 64 * 2 * (16 / esize), ")");
  return p;
}

// [G, rows per workgroup, forward grid x, y, backward grid x, y] of a headnorm launch (no launch)
std::vector<int64_t> headnorm_plan(int64_t B, int64_t R, int64_t H, int64_t D, at::ScalarType dtype) {
  TORCH_CHECK(B > 0 && R > 0 && H > 0 && D > 0, "xdot.headnorm_plan: shape");
  const auto p = hn_plan(B, R, H, D, (int64_t)c10::elementSize(dtype), "headnorm_plan");
  return {p.G, p.rows_per_wg, p.fwd_gx, p.fwd_gy, p.bwd_gx, p.bwd_gy};
}

// out = alpha * rotate(x * rstd * weight) per head of x (B, R, H*D) (rotation with a table only);
// returns rstd (B, R, H) fp32 and, with save, a contiguous bit copy of x (else an empty tensor).
// out may be x itself (the same view)
std::tuple<at::Tensor, at::Tensor> headnorm_fwd(const at::Tensor& x, const at::Tensor& weight, const OptT& cosb,
                                                const OptT& sinb, int64_t H, double eps, double alpha, at::Tensor& out,
                                                bool save) {
  Range rr_("xdot.headnorm_fwd");
  TORCH_CHECK(x.is_cuda() && x.dim() == 3, "xdot.headnorm_fwd: x must be a (B, R, H*D) GPU tensor");
  const int64_t B = x.size(0), R = x.size(1), C = x.size(2);
  TORCH_CHECK(H > 0 && C > 0 && C % H == 0, "xdot.headnorm_fwd: H*D features, got C=", C, " H=", H);
  TORCH_CHECK(eps > 0.0, "xdot.headnorm_fwd: eps must be positive");
  const int64_t D = C / H;
  hn_params(x, weight, cosb, sinb, R, D, "headnorm_fwd");
  const HnViews v = hn_views({&x, static_cast<const at::Tensor*>(&out)}, B, R, C, "headnorm_fwd");
  hn_no_overlap(x, v.st[0], out, v.st[1], B, R, C, "headnorm_fwd");
  auto rstd = at::empty({B, R, H}, x.options().dtype(at::kFloat));
  auto saved = save ? at::empty({B, R, C}, x.options()) : at::empty({0}, x.options());
  if (x.numel() == 0) return {rstd, saved};
  hn_plan(B, R, H, D, (int64_t)x.element_size(), "headnorm_fwd");
  const bool rot = cosb.has_value() && cosb->defined();
  xdot::HeadNormArgs a{};
  a.x = x.data_ptr(); a.out = out.data_ptr(); a.save = save ? saved.data_ptr() : nullptr;
  a.rstd = rstd.data_ptr<float>(); a.w = weight.data_ptr(); a.w_f32 = weight.scalar_type() == at::kFloat;
  a.cos = rot ? cosb->data_ptr<float>() : nullptr; a.sin = rot ? sinb->data_ptr<float>() : nullptr;
  a.B = (int)B; a.R = (int)R; a.H = (int)H; a.D = (int)D;
  a.xs_b = v.st[0][0]; a.xs_r = v.st[0][1]; a.os_b = v.st[1][0]; a.os_r = v.st[1][1];
  a.alpha = (float)alpha; a.eps = (float)eps; a.inv_d = 1.0f / (float)D;
  c10::DeviceGuard guard(x.device());
  launched(xdot_headnorm_fwd_launch(&a, dt_code(x.scalar_type()), v.vec ? 1 : 0, cur_stream(x)), "headnorm_fwd", "shape");
  return {rstd, saved};
}

// dx = rstd * (gw - xh * mean(gw . xh)) with gy = alpha * rotate^-1(g), xh = x * rstd, gw = gy * weight,
// written to dx (may be g itself); returns dw = sum gy . xh in weight's dtype (need_dw), else empty.
// Two launches: the pass, which leaves one fp32 (D,) partial per workgroup, and their ordered sum
at::Tensor headnorm_bwd(const at::Tensor& g, const at::Tensor& x, const at::Tensor& rstd, const at::Tensor& weight,
                        const OptT& cosb, const OptT& sinb, int64_t H, double alpha, at::Tensor& dx, bool need_dw) {
  Range rr_("xdot.headnorm_bwd");
  TORCH_CHECK(g.is_cuda() && g.dim() == 3, "xdot.headnorm_bwd: g must be a (B, R, H*D) GPU tensor");
  const int64_t B = g.size(0), R = g.size(1), C = g.size(2);
  TORCH_CHECK(H > 0 && C > 0 && C % H == 0, "xdot.headnorm_bwd: H*D features, got C=", C, " H=", H);
  const int64_t D = C / H;
  hn_params(g, weight, cosb, sinb, R, D, "headnorm_bwd");
  const HnViews v = hn_views({&g, &x, static_cast<const at::Tensor*>(&dx)}, B, R, C, "headnorm_bwd");
  hn_no_overlap(g, v.st[0], dx, v.st[2], B, R, C, "headnorm_bwd");
  hn_no_overlap(x, v.st[1], dx, v.st[2], B, R, C, "headnorm_bwd");
  TORCH_CHECK(x.data_ptr() != dx.data_ptr() || x.numel() == 0, "xdot.headnorm_bwd: dx may overwrite g, not x");
  TORCH_CHECK(rstd.is_cuda() && rstd.device() == g.device() && rstd.scalar_type() == at::kFloat && rstd.is_contiguous() &&
                  rstd.dim() == 3 && rstd.size(0) == B && rstd.size(1) == R && rstd.size(2) == H,
              "xdot.headnorm_bwd: rstd must be contiguous fp32 (B, R, H)");
  auto dw = need_dw ? at::empty({D}, weight.options()) : at::empty({0}, weight.options());
  if (g.numel() == 0) {
    if (need_dw) dw.zero_();
    return dw;
  }
  const auto p = hn_plan(B, R, H, D, (int64_t)g.element_size(), "headnorm_bwd");
  const int64_t nparts = (int64_t)p.bwd_gx * p.bwd_gy;
  auto part = at::empty({nparts, D}, g.options().dtype(at::kFloat));
  const bool rot = cosb.has_value() && cosb->defined();
  xdot::HeadNormArgs a{};
  a.x = x.data_ptr(); a.g = g.data_ptr(); a.out = dx.data_ptr(); a.rstd = rstd.data_ptr<float>();
  a.w = weight.data_ptr(); a.w_f32 = weight.scalar_type() == at::kFloat; a.part = part.data_ptr<float>();
  a.cos = rot ? cosb->data_ptr<float>() : nullptr; a.sin = rot ? sinb->data_ptr<float>() : nullptr;
  a.B = (int)B; a.R = (int)R; a.H = (int)H; a.D = (int)D;
  a.gs_b = v.st[0][0]; a.gs_r = v.st[0][1]; a.xs_b = v.st[1][0]; a.xs_r = v.st[1][1];
  a.os_b = v.st[2][0]; a.os_r = v.st[2][1];
  a.alpha = (float)alpha; a.inv_d = 1.0f / (float)D;
  c10::DeviceGuard guard(g.device());
  launched(xdot_headnorm_bwd_launch(&a, dt_code(g.scalar_type()), v.vec ? 1 : 0, cur_stream(g)), "headnorm_bwd", "shape");
  if (need_dw)
    launched(xdot_headnorm_dw_launch(part.data_ptr<float>(), dw.data_ptr(), (int)nparts, (int)D, dt_code(weight.scalar_type()),
                                     cur_stream(g)),
             "headnorm_dw", "shape");
  return dw;
}

// ---- attention sinks (csrc/sink.hip) ----
// sinks (H,): fp32, bf16 or fp16 on the launch's device (an fp32 master parameter beside 16-bit tensors)
void sink_param(const at::Tensor& sinks, int64_t H, const at::Device& dev, const char* op) {
  TORCH_CHECK(sinks.is_cuda() && sinks.device() == dev && sinks.dim() == 1 && sinks.size(0) == H && sinks.is_contiguous() &&
                  (sinks.scalar_type() == at::kFloat || sinks.scalar_type() == at::kBFloat16 ||
                   sinks.scalar_type() == at::kHalf),
              "xdot.", op, ": sinks must be a contiguous (H,) = (", H, ",) fp32 / bf16 / fp16 tensor on the same GPU");
}

// the fold of one sink logit per head into a finished forward, in place: lse' = logaddexp(lse, s_h),
// out' = sigmoid(lse - s_h) * out.  out: (B, R, H*D) with unit inner stride and 16-byte aligned
// rows (row / batch strides allowed), lse: contiguous fp32 (B, H, R)
void sink_fold(at::Tensor& out, at::Tensor& lse, const at::Tensor& sinks, int64_t H) {
  Range rr_("xdot.sink_fold");
  TORCH_CHECK(out.is_cuda() && out.dim() == 3, "xdot.sink_fold: out must be a (B, R, H*D) GPU tensor");
  TORCH_CHECK(out.scalar_type() == at::kBFloat16 || out.scalar_type() == at::kHalf || out.scalar_type() == at::kFloat,
              "xdot.sink_fold: bf16/fp16/fp32 only");
  const int64_t B = out.size(0), R = out.size(1), C = out.size(2);
  TORCH_CHECK(H > 0 && C > 0 && C % H == 0, "xdot.sink_fold: H*D features, got C=", C, " H=", H);
  const int64_t D = C / H;
  TORCH_CHECK(D >= 32 && D <= 384 && D % 8 == 0,
              "xdot.sink_fold: the head dim must be one the flash paths produce (32..384 in steps of 8), got ", D);
  TORCH_CHECK(B < (1LL << 31) && R < (1LL << 31) && C < (1LL << 31), "xdot.sink_fold: too large");
  sink_param(sinks, H, out.device(), "sink_fold");
  TORCH_CHECK(lse.dim() == 3 && lse.size(0) == B && lse.size(1) == H && lse.size(2) == R,
              "xdot.sink_fold: lse must be (B, H, R) = (", B, ", ", H, ", ", R, ")");
  check_bhr(lse, B, H, R, out.device(), "xdot.sink_fold: lse must be a contiguous fp32 tensor on the same GPU");
  if (out.numel() == 0) return;
  const int64_t V = 16 / (int64_t)out.element_size();
  TORCH_CHECK(out.stride(2) == 1, "xdot.sink_fold: the last dimension must have stride 1");
  const int64_t sb = B > 1 ? out.stride(0) : 0, sr = R > 1 ? out.stride(1) : 0;
  TORCH_CHECK(sb >= 0 && sr >= 0, "xdot.sink_fold: negative strides");
  // (every (b, row) is written: two of them may not share memory)
  TORCH_CHECK((R == 1 || sr >= C) && (B == 1 || sb >= (R - 1) * sr + C), "xdot.sink_fold: the rows of out overlap");
  TORCH_CHECK((B - 1) * sb + (R - 1) * sr + C <= avail_elems(out), "xdot.sink_fold: view out of bounds");
  TORCH_CHECK(aligned16(out.data_ptr()) && sb % V == 0 && sr % V == 0,
              "xdot.sink_fold: out and its row / batch strides must be 16-byte aligned");
  xdot::SinkArgs a{};
  a.out = out.data_ptr(); a.lse = lse.data_ptr<float>(); a.sinks = sinks.data_ptr();
  a.s_dt = dt_code(sinks.scalar_type());
  a.B = (int)B; a.R = (int)R; a.H = (int)H; a.D = (int)D;
  a.os_b = sb; a.os_r = sr;
  c10::DeviceGuard guard(out.device());
  launched(xdot_sink_fold_launch(&a, dt_code(out.scalar_type()), cur_stream(out)), "sink_fold", "shape");
}

// ds (H,) fp32 = -sum_{b, r} exp(s_h - lse'[b, h, r]) * delta[b, h, r] from the folded lse' and the
// delta of the folded output: per-workgroup partials, then their ordered sum (two launches, no atomics)
at::Tensor sink_grad(const at::Tensor& delta, const at::Tensor& lse, const at::Tensor& sinks) {
  Range rr_("xdot.sink_grad");
  TORCH_CHECK(lse.is_cuda() && lse.dim() == 3 && delta.dim() == 3 && delta.sizes() == lse.sizes(),
              "xdot.sink_grad: delta and lse must be (B, H, R) GPU tensors");
  const int64_t B = lse.size(0), H = lse.size(1), R = lse.size(2);
  TORCH_CHECK(H > 0 && H <= 65535 && B < (1LL << 31) && R < (1LL << 31), "xdot.sink_grad: shape");
  check_bhr(lse, B, H, R, lse.device(), "xdot.sink_grad: lse must be contiguous fp32");
  check_bhr(delta, B, H, R, lse.device(), "xdot.sink_grad: delta must be contiguous fp32 on the same GPU");
  sink_param(sinks, H, lse.device(), "sink_grad");
  auto ds = at::empty({H}, lse.options());
  if (B * R == 0) return ds.zero_();
  const int nparts = xdot_sink_grad_parts((int)B, (int)R);
  TORCH_CHECK(nparts > 0, "xdot.sink_grad: too large");
  auto part = at::empty({H, (int64_t)nparts}, lse.options());
  xdot::SinkGradArgs a{};
  a.delta = delta.data_ptr<float>(); a.lse = lse.data_ptr<float>(); a.sinks = sinks.data_ptr();
  a.part = part.data_ptr<float>(); a.ds = ds.data_ptr<float>();
  a.s_dt = dt_code(sinks.scalar_type());
  a.B = (int)B; a.R = (int)R; a.H = (int)H; a.nparts = nparts;
  c10::DeviceGuard guard(lse.device());
  launched(xdot_sink_grad_launch(&a, cur_stream(lse)), "sink_grad", "shape");
  return ds;
}

// ---- gated attention (csrc/gate.hip) ----
// one (B, R, C) operand of the gate kernels: unit inner stride, non-negative row / batch strides,
// inside its storage; -> (batch stride, row stride) in elements, 0 for a dimension of size 1
struct GateView { int64_t sb, sr; bool vec; };
GateView gate_view(const at::Tensor& t, int64_t B, int64_t R, int64_t C, const at::Tensor& like, bool written,
                   const char* op, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device() && t.scalar_type() == like.scalar_type() && t.dim() == 3 &&
                  t.size(0) == B && t.size(1) == R && t.size(2) == C,
              "xdot.", op, ": ", name, " must be a (", B, ", ", R, ", ", C, ") tensor of o's dtype on the same GPU");
  if (t.numel() == 0) return {0, 0, true};
  TORCH_CHECK(C == 1 || t.stride(2) == 1, "xdot.", op, ": the last dimension of ", name, " must have stride 1");
  const int64_t sb = B > 1 ? t.stride(0) : 0, sr = R > 1 ? t.stride(1) : 0;
  TORCH_CHECK(sb >= 0 && sr >= 0, "xdot.", op, ": negative strides in ", name);
  if (written)  // (every (b, row) is written: two of them may not share memory)
    TORCH_CHECK((R == 1 || sr >= C) && (B == 1 || sb >= (R - 1) * sr + C), "xdot.", op, ": the rows of ", name, " overlap");
  TORCH_CHECK((B - 1) * sb + (R - 1) * sr + C <= avail_elems(t), "xdot.", op, ": view ", name, " out of bounds");
  const int64_t V = 16 / (int64_t)t.element_size();
  return {sb, sr, aligned16(t.data_ptr()) && sb % V == 0 && sr % V == 0};
}

// the bytes [lo, hi) a (B, R, C) view with these strides spans
struct GateSpan { uintptr_t lo, hi; };
GateSpan gate_span(const at::Tensor& t, const GateView& v) {
  const uintptr_t lo = reinterpret_cast<uintptr_t>(t.data_ptr());
  if (t.numel() == 0) return {lo, lo};
  const int64_t n = (t.size(0) - 1) * v.sb + (t.size(1) - 1) * v.sr + t.size(2);
  return {lo, lo + (uintptr_t)n * t.element_size()};
}
bool gate_disjoint(const GateSpan& a, const GateSpan& b) { return a.hi <= b.lo || b.hi <= a.lo; }

// 16-byte lane steps?  mode -1: where D, the pointers and the strides allow; 0: never (one element per
// step); 1: asked for -- the views must be aligned (checked here), D % V is left to the launcher
int gate_vec(int64_t mode, bool aligned, int64_t D, int64_t V, const char* op) {
  TORCH_CHECK(mode >= -1 && mode <= 1, "xdot.", op, ": mode must be -1 (auto), 0 (scalar) or 1 (vector)");
  if (mode == 0) return 0;
  if (mode == 1) {
    TORCH_CHECK(aligned, "xdot.", op, ": vector mode needs 16-byte aligned views and strides");
    return 1;
  }
  return aligned && D % V == 0;
}

int64_t gate_dims(const at::Tensor& o, const at::Tensor& g, int64_t H, const char* op, bool& headwise) {
  TORCH_CHECK(o.is_cuda() && o.dim() == 3, "xdot.", op, ": o must be a (B, R, H*D) GPU tensor");
  TORCH_CHECK(o.scalar_type() == at::kBFloat16 || o.scalar_type() == at::kHalf || o.scalar_type() == at::kFloat,
              "xdot.", op, ": bf16/fp16/fp32 only");
  const int64_t C = o.size(2);
  TORCH_CHECK(H > 0 && C > 0 && C % H == 0, "xdot.", op, ": H*D features, got C=", C, " H=", H);
  TORCH_CHECK(o.size(0) < (1LL << 31) && o.size(1) < (1LL << 31) && C < (1LL << 31), "xdot.", op, ": too large");
  TORCH_CHECK(g.dim() == 3 && (g.size(2) == C || g.size(2) == H), "xdot.", op, ": g must be (B, R, ", C, ") or (B, R, ", H, ")");
  headwise = g.size(2) != C;  // (D = 1: both kinds are the same thing; elementwise it is)
  return C / H;
}

// o' = o * sigmoid(g) into out (out of place: out may not share memory with o or g)
void gate_apply(const at::Tensor& o, const at::Tensor& g, int64_t H, at::Tensor& out, int64_t mode) {
  Range rr_("xdot.gate_apply");
  bool hw = false;
  const int64_t D = gate_dims(o, g, H, "gate_apply", hw);
  const int64_t B = o.size(0), R = o.size(1), C = o.size(2);
  const GateView vo = gate_view(o, B, R, C, o, false, "gate_apply", "o");
  const GateView vg = gate_view(g, B, R, hw ? H : C, o, false, "gate_apply", "g");
  const GateView vy = gate_view(out, B, R, C, o, true, "gate_apply", "out");
  if (o.numel() == 0) return;
  TORCH_CHECK(gate_disjoint(gate_span(out, vy), gate_span(o, vo)) && gate_disjoint(gate_span(out, vy), gate_span(g, vg)),
              "xdot.gate_apply: out may not share memory with o or g (out of place)");
  const int64_t V = 16 / (int64_t)o.element_size();
  const int vec = gate_vec(mode, vo.vec && vy.vec && (hw || vg.vec), D, V, "gate_apply");
  xdot::GateArgs a{};
  a.o = o.data_ptr(); a.g = g.data_ptr(); a.y = out.data_ptr();
  a.B = (int)B; a.R = (int)R; a.H = (int)H; a.D = (int)D; a.headwise = hw ? 1 : 0;
  a.os_b = vo.sb; a.os_r = vo.sr; a.gs_b = vg.sb; a.gs_r = vg.sr; a.ys_b = vy.sb; a.ys_r = vy.sr;
  c10::DeviceGuard guard(o.device());
  launched(xdot_gate_apply_launch(&a, dt_code(o.scalar_type()), vec, cur_stream(o)), "gate_apply", "shape");
}

// do = dy * sigmoid(g) into dout (which may be dy itself) and dg -> a new contiguous tensor shaped like g
at::Tensor gate_backward(const at::Tensor& dy, const at::Tensor& o, const at::Tensor& g, int64_t H, at::Tensor& dout,
                         int64_t mode) {
  Range rr_("xdot.gate_backward");
  bool hw = false;
  const int64_t D = gate_dims(o, g, H, "gate_backward", hw);
  const int64_t B = o.size(0), R = o.size(1), C = o.size(2);
  const GateView vo = gate_view(o, B, R, C, o, false, "gate_backward", "o");
  const GateView vg = gate_view(g, B, R, hw ? H : C, o, false, "gate_backward", "g");
  const GateView vd = gate_view(dy, B, R, C, o, false, "gate_backward", "dy");
  const GateView vy = gate_view(dout, B, R, C, o, true, "gate_backward", "dout");
  auto dg = at::empty({B, R, hw ? H : C}, o.options());
  if (o.numel() == 0) return dg;
  TORCH_CHECK(gate_disjoint(gate_span(dout, vy), gate_span(o, vo)) && gate_disjoint(gate_span(dout, vy), gate_span(g, vg)),
              "xdot.gate_backward: dout may not share memory with o or g");
  // (every element of do is written by the lane that read that element of dy: dy itself, or apart)
  TORCH_CHECK((dout.data_ptr() == dy.data_ptr() && vy.sb == vd.sb && vy.sr == vd.sr) ||
                  gate_disjoint(gate_span(dout, vy), gate_span(dy, vd)),
              "xdot.gate_backward: dout must be dy itself (same strides) or share no memory with it");
  const int64_t V = 16 / (int64_t)o.element_size();
  const int vec = gate_vec(mode, vo.vec && vy.vec && vd.vec && (hw || vg.vec), D, V, "gate_backward");
  xdot::GateArgs a{};
  a.o = o.data_ptr(); a.g = g.data_ptr(); a.dy = dy.data_ptr(); a.y = dout.data_ptr(); a.dg = dg.data_ptr();
  a.B = (int)B; a.R = (int)R; a.H = (int)H; a.D = (int)D; a.headwise = hw ? 1 : 0;
  a.os_b = vo.sb; a.os_r = vo.sr; a.gs_b = vg.sb; a.gs_r = vg.sr; a.ys_b = vy.sb; a.ys_r = vy.sr;
  a.ds_b = vd.sb; a.ds_r = vd.sr;
  c10::DeviceGuard guard(o.device());
  launched(xdot_gate_backward_launch(&a, dt_code(o.scalar_type()), vec, cur_stream(o)), "gate_backward", "shape");
  return dg;
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
  m.impl("headnorm_plan", &headnorm_plan);
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
  m.impl("rope_table", &rope_table);
  m.impl("rope_apply", &rope_apply);
  m.impl("headnorm_fwd", &headnorm_fwd);
  m.impl("headnorm_bwd", &headnorm_bwd);
  m.impl("sink_fold", &sink_fold);
  m.impl("sink_grad", &sink_grad);
  m.impl("gate_apply", &gate_apply);
  m.impl("gate_backward", &gate_backward);
  m.impl("flash_fwd_partial", &flash_fwd_partial);
  m.impl("flash_fwd_combine", &flash_fwd_combine);
  m.impl("flash_fwd_merge", &flash_fwd_merge);
  m.impl("flash_bwd_rows_partial", &flash_bwd_rows_partial);
  m.impl("flash_bwd_rows_sum", &flash_bwd_rows_sum);
}
