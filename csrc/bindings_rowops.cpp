// xdot — torch bindings of the row-wise ops around the attention (schemas: TORCH_LIBRARY in bindings.cpp):
// the rotation (rope.hip), the per-head RMSNorm (headnorm.hip), the attention sinks (sink.hip) and the
// output gate (gate.hip).
//
// Their (B, R, H*D) operands are strided row views -- the q half of a packed [q | v] buffer, a rank slot
// of the gather buffer -- all checked by the one rule of row_view.h (row_view in bindings_common.h); what
// differs per op is stated at the call: whether a view is written, and what an output may share with an input.
#include "bindings_common.h"

#include <vector>

namespace {

using namespace xdot::bind;
using xdot::RowView;
using OptT = c10::optional<at::Tensor>;

void kernel_dtype(const at::Tensor& x, const char* op) {
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kHalf || x.scalar_type() == at::kFloat,
              "xdot.", op, ": bf16/fp16/fp32 only");
}

// `dst` is written while `src` is read by the same lanes: the same view (in place) or disjoint memory
void in_place_or_apart(const RowView& src, const RowView& dst, const char* op) {
  TORCH_CHECK(src.lo != dst.lo || same_view(src, dst), "xdot.", op, ": an in-place output must be the same view as its input");
  TORCH_CHECK(src.lo == dst.lo || disjoint(src, dst), "xdot.", op, ": input and output overlap");
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

// out = alpha * rotate(x): x, out (B, R, H*D) row views; out may be x itself
void rope_apply(const at::Tensor& x, const at::Tensor& cosb, const at::Tensor& sinb, int64_t H, bool inverse,
                double alpha, at::Tensor& out) {
  Range rr_("xdot.rope_apply");
  TORCH_CHECK(x.is_cuda() && x.dim() == 3, "xdot.rope_apply: x must be a (B, R, H*D) GPU tensor");
  kernel_dtype(x, "rope_apply");
  const int64_t B = x.size(0), R = x.size(1), C = x.size(2);
  TORCH_CHECK(H > 0 && C % H == 0 && (C / H) % 2 == 0, "xdot.rope_apply: H*D with an even head dim D, got C=", C, " H=", H);
  TORCH_CHECK(B < (1LL << 31) && R < (1LL << 31) && C < (1LL << 31) && B * H < (1LL << 31), "xdot.rope_apply: too large");
  const int64_t D = C / H;
  TORCH_CHECK(rot_table(cosb, sinb, R, D, x.device(), "rope_apply"), "xdot.rope_apply: cos and sin are required");
  // (written = false: an out whose rows overlap is not refused)
  const RowView vx = row_view(x, B, R, C, x, false, "rope_apply", "x");
  const RowView vo = row_view(out, B, R, C, x, false, "rope_apply", "out");
  if (x.numel() == 0) return;
  in_place_or_apart(vx, vo, "rope_apply");  // a lane reads only the pairs it writes
  xdot::RopeArgs a{};
  a.x = x.data_ptr(); a.out = out.data_ptr();
  a.cos = cosb.data_ptr<float>(); a.sin = sinb.data_ptr<float>();
  a.B = (int)B; a.R = (int)R; a.H = (int)H; a.D = (int)D;
  a.xs_b = vx.sb; a.xs_r = vx.sr; a.os_b = vo.sb; a.os_r = vo.sr;
  a.alpha = (float)alpha; a.inverse = inverse ? 1 : 0;
  const bool vec = vx.vec && vo.vec && aligned16(cosb.data_ptr()) && aligned16(sinb.data_ptr());
  const int64_t V = 16 / (int64_t)x.element_size(), half = D / 2;
  const int mode = !vec ? 0 : (half % V == 0 ? 1 : (half > V ? 2 : 0));
  c10::DeviceGuard guard(x.device());
  launched(xdot_rope_apply_launch(&a, dt_code(x.scalar_type()), mode, cur_stream(x)), "rope_apply", "shape");
}

// ---- per-head RMSNorm fused with the rotation (csrc/headnorm.hip) ----
// (B, R, C) of x with C = H*D, D returned in *D; weight (D,) in x's dtype or fp32; the table, if any
bool hn_params(const at::Tensor& x, const at::Tensor& weight, const OptT& cosb, const OptT& sinb, int64_t H, int64_t* D,
               const char* op) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 3, "xdot.", op, ": the first operand must be a (B, R, H*D) GPU tensor");
  const int64_t C = x.size(2);
  TORCH_CHECK(H > 0 && C > 0 && C % H == 0, "xdot.", op, ": H*D features, got C=", C, " H=", H);
  *D = C / H;
  kernel_dtype(x, op);
  TORCH_CHECK(weight.is_cuda() && weight.device() == x.device() && weight.dim() == 1 && weight.size(0) == *D &&
                  weight.is_contiguous() &&
                  (weight.scalar_type() == x.scalar_type() || weight.scalar_type() == at::kFloat),
              "xdot.", op, ": weight must be a contiguous (D,) = (", *D, ",) tensor of x's dtype or fp32");
  return rot_table(cosb, sinb, x.size(1), *D, x.device(), op);
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
  int64_t D = 0;
  const bool rot = hn_params(x, weight, cosb, sinb, H, &D, "headnorm_fwd");
  TORCH_CHECK(eps > 0.0, "xdot.headnorm_fwd: eps must be positive");
  const int64_t B = x.size(0), R = x.size(1), C = x.size(2);
  // (written = false: an out whose rows overlap is not refused)
  const RowView vx = row_view(x, B, R, C, x, false, "headnorm_fwd", "x");
  const RowView vo = row_view(out, B, R, C, x, false, "headnorm_fwd", "out");
  auto rstd = at::empty({B, R, H}, x.options().dtype(at::kFloat));
  auto saved = save ? at::empty({B, R, C}, x.options()) : at::empty({0}, x.options());
  if (x.numel() == 0) return {rstd, saved};
  in_place_or_apart(vx, vo, "headnorm_fwd");
  hn_plan(B, R, H, D, (int64_t)x.element_size(), "headnorm_fwd");
  xdot::HeadNormArgs a{};
  a.x = x.data_ptr(); a.out = out.data_ptr(); a.save = save ? saved.data_ptr() : nullptr;
  a.rstd = rstd.data_ptr<float>(); a.w = weight.data_ptr(); a.w_f32 = weight.scalar_type() == at::kFloat;
  a.cos = rot ? cosb->data_ptr<float>() : nullptr; a.sin = rot ? sinb->data_ptr<float>() : nullptr;
  a.B = (int)B; a.R = (int)R; a.H = (int)H; a.D = (int)D;
  a.xs_b = vx.sb; a.xs_r = vx.sr; a.os_b = vo.sb; a.os_r = vo.sr;
  a.alpha = (float)alpha; a.eps = (float)eps; a.inv_d = 1.0f / (float)D;
  c10::DeviceGuard guard(x.device());
  launched(xdot_headnorm_fwd_launch(&a, dt_code(x.scalar_type()), vx.vec && vo.vec ? 1 : 0, cur_stream(x)), "headnorm_fwd",
           "shape");
  return {rstd, saved};
}

// dx = rstd * (gw - xh * mean(gw . xh)) with gy = alpha * rotate^-1(g), xh = x * rstd, gw = gy * weight,
// written to dx (may be g itself); returns dw = sum gy . xh in weight's dtype (need_dw), else empty.
// Two launches: the pass, which leaves one fp32 (D,) partial per workgroup, and their ordered sum
at::Tensor headnorm_bwd(const at::Tensor& g, const at::Tensor& x, const at::Tensor& rstd, const at::Tensor& weight,
                        const OptT& cosb, const OptT& sinb, int64_t H, double alpha, at::Tensor& dx, bool need_dw) {
  Range rr_("xdot.headnorm_bwd");
  int64_t D = 0;
  const bool rot = hn_params(g, weight, cosb, sinb, H, &D, "headnorm_bwd");
  const int64_t B = g.size(0), R = g.size(1), C = g.size(2);
  // (written = false: a dx whose rows overlap is not refused)
  const RowView vg = row_view(g, B, R, C, g, false, "headnorm_bwd", "g");
  const RowView vx = row_view(x, B, R, C, g, false, "headnorm_bwd", "x");
  const RowView vd = row_view(dx, B, R, C, g, false, "headnorm_bwd", "dx");
  TORCH_CHECK(rstd.is_cuda() && rstd.device() == g.device() && rstd.scalar_type() == at::kFloat && rstd.is_contiguous() &&
                  rstd.dim() == 3 && rstd.size(0) == B && rstd.size(1) == R && rstd.size(2) == H,
              "xdot.headnorm_bwd: rstd must be contiguous fp32 (B, R, H)");
  auto dw = need_dw ? at::empty({D}, weight.options()) : at::empty({0}, weight.options());
  if (g.numel() == 0) {
    if (need_dw) dw.zero_();
    return dw;
  }
  in_place_or_apart(vg, vd, "headnorm_bwd");
  TORCH_CHECK(disjoint(vx, vd), "xdot.headnorm_bwd: dx may overwrite g, not x");
  const auto p = hn_plan(B, R, H, D, (int64_t)g.element_size(), "headnorm_bwd");
  const int64_t nparts = (int64_t)p.bwd_gx * p.bwd_gy;
  auto part = at::empty({nparts, D}, g.options().dtype(at::kFloat));
  xdot::HeadNormArgs a{};
  a.x = x.data_ptr(); a.g = g.data_ptr(); a.out = dx.data_ptr(); a.rstd = rstd.data_ptr<float>();
  a.w = weight.data_ptr(); a.w_f32 = weight.scalar_type() == at::kFloat; a.part = part.data_ptr<float>();
  a.cos = rot ? cosb->data_ptr<float>() : nullptr; a.sin = rot ? sinb->data_ptr<float>() : nullptr;
  a.B = (int)B; a.R = (int)R; a.H = (int)H; a.D = (int)D;
  a.gs_b = vg.sb; a.gs_r = vg.sr; a.xs_b = vx.sb; a.xs_r = vx.sr; a.os_b = vd.sb; a.os_r = vd.sr;
  a.alpha = (float)alpha; a.inv_d = 1.0f / (float)D;
  c10::DeviceGuard guard(g.device());
  launched(xdot_headnorm_bwd_launch(&a, dt_code(g.scalar_type()), vg.vec && vx.vec && vd.vec ? 1 : 0, cur_stream(g)),
           "headnorm_bwd", "shape");
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
// out' = sigmoid(lse - s_h) * out.  out: a (B, R, H*D) row view with 16-byte aligned rows, lse: contiguous
// fp32 (B, H, R)
void sink_fold(at::Tensor& out, at::Tensor& lse, const at::Tensor& sinks, int64_t H) {
  Range rr_("xdot.sink_fold");
  TORCH_CHECK(out.is_cuda() && out.dim() == 3, "xdot.sink_fold: out must be a (B, R, H*D) GPU tensor");
  kernel_dtype(out, "sink_fold");
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
  const RowView v = row_view(out, B, R, C, out, true, "sink_fold", "out");
  if (out.numel() == 0) return;
  TORCH_CHECK(v.vec, "xdot.sink_fold: out and its row / batch strides must be 16-byte aligned");
  xdot::SinkArgs a{};
  a.out = out.data_ptr(); a.lse = lse.data_ptr<float>(); a.sinks = sinks.data_ptr();
  a.s_dt = dt_code(sinks.scalar_type());
  a.B = (int)B; a.R = (int)R; a.H = (int)H; a.D = (int)D;
  a.os_b = v.sb; a.os_r = v.sr;
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
  kernel_dtype(o, op);
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
  const RowView vo = row_view(o, B, R, C, o, false, "gate_apply", "o");
  const RowView vg = row_view(g, B, R, hw ? H : C, o, false, "gate_apply", "g");
  const RowView vy = row_view(out, B, R, C, o, true, "gate_apply", "out");
  if (o.numel() == 0) return;
  TORCH_CHECK(disjoint(vy, vo) && disjoint(vy, vg), "xdot.gate_apply: out may not share memory with o or g (out of place)");
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
  const RowView vo = row_view(o, B, R, C, o, false, "gate_backward", "o");
  const RowView vg = row_view(g, B, R, hw ? H : C, o, false, "gate_backward", "g");
  const RowView vd = row_view(dy, B, R, C, o, false, "gate_backward", "dy");
  const RowView vy = row_view(dout, B, R, C, o, true, "gate_backward", "dout");
  auto dg = at::empty({B, R, hw ? H : C}, o.options());
  if (o.numel() == 0) return dg;
  TORCH_CHECK(disjoint(vy, vo) && disjoint(vy, vg), "xdot.gate_backward: dout may not share memory with o or g");
  // (every element of do is written by the lane that read that element of dy: dy itself, or apart)
  TORCH_CHECK(same_view(vy, vd) || disjoint(vy, vd),
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

}  // namespace

TORCH_LIBRARY_IMPL(xdot, CompositeExplicitAutograd, m) { m.impl("headnorm_plan", &headnorm_plan); }

TORCH_LIBRARY_IMPL(xdot, CUDA, m) {
  m.impl("rope_table", &rope_table);
  m.impl("rope_apply", &rope_apply);
  m.impl("headnorm_fwd", &headnorm_fwd);
  m.impl("headnorm_bwd", &headnorm_bwd);
  m.impl("sink_fold", &sink_fold);
  m.impl("sink_grad", &sink_grad);
  m.impl("gate_apply", &gate_apply);
  m.impl("gate_backward", &gate_backward);
}
