// xdot — torch operator bindings for the gfx950 kernels (registered as torch.ops.xdot.*).
//
// The kernels themselves live in *.hip translation units that do not include any torch
// header (fast rebuilds); this file only validates arguments on the host, resolves the
// current HIP stream and calls the C-ABI launchers.  Every launch is bounds-checked on
// the host against the tensors' storage so a bad stride can never turn into a GPU fault.
// The flash-attention ops are implemented (and bound to their schemas below) in bindings_flash.cpp,
// the row-wise ops around them (rope_*, headnorm_*, sink_*, gate_*) in bindings_rowops.cpp,
// the GEMM ops (gemm, gemm_plan, proj, wgrad, wgrad2) in bindings_gemm.cpp.
#include "bindings_common.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

// sha256 of csrc/* + flags, compiled in by xdot/build.py (build/xdot/build_id.cpp)
extern "C" const char xdot_build_id[];

using namespace xdot::bind;

namespace {

std::string build_id() { return std::string(xdot_build_id + 14); }  // after "XDOT_BUILD_ID="

// ------------------------------------------------------------------------------------
at::Tensor softmax_fwd(const at::Tensor& x, const c10::optional<at::Tensor>& mask, double scale,
                       int64_t mdiv, int64_t mmul, int64_t mmod) {
  Range rr_("xdot.softmax_fwd");
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(), "xdot.softmax_fwd: x must be a contiguous GPU tensor");
  const int64_t T = x.size(-1);
  const int64_t rows = T == 0 ? 0 : x.numel() / T;
  auto y = at::empty_like(x);
  xdot::smx::Args a{};
  a.x = x.data_ptr(); a.out = y.data_ptr(); a.rows = rows; a.T = T; a.scale = (float)scale;
  a.mdiv = mdiv; a.mmul = mmul; a.mmod = mmod; a.mask = nullptr;
  bool vec = (T % 8 == 0) && aligned16(x.data_ptr()) && aligned16(y.data_ptr());
  if (mask.has_value() && mask->defined()) {
    const auto& m = *mask;
    TORCH_CHECK(m.is_cuda() && m.is_contiguous() && m.scalar_type() == at::kBool, "xdot.softmax_fwd: mask must be contiguous bool on GPU");
    TORCH_CHECK(m.size(-1) == T, "xdot.softmax_fwd: mask last dim mismatch");
    TORCH_CHECK(mdiv > 0 && mmod > 0, "xdot.softmax_fwd: bad mask row map");
    const int64_t mrows = m.numel() / T;
    // furthest mask row touched
    const int64_t lr = ((rows - 1) / mdiv) * mmul + std::min<int64_t>(rows - 1, mmod - 1);
    TORCH_CHECK(rows == 0 || lr < mrows, "xdot.softmax_fwd: mask row map out of bounds");
    a.mask = reinterpret_cast<const uint8_t*>(m.data_ptr());
    vec = vec && ((reinterpret_cast<uintptr_t>(m.data_ptr()) & 7) == 0);
  }
  TORCH_CHECK(rows <= 0x7fffffff, "xdot.softmax_fwd: too many rows");
  c10::DeviceGuard guard(x.device());
  launched(xdot_softmax_fwd_launch(&a, dt_code(x.scalar_type()), vec, cur_stream(x)), "softmax_fwd", "dtype");
  return y;
}

at::Tensor softmax_bwd(const at::Tensor& y, const at::Tensor& dy, double scale) {
  Range rr_("xdot.softmax_bwd");
  TORCH_CHECK(y.is_cuda() && y.is_contiguous() && dy.is_contiguous(), "xdot.softmax_bwd: contiguous GPU tensors required");
  TORCH_CHECK(y.sizes() == dy.sizes() && y.scalar_type() == dy.scalar_type(), "xdot.softmax_bwd: y/dy mismatch");
  const int64_t T = y.size(-1);
  const int64_t rows = T == 0 ? 0 : y.numel() / T;
  auto dx = at::empty_like(y);
  xdot::smx::Args a{};
  a.x = y.data_ptr(); a.dy = dy.data_ptr(); a.out = dx.data_ptr(); a.rows = rows; a.T = T;
  a.scale = (float)scale; a.mdiv = 1; a.mmul = 0; a.mmod = 1;
  const bool vec = (T % 8 == 0) && aligned16(y.data_ptr()) && aligned16(dy.data_ptr()) && aligned16(dx.data_ptr());
  c10::DeviceGuard guard(y.device());
  launched(xdot_softmax_bwd_launch(&a, dt_code(y.scalar_type()), vec, cur_stream(y)), "softmax_bwd", "dtype");
  return dx;
}

// ------------------------------------------------------------------------------------
std::tuple<at::Tensor, at::Tensor, at::Tensor> mask_pack(const at::Tensor& mask) {
  Range rr_("xdot.mask_pack");
  TORCH_CHECK(mask.is_cuda() && mask.scalar_type() == at::kBool && mask.dim() == 3, "xdot.mask_pack: (B, R, T) bool GPU mask");
  auto m = mask.contiguous();
  const int64_t B = m.size(0), R = m.size(1), T = m.size(2);
  const int64_t NKT = (T + 63) / 64, NRT = (R + 63) / 64, Tpad = (T + 127) / 128 * 128;
  auto bits = at::empty({B, NKT, R}, m.options().dtype(at::kLong));
  auto flags = at::empty({B, (R + 31) / 32, (NKT + 3) & ~3}, m.options().dtype(at::kByte));
  auto bitsT = at::empty({B, NRT, Tpad}, m.options().dtype(at::kLong));
  TORCH_CHECK(B * R * NKT < (1LL << 40) && T < (1LL << 31), "xdot.mask_pack: too large");
  c10::DeviceGuard guard(m.device());
  xdot_mask_pack_launch(reinterpret_cast<const uint8_t*>(m.data_ptr()), reinterpret_cast<uint64_t*>(bits.data_ptr()),
                        reinterpret_cast<uint64_t*>(bitsT.data_ptr()), flags.data_ptr<uint8_t>(), (int)B, (int)R, (int)T,
                        cur_stream(m));
  check_launch(hipGetLastError(), "mask_pack");
  return {bits, flags, bitsT};
}

// mask_pack's outputs for the mask `causal / window / lengths / doc_starts` describe
// (xdot.StructuredMask), the packed columns being the runs of `segs` (nseg, 3) int32 (packed_start,
// length, global_start); doc_starts: (n,) shared or (B, n) sorted int32 document starts; row_runs:
// (nrun, 3) int32 (local_start, length, global_start) tiling the R rows, in place of row_offset
std::tuple<at::Tensor, at::Tensor, at::Tensor> mask_gen(int64_t B, int64_t R, int64_t T, bool causal, int64_t window,
                                                        int64_t row_offset, const c10::optional<at::Tensor>& lengths,
                                                        const at::Tensor& segs,
                                                        const c10::optional<at::Tensor>& doc_starts,
                                                        const c10::optional<at::Tensor>& row_runs) {
  Range rr_("xdot.mask_gen");
  TORCH_CHECK(B >= 0 && R >= 0 && T >= 0, "xdot.mask_gen: negative shape");
  TORCH_CHECK(segs.is_cuda() && segs.scalar_type() == at::kInt && segs.dim() == 2 && segs.size(1) == 3 &&
                  segs.is_contiguous(),
              "xdot.mask_gen: segs must be a contiguous (nseg, 3) int32 GPU tensor");
  if (lengths.has_value())
    TORCH_CHECK(lengths->is_cuda() && lengths->device() == segs.device() && lengths->scalar_type() == at::kInt &&
                    lengths->dim() == 1 && lengths->size(0) == B && lengths->is_contiguous(),
                "xdot.mask_gen: lengths must be a contiguous (B,) int32 tensor on the segment table's device");
  const int* starts = nullptr;
  int64_t nstarts = 0, starts_stride = 0;
  if (doc_starts.has_value()) {
    const at::Tensor& d = *doc_starts;
    TORCH_CHECK(d.is_cuda() && d.device() == segs.device() && d.scalar_type() == at::kInt && d.is_contiguous() &&
                    (d.dim() == 1 || (d.dim() == 2 && d.size(0) == B)) && d.size(-1) < (1LL << 31),
                "xdot.mask_gen: doc_starts must be a contiguous (n,) or (B, n) int32 tensor on the segment table's device");
    nstarts = d.size(-1);
    starts_stride = d.dim() == 2 ? nstarts : 0;
    if (d.numel() > 0) starts = d.data_ptr<int>();
  }
  TORCH_CHECK(window >= 0 && window < (1LL << 40) && row_offset >= 0 && row_offset < (1LL << 40),
              "xdot.mask_gen: window / row_offset out of range");
  const int* rows = nullptr;
  int64_t nrows = 0;
  if (row_runs.has_value()) {
    const at::Tensor& t = *row_runs;
    TORCH_CHECK(t.is_cuda() && t.device() == segs.device() && t.scalar_type() == at::kInt && t.dim() == 2 &&
                    t.size(1) == 3 && t.is_contiguous() && t.size(0) < (1LL << 20),
                "xdot.mask_gen: row_runs must be a contiguous (nrun, 3) int32 tensor on the segment table's device");
    nrows = t.size(0);
    if (nrows > 0) rows = t.data_ptr<int>();
  }
  const int64_t NKT = (T + 63) / 64, NRT = (R + 63) / 64, Tpad = (T + 127) / 128 * 128;
  TORCH_CHECK(B * R * NKT < (1LL << 40) && T < (1LL << 31) && R < (1LL << 31) && B < (1LL << 31), "xdot.mask_gen: too large");
  auto bits = at::empty({B, NKT, R}, segs.options().dtype(at::kLong));
  auto flags = at::empty({B, (R + 31) / 32, (NKT + 3) & ~3}, segs.options().dtype(at::kByte));
  auto bitsT = at::empty({B, NRT, Tpad}, segs.options().dtype(at::kLong));
  c10::DeviceGuard guard(segs.device());
  xdot_mask_gen_launch(reinterpret_cast<uint64_t*>(bits.data_ptr()), reinterpret_cast<uint64_t*>(bitsT.data_ptr()),
                       flags.data_ptr<uint8_t>(), lengths.has_value() ? lengths->data_ptr<int>() : nullptr,
                       segs.data_ptr<int>(), (int)segs.size(0), causal ? 1 : 0, window, row_offset, (int)B, (int)R, (int)T,
                       starts, starts == nullptr ? 0 : (int)nstarts, starts_stride, rows, (int)nrows, cur_stream(segs));
  check_launch(hipGetLastError(), "mask_gen");
  return {bits, flags, bitsT};
}


// fused MSE loss forward: (mean (y - t)^2 in y's dtype, dy = 2 (y - t) / n)
std::tuple<at::Tensor, at::Tensor> mse_fwd(const at::Tensor& y, const at::Tensor& t) {
  Range rr_("xdot.mse_fwd");
  const auto st_ = y.scalar_type();
  TORCH_CHECK(y.is_cuda() && t.is_cuda() && y.is_contiguous() && t.is_contiguous() && t.scalar_type() == st_ &&
                  y.sizes() == t.sizes() && (st_ == at::kBFloat16 || st_ == at::kHalf || st_ == at::kFloat) &&
                  aligned16(y.data_ptr()) && aligned16(t.data_ptr()) && y.numel() % (16 / y.element_size()) == 0 &&
                  y.numel() > 0,
              "xdot.mse_fwd: same-shape contiguous 16-byte aligned bf16/fp16/fp32 device tensors, numel % (16 B) == 0");
  auto dy = at::empty_like(y);
  const int64_t nv = y.numel() / (16 / y.element_size());
  const int nparts = (int)std::min<int64_t>(1024, (nv + 255) / 256);
  auto part = at::empty({nparts}, y.options().dtype(at::kFloat));
  auto loss = at::empty({}, y.options());
  c10::DeviceGuard guard(y.device());
  launched(xdot_mse_fwd_launch(y.data_ptr(), t.data_ptr(), dy.data_ptr(), part.data_ptr<float>(), nparts, loss.data_ptr(),
                               y.numel(), dt_code(st_), cur_stream(y)),
           "mse_fwd", "launch rejected");
  return {loss, dy};
}

// dst[i] <- src[i] converted to dst[i]'s dtype (fp32 / bf16 / fp16), every pair in one launch per
// CAST_MAX_T pairs (GradSync: 16-bit gradients <-> the fp32 buffers its all-reduce sums)
void cast_multi(at::TensorList src, at::TensorList dst) {
  Range rr_("xdot.cast_multi");
  const size_t n = src.size();
  TORCH_CHECK(dst.size() == n, "xdot.cast_multi: list sizes");
  if (n == 0) return;
  for (size_t i = 0; i < n; ++i) {
    TORCH_CHECK(src[i].is_cuda() && dst[i].is_cuda() && src[i].device() == dst[0].device() &&
                    dst[i].device() == dst[0].device(),
                "xdot.cast_multi: GPU tensors on one device");
    TORCH_CHECK(src[i].is_contiguous() && dst[i].is_contiguous() && src[i].numel() == dst[i].numel(),
                "xdot.cast_multi: contiguous tensors of equal numel");
    TORCH_CHECK(dt_code(src[i].scalar_type()) >= 0 && dt_code(dst[i].scalar_type()) >= 0,
                "xdot.cast_multi: fp32 / bf16 / fp16 only");
  }
  c10::DeviceGuard guard(dst[0].device());
  for (size_t c0 = 0; c0 < n; c0 += xdot::CAST_MAX_T) {
    xdot::CastArgs a{};
    int blk = 0;
    a.nt = (int)std::min<size_t>(xdot::CAST_MAX_T, n - c0);
    for (int i = 0; i < a.nt; ++i) {
      const size_t k = c0 + i;
      a.src[i] = src[k].data_ptr();
      a.dst[i] = dst[k].data_ptr();
      a.n[i] = src[k].numel();
      a.sdt[i] = dt_code(src[k].scalar_type());
      a.ddt[i] = dt_code(dst[k].scalar_type());
      a.blk0[i] = blk;
      const int64_t nb = (a.n[i] + xdot::CAST_BLOCK_ELEMS - 1) / xdot::CAST_BLOCK_ELEMS;
      TORCH_CHECK(blk + nb < (1LL << 31), "xdot.cast_multi: too many elements");
      blk += (int)nb;
    }
    a.blk0[a.nt] = blk;
    launched(xdot_cast_multi_launch(&a, cur_stream(dst[0])), "cast_multi", "dtype");
  }
}

// one AdamW step for lists of same-dtype params / grads with fp32 moments (chunks of 32)
// grad_out (optional, one per parameter): the gradients are fp32 (GradSync's reduced sums of
// 16-bit parameters) and each is also written into grad_out[i] in the parameter dtype
void adamw_step(at::TensorList params, at::TensorList grads, at::TensorList exp_avg, at::TensorList exp_avg_sq,
                double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                at::TensorList step_ts, const c10::optional<at::Tensor>& lr_t, at::TensorList grad_out) {
  Range rr_("xdot.adamw_step");
  const size_t n = params.size();
  const bool dev_state = step_ts.size() > 0;
  if (dev_state) {
    TORCH_CHECK(step_ts.size() == n && lr_t.has_value() && lr_t->defined(),
                "xdot.adamw_step: device state needs one step tensor per parameter and lr_t");
    for (const auto& t : step_ts)
      TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.numel() == 1,
                  "xdot.adamw_step: step tensors must be one-element fp32 device tensors");
    TORCH_CHECK(lr_t->is_cuda() && lr_t->scalar_type() == at::kFloat && lr_t->numel() == 1,
                "xdot.adamw_step: lr_t must be a one-element fp32 device tensor");
  }
  TORCH_CHECK(grads.size() == n && exp_avg.size() == n && exp_avg_sq.size() == n, "xdot.adamw_step: list sizes");
  const bool g32 = grad_out.size() > 0;
  TORCH_CHECK(!g32 || grad_out.size() == n, "xdot.adamw_step: one grad_out per parameter");
  TORCH_CHECK(step >= 1, "xdot.adamw_step: step counts from 1");
  if (n == 0) return;
  const auto dtype = params[0].scalar_type();
  for (size_t i = 0; i < n; ++i) {
    TORCH_CHECK(params[i].is_cuda() && params[i].is_contiguous() && params[i].scalar_type() == dtype,
                "xdot.adamw_step: contiguous GPU params of one dtype");
    TORCH_CHECK(grads[i].sizes() == params[i].sizes() && grads[i].is_contiguous() &&
                    grads[i].scalar_type() == (g32 ? at::kFloat : dtype),
                "xdot.adamw_step: grad shape/dtype");
    if (g32)
      TORCH_CHECK(dtype != at::kFloat && grad_out[i].sizes() == params[i].sizes() && grad_out[i].is_contiguous() &&
                      grad_out[i].scalar_type() == dtype && grad_out[i].device() == params[i].device(),
                  "xdot.adamw_step: grad_out (16-bit parameters, parameter shape / dtype)");
    for (const at::Tensor* s : {&exp_avg[i], &exp_avg_sq[i]})
      TORCH_CHECK(s->numel() == params[i].numel() && s->is_contiguous() && s->scalar_type() == at::kFloat,
                  "xdot.adamw_step: fp32 moments");
  }
  const float bc1 = 1.f - (float)std::pow(beta1, (double)step);
  const float bc2 = 1.f - (float)std::pow(beta2, (double)step);
  c10::DeviceGuard guard(params[0].device());
  for (size_t c0 = 0; c0 < n; c0 += xdot::ADAM_MAX_T) {
    xdot::AdamArgs a{};
    int blk = 0;
    a.nt = (int)std::min<size_t>(xdot::ADAM_MAX_T, n - c0);
    for (int i = 0; i < a.nt; ++i) {
      const size_t k = c0 + i;
      a.p[i] = params[k].data_ptr(); a.g[i] = grads[k].data_ptr();
      a.m[i] = exp_avg[k].data_ptr<float>(); a.v[i] = exp_avg_sq[k].data_ptr<float>();
      a.n[i] = params[k].numel();
      a.step_dev[i] = dev_state ? step_ts[k].data_ptr<float>() : nullptr;
      a.gout[i] = g32 ? grad_out[k].data_ptr() : nullptr;
      a.blk0[i] = blk;
      const int64_t nb = (a.n[i] + xdot::ADAM_BLOCK_ELEMS - 1) / xdot::ADAM_BLOCK_ELEMS;
      TORCH_CHECK(blk + nb < (1LL << 31), "xdot.adamw_step: too many elements");
      blk += (int)nb;
    }
    a.blk0[a.nt] = blk;
    a.lr = (float)lr; a.beta1 = (float)beta1; a.beta2 = (float)beta2; a.eps = (float)eps; a.wd = (float)weight_decay;
    a.bc1 = bc1; a.bc2_sqrt = std::sqrt(bc2);
    a.dev_state = dev_state ? 1 : 0;
    a.lr_dev = dev_state ? lr_t->data_ptr<float>() : nullptr;
    a.g32 = g32 ? 1 : 0;
    launched(xdot_adamw_launch(&a, dt_code(dtype), cur_stream(params[0])), "adamw_step", "dtype");
  }
}

// ---- native xGMI pull collectives (csrc/ipc.hip; driven by xdot/utils/ipc.py) ----
void ipc_ok(int rc, const char* what) { TORCH_CHECK(rc == 0, "xdot.", what, ": HIP error ", rc); }

std::vector<int64_t> ipc_info() {
  return {xdot_ipc_sig_bytes(), xdot_ipc_max_ranks(), xdot_ipc_max_wgs(), xdot_ipc_handle_bytes(),
          xdot_ipc_wall_clock_khz()};
}
int64_t ipc_alloc(int64_t nbytes, bool uncached) {
  TORCH_CHECK(nbytes > 0, "xdot.ipc_alloc: size");
  void* p = nullptr;
  ipc_ok(xdot_ipc_alloc(nbytes, uncached ? 1 : 0, &p), "ipc_alloc");
  return (int64_t)(uintptr_t)p;
}
void ipc_free(int64_t p) { ipc_ok(xdot_ipc_free((void*)(uintptr_t)p), "ipc_free"); }
at::Tensor ipc_get_handle(int64_t p) {
  auto h = at::empty({xdot_ipc_handle_bytes()}, at::TensorOptions().dtype(at::kByte));
  ipc_ok(xdot_ipc_get_handle((void*)(uintptr_t)p, h.data_ptr()), "ipc_get_handle");
  return h;
}
int64_t ipc_open(const at::Tensor& h) {
  TORCH_CHECK(!h.is_cuda() && h.scalar_type() == at::kByte && h.is_contiguous() && h.numel() == xdot_ipc_handle_bytes(),
              "xdot.ipc_open: a CPU uint8 handle tensor");
  void* p = nullptr;
  ipc_ok(xdot_ipc_open(h.data_ptr(), &p), "ipc_open");
  return (int64_t)(uintptr_t)p;
}
void ipc_close(int64_t p) { ipc_ok(xdot_ipc_close((void*)(uintptr_t)p), "ipc_close"); }
std::vector<int64_t> ipc_host_word() {
  void *host = nullptr, *dev = nullptr;
  ipc_ok(xdot_ipc_host_word(&host, &dev), "ipc_host_word");
  return {(int64_t)(uintptr_t)host, (int64_t)(uintptr_t)dev};
}
int64_t ipc_read_word(int64_t host) { return (int64_t)*reinterpret_cast<volatile uint32_t*>((uintptr_t)host); }
void ipc_write_word(int64_t host, int64_t v) { *reinterpret_cast<volatile uint32_t*>((uintptr_t)host) = (uint32_t)v; }

xdot::ipc::Args ipc_args(const at::Tensor& inp, at::Tensor& out, at::IntArrayRef stage, at::IntArrayRef sig,
                         int64_t status, int64_t rank, int64_t epoch, int64_t ticks, int64_t nwg, const char* what) {
  const int64_t n = (int64_t)stage.size();
  TORCH_CHECK(n >= 2 && n <= xdot::ipc::MAXR && (int64_t)sig.size() == n && rank >= 0 && rank < n, "xdot.", what,
              ": ranks");
  TORCH_CHECK(nwg >= 1 && nwg <= xdot::ipc::MAXG && epoch >= 1 && status != 0, "xdot.", what, ": config");
  TORCH_CHECK(inp.is_cuda() && out.is_cuda() && inp.is_contiguous() && out.is_contiguous() &&
              inp.device() == out.device() && inp.element_size() >= 2 &&
              (uintptr_t)inp.data_ptr() % 2 == 0 && (uintptr_t)out.data_ptr() % 2 == 0,
              "xdot.", what, ": contiguous 16/32-bit device tensors");
  xdot::ipc::Args a{};
  a.src = static_cast<const char*>(inp.data_ptr());
  a.out = static_cast<char*>(out.data_ptr());
  for (int64_t p = 0; p < n; ++p) {
    TORCH_CHECK(stage[p] != 0 && sig[p] != 0 && stage[p] % 16 == 0, "xdot.", what, ": peer pointers");
    a.stage[p] = reinterpret_cast<char*>((uintptr_t)stage[p]);
    a.sig[p] = reinterpret_cast<uint32_t*>((uintptr_t)sig[p]);
  }
  a.status = reinterpret_cast<uint32_t*>((uintptr_t)status);
  a.timeout_ticks = ticks;
  a.rank = (int)rank; a.n = (int)n; a.epoch = (int)epoch; a.nwg = (int)nwg;
  return a;
}

// out (N * inp bytes, rank-major) <- every rank's inp, pulled over xGMI from the peers' staging slots
void ipc_all_gather(const at::Tensor& inp, at::Tensor& out, at::IntArrayRef stage, at::IntArrayRef sig, int64_t status,
                    int64_t rank, int64_t epoch, int64_t ticks, int64_t nwg) {
  Range rr_("xdot.ipc_all_gather");
  auto a = ipc_args(inp, out, stage, sig, status, rank, epoch, ticks, nwg, "ipc_all_gather");
  const int64_t bytes = inp.numel() * inp.element_size();
  TORCH_CHECK(out.numel() * out.element_size() == bytes * a.n && bytes % 16 == 0, "xdot.ipc_all_gather: sizes");
  a.shard = bytes;
  c10::DeviceGuard guard(inp.device());
  launched(xdot_ipc_all_gather_launch(&a, cur_stream(inp)), "ipc_all_gather");
}

// out <- Σ over ranks (rank order, fp32) of block `rank` of the rank-major inp
void ipc_reduce_scatter(const at::Tensor& inp, at::Tensor& out, at::IntArrayRef stage, at::IntArrayRef sig,
                        int64_t status, int64_t rank, int64_t epoch, int64_t ticks, int64_t nwg) {
  Range rr_("xdot.ipc_reduce_scatter");
  auto a = ipc_args(inp, out, stage, sig, status, rank, epoch, ticks, nwg, "ipc_reduce_scatter");
  TORCH_CHECK(inp.scalar_type() == out.scalar_type(), "xdot.ipc_reduce_scatter: dtype");
  const int64_t bytes = out.numel() * out.element_size();
  TORCH_CHECK(inp.numel() == out.numel() * a.n && bytes % 16 == 0, "xdot.ipc_reduce_scatter: sizes");
  a.shard = bytes;
  a.dt = dt_code(inp.scalar_type());
  c10::DeviceGuard guard(inp.device());
  launched(xdot_ipc_reduce_scatter_launch(&a, cur_stream(inp)), "ipc_reduce_scatter");
}

// ---- HIP graph node priorities: diagnostics (benchmarks/micro/graph_prio_probe.py) ----
// Stream capture records the fork/join topology but not the stream priorities, and on ROCm 7.2
// hipGraphKernelNodeSetAttribute(.., hipKernelNodeAttributePriority, ..) returns invalid
// argument, so a captured two-stream backward cannot get its priority back
// (profiles/r3_graph.md); these two ops let the probe re-check a newer runtime.
void graph_ok(hipError_t e, const char* what) {
  if (e != hipSuccess) (void)hipGetLastError();  // do not leave the error for the next HIP call
  TORCH_CHECK(e == hipSuccess, "xdot.", what, ": ", hipGetErrorString(e));
}

bool is_kernel_node(hipGraphNode_t n) {
  hipGraphNodeType t;
  return hipGraphNodeGetType(n, &t) == hipSuccess && t == hipGraphNodeTypeKernel;
}

// priorities of every kernel node of a graph (diagnostics / tests)
std::vector<int64_t> graph_kernel_priorities(int64_t raw) {
  hipGraph_t g = reinterpret_cast<hipGraph_t>((uintptr_t)raw);
  size_t n = 0;
  graph_ok(hipGraphGetNodes(g, nullptr, &n), "graph_kernel_priorities");
  std::vector<hipGraphNode_t> nodes(n);
  graph_ok(hipGraphGetNodes(g, nodes.data(), &n), "graph_kernel_priorities");
  std::vector<int64_t> out;
  for (auto nd : nodes) {
    if (!is_kernel_node(nd)) continue;
    hipKernelNodeAttrValue v{};
    graph_ok(hipGraphKernelNodeGetAttribute(nd, hipKernelNodeAttributePriority, &v), "graph_kernel_priorities");
    out.push_back(v.priority);
  }
  return out;
}

// set the priority attribute of the i-th kernel node of a graph (diagnostics)
void graph_set_kernel_priority(int64_t raw, int64_t index, int64_t prio) {
  hipGraph_t g = reinterpret_cast<hipGraph_t>((uintptr_t)raw);
  size_t n = 0;
  graph_ok(hipGraphGetNodes(g, nullptr, &n), "graph_set_kernel_priority");
  std::vector<hipGraphNode_t> nodes(n);
  graph_ok(hipGraphGetNodes(g, nodes.data(), &n), "graph_set_kernel_priority");
  int64_t k = 0;
  for (auto nd : nodes) {
    if (!is_kernel_node(nd)) continue;
    if (k++ != index) continue;
    hipKernelNodeAttrValue v{};
    v.priority = (int)prio;
    graph_ok(hipGraphKernelNodeSetAttribute(nd, hipKernelNodeAttributePriority, &v), "graph_set_kernel_priority");
    return;
  }
  TORCH_CHECK(false, "xdot.graph_set_kernel_priority: no kernel node ", index);
}

}  // namespace

TORCH_LIBRARY(xdot, m) {
  m.def("gemm(Tensor A, Tensor B, Tensor(a!) C, int M, int N, int K, int nseg, int nb1, int nb2, "
        "int lda, int ldb, int ldc, int sA1, int sA2, int sB1, int sB2, int sC1, int sC2, "
        "int sAseg, int sBseg, bool a_mc, bool b_mc, float alpha, float beta=0.0, int path=0) -> ()");
  m.def("gemm_plan(int M, int N, int K, int nseg, int nb1, int nb2, int lda, int ldb, int ldc, int sA1, int sA2, "
        "int sB1, int sB2, int sC1, int sC2, int sAseg, int sBseg, bool a_mc, bool b_mc, float beta, ScalarType dt_in, "
        "ScalarType dt_out, bool a16, bool b16, bool c16, int path) -> int[]");
  m.def("softmax_fwd(Tensor x, Tensor? mask, float scale, int mdiv, int mmul, int mmod) -> Tensor");
  m.def("softmax_bwd(Tensor y, Tensor dy, float scale) -> Tensor");
  m.def("mask_pack(Tensor mask) -> (Tensor, Tensor, Tensor)");
  m.def("mask_gen(int B, int R, int T, bool causal, int window, int row_offset, Tensor? lengths, Tensor segs, Tensor? doc_starts=None, Tensor? row_runs=None) -> (Tensor, Tensor, Tensor)");
  m.def("flash_fwd(Tensor rows, Tensor kc, Tensor vc, Tensor? bits, Tensor? flags, int H, float scale, int nsplit=0, bool prescaled=False, int fp32_mode=0, Tensor(a!)? sbuf=None, int Hg=0) -> (Tensor, Tensor)");
  m.def("flash_bwd_cols(Tensor dout, Tensor rows, Tensor kc, Tensor vc, Tensor out, Tensor lse, Tensor? bits, "
        "Tensor? flags, int H, float scale, Tensor? delta=None, bool fp32_out=True, bool prescaled=False, "
        "Tensor? lse2=None, int fp32_mode=0, Tensor(a!)? sbuf=None, Tensor(b!)? dsbuf=None, int passes=3, "
        "Tensor(c!)? dkv_out=None, int Hg=0) -> (Tensor, Tensor)");
  m.def("flash_bwd_prep(Tensor dout, Tensor out, Tensor lse, int H) -> (Tensor, Tensor)");
  m.def("flash_bwd_delta(Tensor dout, Tensor out, int H) -> Tensor");
  m.def("sum_partials(Tensor part, ScalarType out_dtype) -> Tensor");
  m.def("flash_splits(int B, int R, int T, int H, bool rows_kernel) -> int");
  m.def("flash_fwd_plan(int B, int R, int T, int H, int D, ScalarType dtype, int fp32_mode, bool sbuf, int nsplit) -> int[]");
  m.def("flash_rows_plan(int B, int R, int T, int H, int D, ScalarType dtype, int fp32_mode, bool prescaled, int nsplit) -> int[]");
  m.def("flash_cols_plan(int B, int R, int T, int H, int D, ScalarType dtype, int fp32_mode, bool sbuf, bool dsbuf, "
        "int passes, bool prescaled, bool fp32_out, int Hg=0) -> int[]");
  m.def("flash_fwd_partial(Tensor rows, Tensor kc, Tensor vc, Tensor? bits, Tensor? flags, int H, float scale, "
        "Tensor(a!) opart, Tensor(b!) lpart, int sp0, int nsplit, bool prescaled=False, int fp32_mode=0, int Hg=0) -> ()");
  m.def("flash_fwd_combine(Tensor opart, Tensor lpart, int H, Tensor like) -> (Tensor, Tensor)");
  m.def("flash_bwd_rows_partial(Tensor dout, Tensor rows, Tensor kc, Tensor vc, Tensor lse, Tensor delta, Tensor? bits, "
        "Tensor? flags, int H, float scale, Tensor(a!) dpart, int sp0, int nsplit, bool prescaled=False, int fp32_mode=0, int Hg=0) -> ()");
  m.def("flash_bwd_rows_sum(Tensor dpart, int H, Tensor like) -> Tensor");
  m.def("flash_fwd_merge(Tensor(a!) opart, Tensor lpart, Tensor(b!) lrun, int H) -> ()");
  m.def("sum_partials_into(Tensor part, Tensor(a!) out) -> ()");
  m.def("cast_multi(Tensor[] src, Tensor(a!)[] dst) -> ()");
  m.def("adamw_step(Tensor(a!)[] params, Tensor[] grads, Tensor(b!)[] exp_avg, Tensor(c!)[] exp_avg_sq, float lr, "
        "float beta1, float beta2, float eps, float weight_decay, int step, Tensor[] step_ts, Tensor? lr_t, "
        "Tensor(d!)[] grad_out) -> ()");
  m.def("flash_bwd_rows(Tensor dout, Tensor rows, Tensor kc, Tensor vc, Tensor lse, Tensor delta, Tensor? bits, "
        "Tensor? flags, int H, float scale, int nsplit=0, bool prescaled=False, int fp32_mode=0, Tensor? sbuf=None, "
        "Tensor? dsbuf=None, int Hg=0) -> Tensor");
  m.def("flash_prescale(Tensor x, float scale) -> Tensor");
  m.def("rope_table(int R, int D, int offset, Tensor inv_freq) -> (Tensor, Tensor)");
  m.def("rope_apply(Tensor x, Tensor cos, Tensor sin, int H, bool inverse, float alpha, Tensor(a!) out) -> ()");
  m.def("headnorm_plan(int B, int R, int H, int D, ScalarType dtype) -> int[]");
  m.def("headnorm_fwd(Tensor x, Tensor weight, Tensor? cos, Tensor? sin, int H, float eps, float alpha, Tensor(a!) out, "
        "bool save) -> (Tensor, Tensor)");
  m.def("headnorm_bwd(Tensor g, Tensor x, Tensor rstd, Tensor weight, Tensor? cos, Tensor? sin, int H, float alpha, "
        "Tensor(a!) dx, bool need_dw) -> Tensor");
  m.def("sink_fold(Tensor(a!) out, Tensor(b!) lse, Tensor sinks, int H) -> ()");
  m.def("sink_grad(Tensor delta, Tensor lse, Tensor sinks) -> Tensor");
  m.def("gate_apply(Tensor o, Tensor g, int H, Tensor(a!) out, int mode=-1) -> ()");
  m.def("gate_backward(Tensor dy, Tensor o, Tensor g, int H, Tensor(a!) dout, int mode=-1) -> Tensor");
  m.def("mse_fwd(Tensor y, Tensor t) -> (Tensor, Tensor)");
  m.def("proj(Tensor x, Tensor w, Tensor? bias, bool nn, Tensor(a!)? out=None, int force=0, float alpha=1.0) -> Tensor");
  m.def("wgrad(Tensor dy, Tensor x, ScalarType out_dtype, int splits=0) -> Tensor");
  m.def("wgrad2(Tensor dy0, Tensor x0, Tensor dy1, Tensor x1, ScalarType out_dtype) -> Tensor[]");
  m.def("ipc_info() -> int[]");
  m.def("ipc_alloc(int nbytes, bool uncached) -> int");
  m.def("ipc_free(int ptr) -> ()");
  m.def("ipc_get_handle(int ptr) -> Tensor");
  m.def("ipc_open(Tensor handle) -> int");
  m.def("ipc_close(int ptr) -> ()");
  m.def("ipc_host_word() -> int[]");
  m.def("ipc_read_word(int host) -> int");
  m.def("ipc_write_word(int host, int v) -> ()");
  m.def("ipc_all_gather(Tensor inp, Tensor(a!) out, int[] stage, int[] sig, int status, int rank, int epoch, "
        "int ticks, int nwg) -> ()");
  m.def("ipc_reduce_scatter(Tensor inp, Tensor(a!) out, int[] stage, int[] sig, int status, int rank, int epoch, "
        "int ticks, int nwg) -> ()");
  m.def("build_id() -> str");
  m.def("graph_kernel_priorities(int graph) -> int[]");
  m.def("graph_set_kernel_priority(int graph, int index, int prio) -> ()");
}

TORCH_LIBRARY_IMPL(xdot, CompositeExplicitAutograd, m) {
  m.impl("build_id", &build_id);
  m.impl("graph_kernel_priorities", &graph_kernel_priorities);
  m.impl("graph_set_kernel_priority", &graph_set_kernel_priority);
  m.impl("ipc_info", &ipc_info);
  m.impl("ipc_alloc", &ipc_alloc);
  m.impl("ipc_free", &ipc_free);
  m.impl("ipc_get_handle", &ipc_get_handle);
  m.impl("ipc_open", &ipc_open);
  m.impl("ipc_close", &ipc_close);
  m.impl("ipc_host_word", &ipc_host_word);
  m.impl("ipc_read_word", &ipc_read_word);
  m.impl("ipc_write_word", &ipc_write_word);
}

TORCH_LIBRARY_IMPL(xdot, CUDA, m) {
  m.impl("softmax_fwd", &softmax_fwd);
  m.impl("softmax_bwd", &softmax_bwd);
  m.impl("mask_pack", &mask_pack);
  m.impl("mask_gen", &mask_gen);
  m.impl("mse_fwd", &mse_fwd);
  m.impl("adamw_step", &adamw_step);
  m.impl("cast_multi", &cast_multi);
  m.impl("ipc_all_gather", &ipc_all_gather);
  m.impl("ipc_reduce_scatter", &ipc_reduce_scatter);
}
