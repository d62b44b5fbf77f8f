// xdot — torch bindings of the GEMM kernels (schemas: TORCH_LIBRARY in bindings.cpp).
// xdot.gemm describes its call as a GemmProblem, asks the host-only planner (gemm_plan.h) for the
// route and executes it; xdot.gemm_plan returns that plan without launching.  Every launch is
// bounds-checked on the host against the tensors' storage first.
#include "bindings_common.h"
#include "gemm_plan.h"

#include <algorithm>
#include <vector>

namespace {

using namespace xdot::bind;
namespace gp = xdot::gp;

static_assert((int)gp::F32 == (int)xdot::DT_F32 && (int)gp::BF16 == (int)xdot::DT_BF16 && (int)gp::F16 == (int)xdot::DT_F16,
              "gemm_plan.h's dtype codes are those of kernels.h");

// XDOT_GEMM_LIB: which plain large products may take the library GEMM (at::baddbmm ->
// hipBLASLt) on in-place strided views.  Default (unset / 0) = none: 16-bit products run gemm3
// (matches or beats the library), exact-fp32 products the xdot fp32 kernels.  "fp32" = exact-fp32
// plain products on the library (kept for A/B); 1 = 16-bit products too.
int gemm_lib() {
  const char* e = std::getenv("XDOT_GEMM_LIB");
  if (e && e[0] == '1') return 2;
  if (e && (e[0] == 'f' || e[0] == 'F')) return 1;  // fp32 only
  return 0;
}

// XDOT_GEMM3: 1 (default) = the automatic path tries the 8-phase kernel first (csrc/gemm3.hip)
int gemm3_auto() {
  const char* e = std::getenv("XDOT_GEMM3");
  return (e && e[0] == '0') ? 0 : 1;
}

double free_device_bytes() {
  size_t fr = 0, tot = 0;
  return hipMemGetInfo(&fr, &tot) == hipSuccess ? (double)fr : -1.0;
}

// the process-level planner inputs, read once
const gp::GemmEnv& gemm_env() {
  static const gp::GemmEnv env{xdot_num_cus(), gemm_lib(), gemm3_auto(), &free_device_bytes};
  return env;
}

// the one way a call's values become the planner's input (xdot.gemm and xdot.gemm_plan)
gp::GemmProblem gemm_problem(int64_t M, int64_t N, int64_t K, int64_t nseg, int64_t nb1, int64_t nb2, int64_t lda,
                             int64_t ldb, int64_t ldc, int64_t sA1, int64_t sA2, int64_t sB1, int64_t sB2, int64_t sC1,
                             int64_t sC2, int64_t sAseg, int64_t sBseg, bool a_mc, bool b_mc, double beta,
                             at::ScalarType dt_in, at::ScalarType dt_out, bool a16, bool b16, bool c16, int64_t path) {
  gp::GemmProblem p{};
  p.M = M; p.N = N; p.K = K; p.nseg = nseg; p.nb1 = nb1; p.nb2 = nb2;
  p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.sA1 = sA1; p.sA2 = sA2; p.sB1 = sB1; p.sB2 = sB2; p.sC1 = sC1; p.sC2 = sC2; p.sAseg = sAseg; p.sBseg = sBseg;
  p.a_mc = a_mc; p.b_mc = b_mc;
  p.beta0 = (float)beta == 0.f;
  p.dt_in = (gp::DType)dt_code(dt_in);
  p.dt_out = (gp::DType)dt_code(dt_out);
  p.esize = p.dt_in == gp::F32 ? 4 : 2;
  p.a16 = a16; p.b16 = b16; p.c16 = c16;
  p.path = (int)path;
  return p;
}

gp::GemmPlan checked_plan(const gp::GemmProblem& p, at::ScalarType dt_in, at::ScalarType dt_out) {
  const gp::GemmPlan pl = gp::plan_gemm(p, gemm_env());
  switch (pl.error) {
    case gp::PLAN_OK: break;
    case gp::ERR_PATH4: TORCH_CHECK(false, "xdot.gemm: path 4 (split fp32) not eligible for this call");
    case gp::ERR_PATH2_F32:
      TORCH_CHECK(false, "xdot.gemm: path 2 (fp32 v2) needs K % 4 == 0 for k-contiguous operands and "
                         "an mn extent % 4 == 0 for mn-contiguous ones");
    case gp::ERR_PATH3_LAYOUT: TORCH_CHECK(false, "xdot.gemm: path 3 (gemm3) needs 16-bit operands with aligned layouts");
    case gp::ERR_PATH3_DECLINED: TORCH_CHECK(false, "xdot.gemm: path 3 (gemm3) not eligible for this call (", pl.rc, ")");
    case gp::ERR_SPLIT3_DECLINED: TORCH_CHECK(false, "xdot.gemm: split fp32 gemm3 launch declined (", pl.rc, ")");
    case gp::ERR_DTYPE: TORCH_CHECK(false, "xdot.gemm: unsupported dtype combination ", dt_in, " -> ", dt_out);
  }
  return pl;
}

// exact-fp32 products: the f32-MFMA kernel of csrc/gemm_f32.hip (fp32 out); anything else (an
// fp32 -> 16-bit output) the generic kernel
int gemm_exact(const xdot::GemmArgs* g, int batches, int dt_in, int dt_out, bool a_mc, bool b_mc, bool vec,
               hipStream_t st) {
  if (dt_in == xdot::DT_F32 && dt_out == xdot::DT_F32) return xdot_gemm_f32_launch(g, batches, a_mc, b_mc, vec, st);
  return xdot_gemm_launch(g, batches, dt_in, dt_out, a_mc, b_mc, vec, st);
}

// LIBRARY: opA / opB / C as strided views of the operands' storage (no copies; the BLAS reads
// leading dimensions / batch strides directly), one batch level, K segments merged
void run_library(const at::Tensor& A, const at::Tensor& B, at::Tensor& C, const gp::GemmProblem& p,
                 const gp::GemmPlan& pl, double alpha, double beta) {
  const int64_t nb = p.nb1 * p.nb2, M = p.M, N = p.N, K = pl.lib_K;
  at::Tensor a = A.as_strided({nb, M, K}, {nb > 1 ? pl.lib_sa : M * K, p.a_mc ? 1 : p.lda, p.a_mc ? p.lda : 1}, A.storage_offset());
  at::Tensor b = B.as_strided({nb, K, N}, {nb > 1 ? pl.lib_sb : K * N, p.b_mc ? p.ldb : 1, p.b_mc ? 1 : p.ldb}, B.storage_offset());
  at::Tensor c = C.as_strided({nb, M, N}, {nb > 1 ? pl.lib_sc : M * N, p.ldc, 1}, C.storage_offset());
  if (nb == 1) {
    at::Tensor c2 = c.select(0, 0);
    at::addmm_out(c2, c2, a.select(0, 0), b.select(0, 0), beta, alpha);
  } else {
    at::baddbmm_out(c, c, a, b, beta, alpha);
  }
}

// SPLIT3: hi/lo bf16 copies of both operands, A' = [hi, lo, hi], B' = [hi, hi, lo] (hi.hi + lo.hi +
// hi.lo), one gemm3 call over 3x the K segments of the compact copies
void run_split3(const at::Tensor& A, const at::Tensor& B, const xdot::GemmArgs& g, const gp::GemmProblem& p,
                int S, float* ws, hipStream_t st) {
  const int64_t nb = p.nb1 * p.nb2, nseg = p.nseg;
  const int64_t Ra = p.a_mc ? p.K : p.M, Ca = p.a_mc ? p.M : p.K, Rb = p.b_mc ? p.K : p.N, Cb = p.b_mc ? p.N : p.K;
  at::Tensor a3 = at::empty({nb * 3 * nseg * Ra * Ca}, A.options().dtype(at::kBFloat16));
  at::Tensor b3 = at::empty({nb * 3 * nseg * Rb * Cb}, A.options().dtype(at::kBFloat16));
  xdot_split3_launch(A.data_ptr<float>(), a3.data_ptr(), p.sA1, p.sA2, p.sAseg, p.lda, (int)p.nb1, (int)p.nb2, (int)nseg,
                     (int)Ra, (int)Ca, 0b010, st);
  xdot_split3_launch(B.data_ptr<float>(), b3.data_ptr(), p.sB1, p.sB2, p.sBseg, p.ldb, (int)p.nb1, (int)p.nb2, (int)nseg,
                     (int)Rb, (int)Cb, 0b100, st);
  check_launch(hipGetLastError(), "split3");
  xdot::GemmArgs g3 = g;
  g3.A = a3.data_ptr();
  g3.B = b3.data_ptr();
  g3.nseg = (int)(3 * nseg);
  g3.lda = Ca;
  g3.ldb = Cb;
  g3.sAseg = Ra * Ca;
  g3.sBseg = Rb * Cb;
  g3.sA2 = 3 * nseg * Ra * Ca;
  g3.sA1 = p.nb2 * g3.sA2;
  g3.sB2 = 3 * nseg * Rb * Cb;
  g3.sB1 = p.nb2 * g3.sB2;
  const int rc3 = xdot_gemm3_launch(&g3, (int)nb, xdot::DT_BF16, xdot::DT_F32, p.a_mc, p.b_mc, S, ws, st);
  TORCH_CHECK(rc3 == 0, "xdot.gemm: split fp32 gemm3 launch declined (", rc3, ")");
  check_launch(hipGetLastError(), "gemm3 (split fp32)");
}

// SLABS: slab s of every (batch, segment) is one outer batch entry of the 128x128 kernel writing an
// fp32 partial (the short last slab in a launch of its own); one ordered sum applies alpha / beta / the cast
void run_slabs(const at::Tensor& A, const at::Tensor& B, const xdot::GemmArgs& g, const gp::GemmProblem& p,
               const gp::GemmPlan& pl, int dt_in, int dt_out, hipStream_t st) {
  const int64_t M = p.M, N = p.N, nb2 = p.nb2, Ks = pl.Ks, S = pl.slabs, full = pl.full;
  at::Tensor ws = at::empty({S * nb2 * M * N}, A.options().dtype(at::kFloat));
  xdot::GemmArgs gs = g;
  gs.C = ws.data_ptr();
  gs.ldc = N;
  gs.sC2 = M * N;
  gs.sC1 = nb2 * M * N;
  gs.alpha = 1.f;
  gs.beta = 0.f;
  gs.sA1 = p.a_mc ? Ks * p.lda : Ks;
  gs.sB1 = p.b_mc ? Ks * p.ldb : Ks;
  gs.K = (int)Ks;
  int rc1 = gemm_exact(&gs, (int)(full * nb2), dt_in, xdot::DT_F32, p.a_mc, p.b_mc, pl.vec_full, st);
  if (rc1 == 0 && full < S) {  // the short last slab
    xdot::GemmArgs gl = gs;
    const int64_t k0 = full * Ks;
    gl.A = static_cast<const char*>(A.data_ptr()) + A.element_size() * (p.a_mc ? k0 * p.lda : k0);
    gl.B = static_cast<const char*>(B.data_ptr()) + B.element_size() * (p.b_mc ? k0 * p.ldb : k0);
    gl.C = ws.data_ptr<float>() + full * nb2 * M * N;
    gl.K = (int)(p.K - k0);
    rc1 = gemm_exact(&gl, (int)nb2, dt_in, xdot::DT_F32, p.a_mc, p.b_mc, pl.vec_last, st);
  }
  TORCH_CHECK(rc1 == 0, "xdot.gemm: unsupported dtype combination ", A.scalar_type(), " -> fp32 slabs");
  check_launch(hipGetLastError(), "gemm (K slabs)");
  TORCH_CHECK(xdot_gemm_reduce_launch(&g, ws.data_ptr<float>(), (int)S, (int)nb2, dt_out, st) == 0,
              "xdot.gemm: slab reduce dtype");
  check_launch(hipGetLastError(), "gemm slab reduce");
}

// ------------------------------------------------------------------------------------
void gemm(const at::Tensor& A, const at::Tensor& B, at::Tensor& C, int64_t M, int64_t N,
          int64_t K, int64_t nseg, int64_t nb1, int64_t nb2, int64_t lda, int64_t ldb,
          int64_t ldc, int64_t sA1, int64_t sA2, int64_t sB1, int64_t sB2, int64_t sC1,
          int64_t sC2, int64_t sAseg, int64_t sBseg, bool a_mc, bool b_mc, double alpha, double beta,
          int64_t path) {
  Range rr_("xdot.gemm");
  TORCH_CHECK(A.is_cuda() && B.is_cuda() && C.is_cuda(), "xdot.gemm: tensors must be on GPU");
  TORCH_CHECK(A.scalar_type() == B.scalar_type(), "xdot.gemm: A/B dtype mismatch");
  TORCH_CHECK(M >= 0 && N >= 0 && K >= 0 && nseg >= 1 && nb1 >= 1 && nb2 >= 1, "xdot.gemm: bad sizes");
  if (M == 0 || N == 0) return;
  TORCH_CHECK(M < (1LL << 31) && N < (1LL << 31) && K < (1LL << 31), "xdot.gemm: dim too large");
  TORCH_CHECK(nb1 * nb2 <= 65535, "xdot.gemm: too many batches");
  // host-side bounds check of the furthest element each operand touches
  auto last = [](int64_t b1, int64_t s1, int64_t b2, int64_t s2, int64_t ns, int64_t ss) {
    return (b1 - 1) * s1 + (b2 - 1) * s2 + (ns - 1) * ss;
  };
  if (K > 0) {
    const int64_t la = last(nb1, sA1, nb2, sA2, nseg, sAseg) + (a_mc ? (K - 1) * lda + (M - 1) : (M - 1) * lda + (K - 1));
    const int64_t lb = last(nb1, sB1, nb2, sB2, nseg, sBseg) + (b_mc ? (K - 1) * ldb + (N - 1) : (N - 1) * ldb + (K - 1));
    TORCH_CHECK(la < avail_elems(A), "xdot.gemm: A access out of bounds (", la, " >= ", avail_elems(A), ")");
    TORCH_CHECK(lb < avail_elems(B), "xdot.gemm: B access out of bounds (", lb, " >= ", avail_elems(B), ")");
  }
  const int64_t lc = last(nb1, sC1, nb2, sC2, 1, 0) + (M - 1) * ldc + (N - 1);
  TORCH_CHECK(lc < avail_elems(C), "xdot.gemm: C access out of bounds");

  const gp::GemmProblem p = gemm_problem(M, N, K, nseg, nb1, nb2, lda, ldb, ldc, sA1, sA2, sB1, sB2, sC1, sC2, sAseg, sBseg,
                                         a_mc, b_mc, beta, A.scalar_type(), C.scalar_type(), aligned16(A.data_ptr()),
                                         aligned16(B.data_ptr()), aligned16(C.data_ptr()), path);
  xdot::GemmArgs g{};
  g.A = A.data_ptr(); g.B = B.data_ptr(); g.C = C.data_ptr();
  g.M = (int)M; g.N = (int)N; g.K = (int)K; g.nseg = (int)nseg; g.nb2 = (int)nb2;
  g.lda = lda; g.ldb = ldb; g.ldc = ldc;
  g.sA1 = sA1; g.sA2 = sA2; g.sB1 = sB1; g.sB2 = sB2; g.sC1 = sC1; g.sC2 = sC2;
  g.sAseg = sAseg; g.sBseg = sBseg; g.alpha = (float)alpha; g.beta = (float)beta;
  c10::DeviceGuard guard(A.device());
  const gp::GemmPlan pl = checked_plan(p, A.scalar_type(), C.scalar_type());

  const int nb = (int)(nb1 * nb2), S = (int)pl.splits, dti = (int)p.dt_in, dto = (int)p.dt_out;
  hipStream_t st = cur_stream(A);
  at::Tensor ws;  // fp32 partials of the split-K routes
  if (S > 1) ws = at::empty({S * nb1 * nb2 * M * N}, A.options().dtype(at::kFloat));
  float* wsp = ws.defined() ? ws.data_ptr<float>() : nullptr;
  // the planner has asked every eligibility rule: a launcher that declines its route is a bug, never a second route
  auto took = [&](int rc, const char* what) {
    TORCH_CHECK(rc == 0, "xdot.gemm: planned ", what, " but its launcher declined (", rc, ")");
    check_launch(hipGetLastError(), what);
  };
  switch (pl.route) {
    case gp::SPLIT3: run_split3(A, B, g, p, S, wsp, st); break;
    case gp::LIBRARY: run_library(A, B, C, p, pl, alpha, beta); break;
    case gp::G2_F32: took(xdot_gemm2_f32_launch(&g, nb, a_mc, b_mc, S, wsp, st), "gemm2_f32"); break;
    case gp::G3: took(xdot_gemm3_launch(&g, nb, dti, dto, a_mc, b_mc, S, wsp, st), "gemm3"); break;
    case gp::G2: took(xdot_gemm2_launch(&g, nb, dti, dto, a_mc, b_mc, S, wsp, st), "gemm2"); break;
    case gp::SLABS: run_slabs(A, B, g, p, pl, dti, dto, st); break;
    case gp::G1: took(gemm_exact(&g, nb, dti, dto, a_mc, b_mc, pl.vec, st), "gemm"); break;
  }
}

// The plan xdot.gemm would execute for these values (no tensors, nothing launched; raises where
// xdot.gemm raises): [route, splits, slab length, full slabs, plain vec, slabs, full-slab vec, last-slab vec],
// route numbered as gp::Route (SPLIT3 0, LIBRARY, G2_F32, G3, G2, SLABS, G1 6)
std::vector<int64_t> gemm_plan(int64_t M, int64_t N, int64_t K, int64_t nseg, int64_t nb1, int64_t nb2, int64_t lda,
                               int64_t ldb, int64_t ldc, int64_t sA1, int64_t sA2, int64_t sB1, int64_t sB2, int64_t sC1,
                               int64_t sC2, int64_t sAseg, int64_t sBseg, bool a_mc, bool b_mc, double beta,
                               at::ScalarType dt_in, at::ScalarType dt_out, bool a16, bool b16, bool c16, int64_t path) {
  const gp::GemmPlan pl = checked_plan(gemm_problem(M, N, K, nseg, nb1, nb2, lda, ldb, ldc, sA1, sA2, sB1, sB2, sC1, sC2,
                                                    sAseg, sBseg, a_mc, b_mc, beta, dt_in, dt_out, a16, b16, c16, path),
                                       dt_in, dt_out);
  return {(int64_t)pl.route, pl.splits, pl.Ks, pl.full, (int64_t)pl.vec, pl.slabs, (int64_t)pl.vec_full, (int64_t)pl.vec_last};
}

// Projection GEMM (csrc/gemm_proj.hip): nn = false: y = x Wᵀ (+ bias), W (N, K); nn = true:
// dx = dy W, W (K, N) (the input gradient of the same Linear).  x: (..., K) with unit last
// stride; out (optional): an (M, N) row-major view to write (e.g. this rank's block of the
// all-gather buffer).  Shapes / layouts the kernel does not take, and (force = 0) products
// large enough for the library to be faster, run on the library GEMM.
at::Tensor proj(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias, bool nn,
                const c10::optional<at::Tensor>& out, int64_t force, double alpha) {
  Range rr_("xdot.proj");
  TORCH_CHECK(x.is_cuda() && w.is_cuda() && w.dim() == 2 && x.dim() >= 1 && x.scalar_type() == w.scalar_type(),
              "xdot.proj: device tensors of one dtype, 2-D weight");
  const int64_t K = x.size(-1);
  const int64_t N = nn ? w.size(1) : w.size(0);
  TORCH_CHECK((nn ? w.size(0) : w.size(1)) == K, "xdot.proj: weight ", w.sizes(), " does not match input features ", K);
  at::Tensor a = x.dim() == 2 ? x : x.reshape({-1, K});
  if (a.stride(1) != 1) a = a.contiguous();
  const int64_t M = a.size(0);
  std::vector<int64_t> oshape(x.sizes().begin(), x.sizes().end() - 1);
  oshape.push_back(N);
  at::Tensor c;
  if (out.has_value()) {
    c = *out;
    TORCH_CHECK(c.is_cuda() && c.dim() == 2 && c.size(0) == M && c.size(1) == N && c.stride(1) == 1 &&
                    c.scalar_type() == x.scalar_type(),
                "xdot.proj: out must be an (M, N) row-major view of the input dtype");
  } else {
    c = at::empty({M, N}, x.options());
  }
  const bool has_b = bias.has_value() && bias->defined();
  TORCH_CHECK(!has_b || (!nn && bias->numel() == N && bias->is_contiguous() && bias->scalar_type() == x.scalar_type()),
              "xdot.proj: bias must be a contiguous (N,) tensor of the input dtype (forward only)");
  int rc = -3;
  if (M > 0 && (x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kHalf) && w.stride(1) == 1 &&
      M <= INT32_MAX && N <= INT32_MAX && K <= INT32_MAX) {
    xdot::ProjArgs p{};
    p.A = a.data_ptr();
    p.B = w.data_ptr();
    p.bias = has_b ? bias->data_ptr() : nullptr;
    p.C = c.data_ptr();
    p.M = (int)M;
    p.N = (int)N;
    p.K = (int)K;
    p.lda = a.stride(0);
    p.ldb = w.stride(0);
    p.ldc = c.stride(0);
    p.alpha = (float)alpha;
    // every address the kernel can touch lies inside the operands' storage
    TORCH_CHECK((M - 1) * p.lda + K <= avail_elems(a) && (nn ? (K - 1) * p.ldb + N : (N - 1) * p.ldb + K) <= avail_elems(w) &&
                    (M - 1) * p.ldc + N <= avail_elems(c),
                "xdot.proj: operand extents exceed their storage");
    c10::DeviceGuard guard(x.device());
    rc = xdot_gemm_proj_launch(&p, dt_code(x.scalar_type()), nn ? 1 : 0, (int)force, cur_stream(x));
    if (rc != -3) check_launch((hipError_t)rc, "gemm_proj");
  }
  if (rc == -3) {  // library GEMM (alpha scales the bias too: C = alpha (A op(B) + bias), one rounding)
    const at::Tensor wt = nn ? w : w.t();
    if (has_b) at::addmm_out(c, *bias, a, wt, alpha, alpha);
    else if (alpha == 1.0) at::mm_out(c, a, wt);
    else at::addmm_out(c, c, a, wt, 0.0, alpha);
  }
  return out.has_value() ? c : c.view(oshape);
}

// Weight gradient of a Linear: dy (K, M), x (K, N) row-major 16-bit -> dyᵀ x (M, N) in out_dtype,
// fp32 accumulation (csrc/gemm_wgrad.hip: S slabs of K -> fp32 partials -> one ordered sum).
// splits 0: the slab count from the cost model of gemm_plan.h (wgrad_slabs).  Returns an undefined tensor
// when the shape is not eligible (the caller takes another route).
struct WgradProb {
  at::Tensor dy, x, part;
  int64_t K, M, N, S;
};

bool wgrad_prob(const at::Tensor& dy, const at::Tensor& x, int64_t splits, WgradProb& q) {
  TORCH_CHECK(dy.is_cuda() && x.is_cuda() && dy.dim() == 2 && x.dim() == 2 && dy.size(0) == x.size(0) &&
                  dy.scalar_type() == x.scalar_type() && dy.stride(1) == 1 && x.stride(1) == 1,
              "xdot.wgrad: (K, M) and (K, N) row-major device tensors of one dtype");
  const int64_t K = dy.size(0), M = dy.size(1), N = x.size(1);
  if (K < 1 || M % 128 || N % 128 || (dy.scalar_type() != at::kBFloat16 && dy.scalar_type() != at::kHalf) ||
      M > INT32_MAX || N > INT32_MAX || K > INT32_MAX)
    return false;
  const int64_t S = gp::wgrad_slabs(K, M, N, splits);
  TORCH_CHECK((K - 1) * dy.stride(0) + M <= avail_elems(dy) && (K - 1) * x.stride(0) + N <= avail_elems(x),
              "xdot.wgrad: operand extents exceed their storage");
  q = WgradProb{dy, x, at::empty({S, M, N}, dy.options().dtype(at::kFloat)), K, M, N, S};
  return true;
}

// launch 1 or 2 products in one kernel, then one ordered sum per product; empty when not eligible
std::vector<at::Tensor> wgrad_run(std::vector<WgradProb>& qs, at::ScalarType out_dtype) {
  const int np = (int)qs.size();
  const void* A[2];
  const void* B[2];
  float* part[2];
  int M[2], N[2], K[2], S[2];
  int64_t lda[2], ldb[2];
  for (int i = 0; i < np; ++i) {
    A[i] = qs[i].dy.data_ptr(); B[i] = qs[i].x.data_ptr(); part[i] = qs[i].part.data_ptr<float>();
    M[i] = (int)qs[i].M; N[i] = (int)qs[i].N; K[i] = (int)qs[i].K; S[i] = (int)qs[i].S;
    lda[i] = qs[i].dy.stride(0); ldb[i] = qs[i].x.stride(0);
  }
  const at::Tensor& d0 = qs[0].dy;
  c10::DeviceGuard guard(d0.device());
  const int rc = xdot_gemm_wgrad_launch(np, A, B, part, M, N, K, S, lda, ldb, dt_code(d0.scalar_type()), cur_stream(d0));
  if (rc == -3) return {};
  check_launch((hipError_t)rc, "gemm_wgrad");
  std::vector<at::Tensor> outs;
  for (int i = 0; i < np; ++i) outs.push_back(at::empty({qs[i].M, qs[i].N}, d0.options().dtype(out_dtype)));
  if (np == 2) {  // both ordered sums in one launch
    TORCH_CHECK(xdot_sum_partials2_launch(part[0], outs[0].data_ptr(), S[0], qs[0].M * qs[0].N, part[1],
                                          outs[1].data_ptr(), S[1], qs[1].M * qs[1].N, dt_code(out_dtype),
                                          cur_stream(d0)) == 0, "xdot.wgrad2: out dtype");
    check_launch(hipGetLastError(), "wgrad2 sum");
    return outs;
  }
  for (int i = 0; i < np; ++i) {
    TORCH_CHECK(xdot_sum_partials_launch(part[i], outs[i].data_ptr(), S[i], qs[i].M * qs[i].N, dt_code(out_dtype),
                                         cur_stream(d0)) == 0, "xdot.wgrad: out dtype");
    check_launch(hipGetLastError(), "wgrad sum");
  }
  return outs;
}

at::Tensor wgrad(const at::Tensor& dy, const at::Tensor& x, at::ScalarType out_dtype, int64_t splits) {
  Range rr_("xdot.wgrad");
  std::vector<WgradProb> qs(1);
  if (!wgrad_prob(dy, x, splits, qs[0])) return at::Tensor();
  auto outs = wgrad_run(qs, out_dtype);
  return outs.empty() ? at::Tensor() : outs[0];
}

// two weight gradients in ONE launch (the fused backward's dWk and dW[q|v]); [] when either
// shape is not eligible
std::vector<at::Tensor> wgrad2(const at::Tensor& dy0, const at::Tensor& x0, const at::Tensor& dy1,
                               const at::Tensor& x1, at::ScalarType out_dtype) {
  Range rr_("xdot.wgrad2");
  TORCH_CHECK(dy0.scalar_type() == dy1.scalar_type() && dy0.device() == dy1.device(), "xdot.wgrad2: dtype / device");
  std::vector<WgradProb> qs(2);
  if (!wgrad_prob(dy0, x0, 0, qs[0]) || !wgrad_prob(dy1, x1, 0, qs[1])) return {};
  return wgrad_run(qs, out_dtype);
}

}  // namespace

TORCH_LIBRARY_IMPL(xdot, CompositeExplicitAutograd, m) {
  m.impl("gemm_plan", &gemm_plan);
}

TORCH_LIBRARY_IMPL(xdot, CUDA, m) {
  m.impl("gemm", &gemm);
  m.impl("proj", &proj);
  m.impl("wgrad", &wgrad);
  m.impl("wgrad2", &wgrad2);
}
