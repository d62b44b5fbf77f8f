// xdot — route planning of xdot.gemm: which kernel a strided product runs on, with how many split-K
// slices or K slabs.  Host-only arithmetic over standard headers (plain g++ compiles it:
// tests/test_gemm_plan.py); bindings_gemm.cpp describes a call as a GemmProblem, asks plan_gemm and
// executes the plan, the op xdot.gemm_plan returns the same plan without launching anything.
#pragma once
#include <algorithm>
#include <cstdint>

namespace xdot {
namespace gp {

// the codes of xdot::DType (kernels.h, which needs the HIP headers; bindings_gemm.cpp asserts the match)
enum DType : int { F32 = 0, BF16 = 1, F16 = 2 };

// Everything the route decision reads of one call, and nothing else.  Strides in elements.
struct GemmProblem {
  int64_t M, N, K, nseg, nb1, nb2;
  int64_t lda, ldb, ldc;
  int64_t sA1, sA2, sB1, sB2, sC1, sC2, sAseg, sBseg;
  bool a_mc, b_mc;     // operand stored mn-contiguous (else k-contiguous)
  bool beta0;          // (float)beta == 0: C is not read
  DType dt_in, dt_out;
  int esize;           // bytes per operand element
  bool a16, b16, c16;  // base address 16-byte aligned
  int path;            // 0 auto, 1 .. 5 forced kernels, 6 auto with split fp32 allowed (xdot.ops.gemm.strided_gemm)
};

// The process-level inputs.
struct GemmEnv {
  int64_t ncu;           // compute units of the device
  int gemm_lib;          // XDOT_GEMM_LIB: 0 no product on the library GEMM, 1 exact-fp32 ones, 2 16-bit ones too
  int gemm3_auto;        // XDOT_GEMM3: 1 = the automatic path prefers the 8-phase kernel
  double (*free_bytes)();  // free device memory, < 0 when the query fails; asked only when the
                           // split-fp32 operand copies reach 1e9 bytes
};

enum Route : int { SPLIT3 = 0, LIBRARY, G2_F32, G3, G2, SLABS, G1 };

// the calls that raise instead of launching
enum PlanError : int {
  PLAN_OK = 0,
  ERR_PATH4,            // path 4 (split fp32) not eligible
  ERR_PATH2_F32,        // path 2 on fp32 operands whose extents break the 256x256 kernel's rules
  ERR_PATH3_LAYOUT,     // path 3 without 16-bit operands in aligned layouts
  ERR_PATH3_DECLINED,   // path 3 and the 8-phase kernel does not take the call (rc: its code)
  ERR_SPLIT3_DECLINED,  // split fp32 chosen and the 8-phase kernel does not take its product
  ERR_DTYPE,            // no kernel for this operand -> output dtype pair
};

struct GemmPlan {
  Route route = G1;
  int64_t splits = 1;  // split-K slices (SPLIT3, G2_F32, G3, G2)
  // SLABS: `slabs` K slabs of length Ks, the first `full` of them whole, then (full < slabs) one short one
  int64_t Ks = 0, slabs = 0, full = 0;
  bool vec_full = false, vec_last = false;  // 16-byte operand loads in the full / the last slab
  bool vec = false;                         // 16-byte operand loads from the call's own layout (G1)
  // LIBRARY: the one batch level and the merged K the BLAS call is expressed with
  int64_t lib_K = 0, lib_sa = 0, lib_sb = 0, lib_sc = 0;
  PlanError error = PLAN_OK;
  int rc = 0;  // ERR_PATH3_DECLINED / ERR_SPLIT3_DECLINED: the launcher's code (-3 shape, -1 dtype pair)
};

// split-K: fewest k-slices S minimising ceil(items / CUs) / S (idle CUs of the last round),
// each slice >= 4 k-tiles, with a 3 % charge per slice for the fp32 partial round trip
inline int64_t pick_splits(int64_t tiles, int64_t kt, int64_t ncu) {
  int64_t S = 1;
  double best = 1e300;
  for (int64_t s = 1; s <= 64 && (s == 1 || kt / s >= 4); ++s) {
    const double cost = (double)((tiles * s + ncu - 1) / ncu) / (double)s * (1.0 + 0.03 * (s - 1));
    if (cost < best * 0.98) { best = cost; S = s; }
  }
  return S;
}

inline int64_t tiles256(int64_t M, int64_t N) { return ((M + 255) / 256) * ((N + 255) / 256); }

// The 8-phase kernel (csrc/gemm3.hip: 256x256 tiles, 64-deep k-tiles, persistent workgroups with
// at most G3_MAX_ITEMS work items each) takes a product with beta = 0 and M, N >= 256.  K % 8: a
// k-contiguous operand's K tail is zero-filled per 16-byte chunk; two mn-contiguous operands (the
// weight gradients dYᵀ·X, K = the sequence rows) are tail-filled per k row, any K.  Every split-K
// slice needs one k-tile.  xdot_gemm3_launch returns -3 through this; plan_gemm asks it first.
constexpr int G3_BM = 256, G3_BN = 256, G3_BK = 64, G3_MAX_ITEMS = 2048;
inline bool gemm3_takes(int64_t M, int64_t N, int64_t K, int64_t nseg, int64_t batches, int64_t splits, bool a_mc,
                        bool b_mc, bool beta0, int64_t ncu) {
  if (M < G3_BM || N < G3_BN || ((K % 8) != 0 && !(a_mc && b_mc)) || !beta0) return false;
  if (batches == 0 || K == 0) return false;
  if (((K + G3_BK - 1) / G3_BK) * nseg < splits) return false;
  const int64_t tm = (M + G3_BM - 1) / G3_BM, tn = (N + G3_BN - 1) / G3_BN;
  const int64_t W = tm * tn * batches * splits;
  return (W + ncu - 1) / ncu <= G3_MAX_ITEMS && tm <= 65535 && tn <= 65535;
}

// dtype pairs of the 16-bit 256x256 kernels (gemm2, gemm3) and of the 128x128 kernels (gemm, gemm_f32)
inline bool pair16(DType i, DType o) { return (i == BF16 || i == F16) && (o == i || o == F32); }
inline bool pair_g1(DType i, DType o) { return pair16(i, o) || (i == F32 && (o == F32 || o == BF16)); }

// operand loads vectorise on A/B alignment alone; the output is stored 16 bytes at a time
// wherever the address allows, element by element elsewhere (the kernels test each strip's
// address: an odd column block of nt's (P, R, T) output at T/N = 3125 must not turn every
// operand load of the GEMM into element loads)
inline bool operand_vec(const GemmProblem& p) {
  const int64_t eps = 16 / p.esize;
  auto mult = [&](int64_t v) { return v % eps == 0; };
  return p.a16 && p.b16 && mult(p.lda) && mult(p.ldb) && mult(p.sA1) && mult(p.sA2) && mult(p.sB1) && mult(p.sB2) &&
         mult(p.sAseg) && mult(p.sBseg);
}

// Split fp32 (three bf16 products of hi/lo operand copies on gemm3) against the exact kernel, for an
// eligible call with `s3` split-K slices.  Worth it when three bf16 products plus the operand
// copies (read 4 B, write 6 B per element) beat one exact fp32 product: a product whose operand is
// far larger than its output (the materialised P.V: 2.5 GB of P per head) keeps the exact kernel.
// Both sides are priced at the fraction of the CUs their grid fills: the exact kernel has no
// split-K (128x128 tiles), gemm3 splits K, so a product with few output tiles and a long K (the
// K = T weight-side products of the autograd ops) goes split.  The hi/lo copies are transient HBM
// (6 B per operand element): never more than a quarter of what is free.
inline bool split3_pays(const GemmProblem& p, const GemmEnv& env, int64_t s3) {
  const int64_t nb = p.nb1 * p.nb2;
  const double flop = 2.0 * (double)p.M * p.N * p.K * p.nseg * p.nb1 * p.nb2;
  const double elems = (double)p.nb1 * p.nb2 * p.nseg * p.K * ((double)p.M + (double)p.N);
  const int64_t t128 = ((p.M + 127) / 128) * ((p.N + 127) / 128) * nb;
  const double fill1 = std::min(1.0, (double)t128 / (double)env.ncu);
  const double fill3 = std::min(1.0, (double)(tiles256(p.M, p.N) * nb * s3) / (double)env.ncu);
  const double t_split = 3.0 * flop / (1.1e15 * fill3) + 10.0 * elems / 5e12 +
                         (s3 > 1 ? 8.0 * (double)s3 * p.M * p.N * p.nb1 * p.nb2 / 5e12 : 0.0);
  const double t_exact = flop / (1.15e14 * fill1);
  const double copy_bytes = 6.0 * elems;
  const bool fits = copy_bytes < 1e9 || copy_bytes < 0.25 * env.free_bytes();
  return flop >= 2e9 && t_split < t_exact && fits;
}

// The library GEMM (at::addmm / baddbmm on strided views) takes plain large products: operands and
// output of one dtype, one batch level, K segments that continue each other, every output batch its
// own dense matrix of whole rows (no batches interleaved inside one output row -- the per-rank
// column blocks of nt's (P, R, T) output, which faulted on this route, stay on the xdot kernels;
// input batches may interleave or be broadcast), 16-byte aligned bases, leading dims and batch
// strides.  16-bit: only where the output alone fills >= 2 rounds of 256x256 tiles (skinny long-K
// products keep the split-K kernel); fp32: every product of >= 2e10 flop.
inline bool library_takes(const GemmProblem& p, GemmPlan* v) {
  if (p.dt_out != p.dt_in || p.K == 0) return false;
  const int64_t nb = p.nb1 * p.nb2;
  int64_t sa = 0, sb = 0, sc = 0, K = p.K;
  if (p.nb1 == 1) { sa = p.sA2; sb = p.sB2; sc = p.sC2; }
  else if (p.nb2 == 1) { sa = p.sA1; sb = p.sB1; sc = p.sC1; }
  else if (p.sA1 == p.nb2 * p.sA2 && p.sB1 == p.nb2 * p.sB2 && p.sC1 == p.nb2 * p.sC2) { sa = p.sA2; sb = p.sB2; sc = p.sC2; }
  else return false;
  if (p.nseg > 1) {
    if (p.sAseg != (p.a_mc ? K * p.lda : K) || p.sBseg != (p.b_mc ? K * p.ldb : K)) return false;
    K *= p.nseg;
  }
  if (nb > 1 && (sa < 0 || sb < 0 || sc < p.M * p.ldc)) return false;
  const int64_t ev = 16 / p.esize;
  auto al = [&](int64_t x) { return x % ev == 0; };
  if (p.ldc != p.N) return false;
  if (!p.a16 || !p.b16 || !p.c16 || !al(p.lda) || !al(p.ldb) || !al(p.ldc) || (nb > 1 && (!al(sa) || !al(sb) || !al(sc))))
    return false;
  const double flop = 2.0 * (double)p.M * (double)p.N * (double)K * (double)nb;
  if (flop < 2e10 || (p.esize == 2 && tiles256(p.M, p.N) * nb < 512)) return false;
  v->lib_K = K; v->lib_sa = sa; v->lib_sb = sb; v->lib_sc = sc;
  return true;
}

// extents the 256x256 LDS-DMA kernels stream 16 bytes at a time (`q` elements: 4 fp32, gemm2_f32.hip;
// 8 16-bit, gemm2.hip / gemm3.hip): K of a k-contiguous operand, the mn extent of an mn-contiguous one
inline bool dma_extents(const GemmProblem& p, int64_t q) {
  return ((p.a_mc && p.b_mc) || p.K % q == 0) && (!p.a_mc || p.M % q == 0) && (!p.b_mc || p.N % q == 0);
}

// K slabs for the 128x128 kernels: a product with few output tiles and a long K (the K = T
// weight-side products of the autograd ops: e.g. 1562 x 768 x 12496 = 78 tiles) would leave most
// CUs idle.  Slab s of every (batch, segment) is one outer batch entry writing an fp32 partial
// (<= 256 MB in all); one ordered sum applies alpha / beta / the cast.  false: fewer than 2 slabs.
inline bool slab_geometry(const GemmProblem& p, bool vec, GemmPlan* v) {
  const int64_t tiles = ((p.M + 127) / 128) * ((p.N + 127) / 128) * p.nb2;
  if (tiles >= 384) return false;
  int64_t S = std::min<int64_t>(std::min<int64_t>((768 + tiles - 1) / tiles, p.K / 256), 32);
  S = std::min<int64_t>(S, (int64_t)(64 << 20) / std::max<int64_t>(1, p.nb2 * p.M * p.N));
  const int64_t Ks = ((p.K + S - 1) / S + 15) / 16 * 16;
  S = (p.K + Ks - 1) / Ks;
  if (S < 2) return false;
  const int64_t eps = 16 / p.esize;
  v->Ks = Ks;
  v->slabs = S;
  v->full = p.K / Ks == S ? S : S - 1;
  v->vec_full = vec && (Ks * (p.a_mc ? p.lda : 1)) % eps == 0 && (Ks * (p.b_mc ? p.ldb : 1)) % eps == 0;
  const int64_t k0 = v->full * Ks;
  v->vec_last = v->full < S && v->vec_full && (p.a_mc ? k0 * p.lda : k0) % eps == 0 && (p.b_mc ? k0 * p.ldb : k0) % eps == 0;
  return true;
}

inline GemmPlan plan_error(GemmPlan pl, PlanError e, int rc = 0) {
  pl.error = e;
  pl.rc = rc;
  return pl;
}

// The route of one call, first match wins: split fp32, the library, the exact-fp32 256x256 kernel,
// the 8-phase kernel, the 16-bit 256x256 kernel, K slabs of the 128x128 kernels, the 128x128 kernels.
inline GemmPlan plan_gemm(const GemmProblem& p, const GemmEnv& env) {
  GemmPlan pl;
  const int64_t nb = p.nb1 * p.nb2, tpb = tiles256(p.M, p.N), tiles = tpb * nb;
  const bool vec = pl.vec = operand_vec(p);
  int mode = p.path;
  // fp32 operands on the bf16 matrix pipe (path 6 = automatic with split allowed, path 4 forces it):
  // hi/lo bf16 copies, three bf16 products in one gemm3 call over 3x the K segments
  if (p.dt_in == F32 && (mode == 4 || (mode == 6 && env.gemm3_auto))) {
    const int64_t s3 = pick_splits(tiles, 3 * p.nseg * ((p.K + 63) / 64), env.ncu);
    const bool pays = split3_pays(p, env, s3);
    const bool ok = p.beta0 && p.K > 0 && p.M >= 256 && p.N >= 256 && p.K % 8 == 0 && (!p.a_mc || p.M % 8 == 0) &&
                    (!p.b_mc || p.N % 8 == 0) && p.dt_out == F32 && nb * 3 * p.nseg <= 65535;
    if (mode == 4 && !ok) return plan_error(pl, ERR_PATH4);
    if (ok && (mode == 4 || pays)) {
      pl.route = SPLIT3;
      pl.splits = s3;
      if (!gemm3_takes(p.M, p.N, p.K, 3 * p.nseg, nb, s3, p.a_mc, p.b_mc, true, env.ncu))
        return plan_error(pl, ERR_SPLIT3_DECLINED, -3);
      return pl;
    }
  }
  if (mode == 6) mode = 0;
  if (mode == 0 && (env.gemm_lib == 2 || (env.gemm_lib == 1 && p.dt_in == F32)) && library_takes(p, &pl)) {
    pl.route = LIBRARY;
    return pl;
  }
  // exact fp32: the persistent 256x256 LDS-DMA kernel (csrc/gemm2_f32.hip) where its layout rules
  // hold (16-byte operand rows: `vec`, dma_extents) and the output has at least one 128-wide tile in
  // each direction; split-K over 32-deep k-tiles, partials <= 512 MB.  path 1 keeps the 128x128
  // kernel, path 2 forces this one.
  if (p.dt_in == F32 && p.dt_out == F32 && vec && p.K > 0 && mode != 1) {
    const bool ok = dma_extents(p, 4);
    if (mode == 2 && !ok) return plan_error(pl, ERR_PATH2_F32);
    // auto: >= 2 rounds of 256x256 tiles, or a long K (split-K fills the GPU).  Short-K products
    // with few tiles (the 25000 x 768 x 768 projections: 294 tiles, K = 768) stay on the 128x128
    // kernel: 82-94 TF/s there vs 63-65 for this one split 4-6 ways
    if (ok && (mode == 2 || (p.M >= 128 && p.N >= 128 && (tiles >= 512 || p.K * p.nseg >= 4096)))) {
      int64_t S = pick_splits(tiles, p.nseg * ((p.K + 31) / 32), env.ncu);
      while (S > 1 && S * nb * p.M * p.N > (128LL << 20)) --S;
      pl.route = G2_F32;
      pl.splits = S;
      return pl;
    }
  }
  // 16-bit operands whose layout meets the 256x256 kernels' rules.  auto: enough 256x256 tiles
  // (>= 32 per batch entry or >= 512 overall) -- small outputs batched over K slabs (the split-K
  // weight gradients of xdot.ops.linear) keep the 128x128 kernel, which fills the GPU without a
  // second split.  Skinny outputs (one side 64..191, e.g. N = head dim 96 in the materialised
  // path) still go here: streaming the long operand through the deeper LDS-DMA ring beats the
  // 128x128 kernel's register staging even with 62 % of the tile idle
  bool v2 = p.esize == 2 && vec && mode != 1 && dma_extents(p, 8);
  if (v2 && mode != 2 && mode != 3 && mode != 5) v2 = p.M >= 64 && p.N >= 64 && (tpb >= 32 || tiles >= 512);
  if (mode == 3 && !(v2 && p.K > 0)) return plan_error(pl, ERR_PATH3_LAYOUT);
  if (v2 && p.K > 0) {
    const int64_t S = pick_splits(tiles, p.nseg * ((p.K + 63) / 64), env.ncu);
    // the 8-phase kernel first (paths 3, 5 and the automatic one); the 256x256 kernel takes the rest
    if (mode == 3 || mode == 5 || (mode == 0 && env.gemm3_auto)) {
      const int rc3 = !gemm3_takes(p.M, p.N, p.K, p.nseg, nb, S, p.a_mc, p.b_mc, p.beta0, env.ncu) ? -3
                      : !pair16(p.dt_in, p.dt_out)                                                    ? -1
                                                                                                      : 0;
      if (mode == 3 && rc3 != 0) return plan_error(pl, ERR_PATH3_DECLINED, rc3);
      if (rc3 == 0) {
        pl.route = G3;
        pl.splits = S;
        return pl;
      }
    }
    if (pair16(p.dt_in, p.dt_out)) {
      pl.route = G2;
      pl.splits = S;
      return pl;
    }
  }
  if (mode == 0 && p.nb1 == 1 && p.K >= 1024 && slab_geometry(p, vec, &pl)) {
    pl.route = SLABS;
    return pl;
  }
  pl.route = G1;
  if (!pair_g1(p.dt_in, p.dt_out)) return plan_error(pl, ERR_DTYPE);
  return pl;
}

// Slab count of the weight-gradient kernel (csrc/gemm_wgrad.hip: 128x128 tiles x S slabs of K):
// rounds of 512 workgroup slots x (k-tiles per slab + a per-workgroup overhead of ~4 k-tiles) + the
// fp32 partials' write and ordered-sum read (~0.07 k-tile per tile and slab); fitted to the S sweep
// of benchmarks/micro/wgrad_splits.py.  requested > 0: that count, clamped to the k-tiles.
inline int64_t wgrad_slabs(int64_t K, int64_t M, int64_t N, int64_t requested) {
  const int64_t KT = (K + 63) / 64, tiles = (M / 128) * (N / 128);
  int64_t S = requested;
  if (S <= 0) {
    double best = 1e300;
    for (int64_t s = 1; s <= std::min<int64_t>(KT, 64); ++s) {
      const double cost = (double)((tiles * s + 511) / 512) * ((double)KT / s + 4.0) + 0.07 * (double)(tiles * s);
      if (cost < best) { best = cost; S = s; }
    }
  }
  return std::max<int64_t>(1, std::min<int64_t>(S, KT));
}

}  // namespace gp
}  // namespace xdot
