// Dumps the GEMM route planner (csrc/gemm_plan.h) over a fixed case table, one line per case:
// tests/test_gemm_plan.py compiles this with plain g++ and compares the output with
// tests/golden/gemm_plan.txt, which was recorded from the dispatch code of xdot.gemm as it stood
// before it moved into the header.  Line formats:
//   gemm M N K nseg nb1 nb2 lda ldb ldc <sA1 sA2 sB1 sB2 sC1 sC2 sAseg sBseg, or "dense" for the strides of `dense`>
//        <k|m: A, B k- or mn-contiguous> b<0: beta == 0> in out <a16 b16 c16> p<path> | ncu gemm_lib gemm3_auto free_bytes
//        -> ROUTE splits vec | SLABS Ks slabs full vec_full vec_last vec | LIBRARY K sa sb sc | error <code> <rc>
//   pick_splits tiles kt ncu -> S        wgrad_slabs K M N requested -> S
#include "gemm_plan.h"

#include <cstdio>

using namespace xdot::gp;

static double g_free = 64e9;  // the fixed free-memory answer
static double free_fixed() { return g_free; }
static const char* const ROUTES[] = {"SPLIT3", "LIBRARY", "G2_F32", "G3", "G2", "SLABS", "G1"};
static const char* const DTS[] = {"f32", "bf16", "f16"};

struct Env {
  int64_t ncu = 256;
  int lib = 0, g3 = 1;
};

static GemmProblem dense(int64_t M, int64_t N, int64_t K, DType in, DType out, bool a_mc, bool b_mc, int64_t nseg = 1,
                         int64_t nb1 = 1, int64_t nb2 = 1);

static void line(const GemmProblem& p, const Env& e = Env()) {
  const GemmEnv env{e.ncu, e.lib, e.g3, free_fixed};
  const GemmPlan pl = plan_gemm(p, env);
  std::printf("gemm %lld %lld %lld %lld %lld %lld %lld %lld %lld ", (long long)p.M, (long long)p.N, (long long)p.K,
              (long long)p.nseg, (long long)p.nb1, (long long)p.nb2, (long long)p.lda, (long long)p.ldb, (long long)p.ldc);
  const GemmProblem d = dense(p.M, p.N, p.K, p.dt_in, p.dt_out, p.a_mc, p.b_mc, p.nseg, p.nb1, p.nb2);
  if (p.sA1 == d.sA1 && p.sA2 == d.sA2 && p.sB1 == d.sB1 && p.sB2 == d.sB2 && p.sC1 == d.sC1 && p.sC2 == d.sC2 &&
      p.sAseg == d.sAseg && p.sBseg == d.sBseg)
    std::printf("dense");
  else
    std::printf("%lld %lld %lld %lld %lld %lld %lld %lld", (long long)p.sA1, (long long)p.sA2, (long long)p.sB1,
                (long long)p.sB2, (long long)p.sC1, (long long)p.sC2, (long long)p.sAseg, (long long)p.sBseg);
  std::printf(" %c%c b%d %s %s %d%d%d p%d | %lld %d %d %g -> ", p.a_mc ? 'm' : 'k', p.b_mc ? 'm' : 'k', p.beta0 ? 0 : 1,
              DTS[p.dt_in], DTS[p.dt_out], (int)p.a16, (int)p.b16, (int)p.c16, p.path, (long long)e.ncu, e.lib, e.g3, g_free);
  if (pl.error != PLAN_OK)
    std::printf("error %d %d\n", (int)pl.error, pl.rc);
  else if (pl.route == SLABS)
    std::printf("SLABS %lld %lld %lld %d %d %d\n", (long long)pl.Ks, (long long)pl.slabs, (long long)pl.full,
                (int)pl.vec_full, (int)pl.vec_last, (int)pl.vec);
  else if (pl.route == LIBRARY)
    std::printf("LIBRARY %lld %lld %lld %lld\n", (long long)pl.lib_K, (long long)pl.lib_sa, (long long)pl.lib_sb, (long long)pl.lib_sc);
  else
    std::printf("%s %lld %d\n", ROUTES[pl.route], (long long)pl.splits, (int)pl.vec);
}

// dense operands [nb1][nb2][nseg][rows][cols], dense output [nb1][nb2][M][N], aligned bases, beta = 0, path 0
static GemmProblem dense(int64_t M, int64_t N, int64_t K, DType in, DType out, bool a_mc, bool b_mc, int64_t nseg,
                         int64_t nb1, int64_t nb2) {
  GemmProblem p{};
  p.M = M; p.N = N; p.K = K; p.nseg = nseg; p.nb1 = nb1; p.nb2 = nb2;
  p.lda = a_mc ? M : K; p.ldb = b_mc ? N : K; p.ldc = N;
  p.sAseg = M * K; p.sA2 = nseg * M * K; p.sA1 = nb2 * p.sA2;
  p.sBseg = N * K; p.sB2 = nseg * N * K; p.sB1 = nb2 * p.sB2;
  p.sC2 = M * N; p.sC1 = nb2 * M * N;
  p.a_mc = a_mc; p.b_mc = b_mc; p.beta0 = true; p.dt_in = in; p.dt_out = out; p.esize = in == F32 ? 4 : 2;
  p.a16 = p.b16 = p.c16 = true; p.path = 0;
  return p;
}

struct Pair { DType in, out; };
struct S3 { int64_t v[3]; int64_t operator[](int i) const { return v[i]; } };
struct S2 { int64_t v[2]; int64_t operator[](int i) const { return v[i]; } };
static const Pair PAIRS[] = {{BF16, BF16}, {BF16, F32}, {F16, F16}, {F16, F32}, {F32, F32}, {F32, BF16}};
static const bool LAYOUTS[][2] = {{false, false}, {false, true}, {true, false}, {true, true}};

// the products of the attention workload (xdot/ops/gemm.py, xdot/ops/linear.py): T = 25000, d = 768,
// h = 8 heads of 96, world sizes 1 and 8; operands are the head-split views of (R, 768) projections
static void workload(DType dt, int path) {
  const int64_t T = 25000, D = 96, H = 8, d = 768;
  const int es = dt == F32 ? 4 : 2;
  for (int64_t W : {(int64_t)1, (int64_t)8}) {
    const int64_t R = T / W;
    GemmProblem p;
    // nt, whole shards: W = 1 per-rank form (nb1 = 1), W = 8 one GEMM over all T columns
    p = dense(R, T, D, dt, dt, false, false, 1, 1, H);
    p.path = path;
    p.lda = d; p.ldb = d; p.ldc = T; p.sA1 = 0; p.sA2 = D; p.sB1 = 0; p.sB2 = D; p.sC1 = W == 1 ? T : 0; p.sC2 = R * T;
    p.sAseg = p.sBseg = 0;
    line(p);
    const GemmProblem nt = p;
    if (W > 1) {
      // nt, two row chunks per shard: per-rank column blocks of the (P, R, T) output, the second off 16 bytes
      for (int64_t c0 : {(int64_t)0, (int64_t)1563}) {
        p = nt;
        p.N = c0 ? R - 1563 : 1563; p.nb1 = W; p.sB1 = R * d; p.sC1 = R; p.c16 = (c0 * es) % 16 == 0;
        line(p);
      }
    }
    // all: K segments = ranks, feature columns of every rank's right
    p = dense(R, D, R, dt, dt, false, true, W, 1, H);
    p.path = path;
    p.lda = T; p.ldb = d; p.ldc = d; p.sA1 = 0; p.sA2 = R * T; p.sB1 = 0; p.sB2 = D; p.sC1 = 0; p.sC2 = D;
    p.sAseg = R; p.sBseg = W > 1 ? R * d : 0;
    line(p);
    // all, row-block chunks (two per shard), overwriting then accumulating
    const GemmProblem all = p;
    const int64_t h = (R + 1) / 2;
    for (int64_t r0 : {(int64_t)0, h}) {
      p = all;
      p.K = r0 ? R - h : h; p.a16 = (r0 * es) % 16 == 0; p.beta0 = r0 == 0;
      line(p);
    }
    // tn: per-rank blocks (W = 1), else one GEMM over all T rows into the R-major / the contiguous send buffer
    p = dense(W == 1 ? R : T, D, R, dt, dt, true, true, 1, 1, H);
    p.path = path;
    p.lda = T; p.ldb = d; p.ldc = d; p.sA1 = W == 1 ? R : 0; p.sA2 = R * T; p.sB1 = 0; p.sB2 = D; p.sC1 = 0; p.sC2 = D;
    p.sAseg = p.sBseg = 0;
    line(p);
    if (W > 1) {
      p.ldc = D; p.sC2 = T * D;
      line(p);
    }
    // fp32 projections: forward (with and without bias), input gradient, weight gradient;
    // 16-bit weight gradients off the wgrad kernel (path 5), fp32 and 16-bit out
    for (int64_t Nout : {d, 3 * d}) {
      if (dt == F32) {
        p = dense(R, Nout, d, dt, dt, false, false); line(p);
        p.beta0 = false; line(p);
        p = dense(R, d, Nout, dt, dt, false, true); line(p);
        p = dense(Nout, d, R, dt, dt, true, true); line(p);
      } else {
        p = dense(Nout, d, R, dt, dt, true, true); p.path = 5; line(p);
        p.dt_out = F32; line(p);
      }
    }
  }
}

int main() {
  // ---- every dtype pair in every layout across the M / N thresholds
  const int64_t MN[][2] = {{63, 300}, {64, 300}, {127, 128}, {128, 128}, {255, 256}, {256, 256}};
  for (const Pair& pr : PAIRS)
    for (const auto& l : LAYOUTS)
      for (const auto& mn : MN)
        for (int64_t K : {(int64_t)100, (int64_t)1024})
          line(dense(mn[0], mn[1], K, pr.in, pr.out, l[0], l[1]));
  // ---- M and N on both sides of 64 / 128 / 256 where that threshold alone decides the route: the 16-bit auto
  // rule past its tile gate (512 batches), the fp32 auto rule past its long-K and its tile gate, gemm3 against
  // gemm2 (path 5, and auto past the tile gate), split fp32 (paths 4 and 6)
  for (int side = 0; side < 2; ++side)
    for (int64_t d : {(int64_t)0, (int64_t)1}) {
      auto mn = [&](int64_t edge, int64_t other, int64_t K, DType in, DType out, int path, int64_t nb2) {
        GemmProblem p = dense(side ? other : edge - 1 + d, side ? edge - 1 + d : other, K, in, out, false, false, 1, 1, nb2);
        p.path = path;
        line(p);
      };
      mn(64, 300, 64, BF16, BF16, 0, 512);
      mn(64, 300, 64, F16, F32, 0, 512);
      mn(128, 300, 4096, F32, F32, 0, 1);
      mn(128, 300, 64, F32, F32, 0, 512);
      mn(256, 300, 64, BF16, BF16, 5, 1);
      mn(256, 300, 64, F16, F32, 5, 2);
      mn(256, 300, 64, BF16, BF16, 0, 512);
      mn(256, 300, 4096, F32, F32, 4, 1);
      mn(256, 300, 16384, F32, F32, 6, 1);
    }
  // ---- forced paths, beta, the dtype pairs no kernel takes
  const Pair MORE[] = {{BF16, BF16}, {BF16, F32}, {F16, F16}, {F16, F32}, {F32, F32}, {F32, BF16}, {F32, F16}, {BF16, F16}};
  const int64_t SH[][4] = {{256, 256, 64, 1}, {256, 256, 64, 0}, {130, 130, 2000, 1}, {264, 520, 4100, 1}};  // M N K beta0
  for (int path = 0; path <= 6; ++path)
    for (const Pair& pr : MORE)
      for (int li : {0, 3}) {
        if (li == 3 && pr.in != pr.out) continue;
        for (const auto& s : SH) {
          GemmProblem p = dense(s[0], s[1], s[2], pr.in, pr.out, LAYOUTS[li][0], LAYOUTS[li][1]);
          p.path = path; p.beta0 = s[3] != 0;
          line(p);
        }
      }
  // ---- extents % 8 and % 4 (k and mn) under leading dimensions padded to 16 bytes (vec stays on), K = 0
  for (const Pair& pr : {Pair{BF16, BF16}, Pair{F32, F32}})
    for (const auto& l : LAYOUTS)
      for (int path : {0, 2, 3, 5})
        for (const S3& s : {S3{{512, 512, 2044}}, S3{{516, 512, 2048}}, S3{{512, 516, 2048}}, S3{{514, 514, 2048}}, S3{{512, 512, 2046}}, S3{{512, 512, 0}}}) {
          GemmProblem p = dense(s[0], s[1], s[2], pr.in, pr.out, l[0], l[1]);
          p.path = path;
          p.lda = (p.lda + 7) / 8 * 8;
          p.ldb = (p.ldb + 7) / 8 * 8;
          line(p);
        }
  // ---- vec off: an unaligned base, an odd leading dimension, odd batch / segment strides
  for (const Pair& pr : {Pair{BF16, BF16}, Pair{F16, F32}, Pair{F32, F32}})
    for (const auto& l : LAYOUTS)
      for (int64_t K : {(int64_t)2048})
        for (int v = 0; v < 6; ++v) {
          GemmProblem p = dense(512, 512, K, pr.in, pr.out, l[0], l[1], 2, 1, 2);
          if (v == 1) p.a16 = false;
          if (v == 2) p.b16 = false;
          if (v == 3) { p.lda += 1; p.sAseg += 512; p.sA2 += 1024; }
          if (v == 4) p.sB2 += 1;
          if (v == 5) p.sAseg += 2;
          line(p);
        }
  // ---- tiles per batch 31 / 32, total tiles 511 / 512 (16-bit auto rule, fp32 auto rule, the library's)
  for (const Pair& pr : {Pair{BF16, BF16}, Pair{F32, F32}})
    for (int lib : {0, 1, 2})
      for (int64_t K : {(int64_t)64, (int64_t)1024}) {
        Env e; e.lib = lib;
        for (int64_t M : {(int64_t)7936, (int64_t)8192}) {
          line(dense(M, 100, K, pr.in, pr.out, false, false), e);
          line(dense(M, 256, K, pr.in, pr.out, false, true), e);
        }
        for (int64_t nb : {(int64_t)511, (int64_t)512}) {
          line(dense(100, 200, K, pr.in, pr.out, false, false, 1, 1, nb), e);
          line(dense(256, 256, K, pr.in, pr.out, false, false, 1, nb, 1), e);
        }
        line(dense(512, 1792, K, pr.in, pr.out, false, false, 1, 1, 73), e);  // 7 x 73 = 511
        line(dense(512, 2048, K, pr.in, pr.out, false, false, 1, 1, 64), e);  // 8 x 64 = 512
      }
  // ---- the library route: flop on both sides of 2e10, batch forms, K segments, output layouts
  for (int lib : {0, 1, 2})
    for (int g3 : {0, 1}) {
      Env e; e.lib = lib; e.g3 = g3;
      for (int64_t K : {(int64_t)144, (int64_t)152}) line(dense(8192, 8192, K, BF16, BF16, false, false), e);
      for (int64_t K : {(int64_t)9536, (int64_t)9540}) line(dense(1024, 1024, K, F32, F32, false, true), e);
      for (const Pair& pr : {Pair{BF16, BF16}, Pair{F32, F32}, Pair{BF16, F32}}) {
        line(dense(4096, 4096, 512, pr.in, pr.out, false, false, 1, 1, 4), e);   // one level (inner)
        line(dense(4096, 4096, 512, pr.in, pr.out, true, false, 1, 4, 1), e);    // one level (outer)
        line(dense(4096, 4096, 512, pr.in, pr.out, false, true, 1, 2, 3), e);    // two levels, collapsible
        GemmProblem p = dense(4096, 4096, 512, pr.in, pr.out, false, false, 1, 2, 3);
        p.sA1 = 0;                                                               // broadcast outer: not collapsible
        line(p, e);
        line(dense(4096, 4096, 256, pr.in, pr.out, false, false, 3, 1, 2), e);   // scattered K segments
        p = dense(4096, 4096, 256, pr.in, pr.out, false, true, 3, 1, 2);         // merged K segments
        p.lda = 768; p.sAseg = 256; p.sA2 = 4096 * 768; p.sBseg = 256 * 4096;
        line(p, e);
        p = dense(4096, 4096, 512, pr.in, pr.out, false, false, 1, 1, 4);        // column-slice output
        p.ldc = 8192; p.sC2 = 4096 * 8192;
        line(p, e);
        p.ldc = 4096; p.sC2 = 4096;                                              // batches interleaved in one output row
        line(p, e);
        p = dense(4096, 4096, 512, pr.in, pr.out, false, false, 1, 1, 4);
        p.c16 = false;
        line(p, e);
        p = dense(4096, 4096, 512, pr.in, pr.out, false, false, 1, 1, 4);
        p.beta0 = false;
        line(p, e);
      }
    }
  // ---- batch and segment shapes
  const int64_t NBS[][2] = {{1, 1}, {1, 8}, {8, 1}, {2, 3}};
  for (const Pair& pr : {Pair{BF16, BF16}, Pair{F16, F32}, Pair{F32, F32}})
    for (int64_t nseg : {(int64_t)1, (int64_t)3, (int64_t)8})
      for (const auto& nb : NBS)
        for (const S3& s : {S3{{512, 512, 512}}, S3{{300, 200, 2048}}, S3{{130, 96, 1500}}})
          for (int li : {1, 3})
            line(dense(s[0], s[1], s[2], pr.in, pr.out, LAYOUTS[li][0], LAYOUTS[li][1], nseg, nb[0], nb[1]));
  // ---- K x nseg on both sides of 4096 (the exact-fp32 256x256 kernel's long-K rule), one and three segments
  for (const auto& l : LAYOUTS)
    for (int64_t nseg : {(int64_t)1, (int64_t)3})
      for (int64_t K : {(int64_t)4092 / nseg, (int64_t)4092 / nseg + 4})
        for (bool beta0 : {true, false}) {
          GemmProblem p = dense(300, 200, K, F32, F32, l[0], l[1], nseg, 1, 2);
          p.beta0 = beta0;
          line(p);
        }
  // ---- K slabs: 383 / 384 tiles, K on both sides of 1024, both slab geometries and their vec bits
  for (const Pair& pr : {Pair{F32, F32}, Pair{BF16, F32}, Pair{F32, F16}})
    for (const auto& l : LAYOUTS) {
      for (int64_t nb2 : {(int64_t)383, (int64_t)384})
        for (int64_t K : {(int64_t)1023, (int64_t)1025}) line(dense(100, 100, K, pr.in, pr.out, l[0], l[1], 1, 1, nb2));
      for (int64_t K : {(int64_t)1028, (int64_t)2000, (int64_t)5001}) {
        GemmProblem p = dense(130, 130, K, pr.in, pr.out, l[0], l[1]);
        line(p);
        if (l[0]) p.lda = 136;
        if (l[1]) p.ldb = 132;
        p.a16 = false;
        line(p);
        line(dense(1562, 768, K + 2, pr.in, pr.out, l[0], l[1], 1, 1, 2));
        p = dense(300, 200, K, pr.in, pr.out, l[0], l[1], 1, 2, 1);  // an outer batch level keeps off the slabs
        line(p);
      }
    }
  // ---- split fp32: the flop gates, the cost comparison, copy bytes / free memory, batch and item limits
  for (int path : {4, 6})
    for (int g3 : {0, 1}) {
      Env e; e.g3 = g3;
      for (const auto& l : LAYOUTS) {
        for (int64_t K : {(int64_t)992, (int64_t)1000, (int64_t)1004})
          for (bool beta0 : {true, false}) {
            GemmProblem p = dense(1000, 1000, K, F32, F32, l[0], l[1]);
            p.path = path; p.beta0 = beta0;
            line(p, e);
          }
        for (const S3& s : {S3{{256, 256, 4104}}, S3{{255, 256, 4096}}, S3{{768, 768, 25000}}, S3{{25000, 96, 25000}}, S3{{25000, 25000, 96}}, S3{{4096, 4096, 4096}}, S3{{520, 776, 200}}}) {
          GemmProblem p = dense(s[0], s[1], s[2], F32, F32, l[0], l[1]);
          p.path = path;
          line(p, e);
        }
      }
      for (const Pair& pr : {Pair{F32, BF16}, Pair{BF16, BF16}}) {
        GemmProblem p = dense(1024, 1024, 2048, pr.in, pr.out, false, false);
        p.path = path;
        line(p, e);
      }
      for (double fr : {-1.0, 3.9e9, 4.0e9, 4.1e9}) {
        g_free = fr;
        for (int64_t K : {(int64_t)20344, (int64_t)20352}) {  // 6 B x K x (M + N): 0.99995e9 and 1.00034e9
          GemmProblem p = dense(4096, 4096, K, F32, F32, false, false);
          p.path = path;
          line(p, e);
        }
      }
      g_free = 64e9;
      for (int64_t nb : {(int64_t)21845, (int64_t)21846}) {  // 3 x nseg x batches <= 65535
        GemmProblem p = dense(256, 256, 64, F32, F32, false, false, 1, 1, nb);
        p.path = path;
        line(p, e);
      }
      for (int64_t M : {(int64_t)1024, (int64_t)1280})  // 16 / 25 tiles x 21845 batches: gemm3's MAX_ITEMS x CUs = 524288
        for (int64_t ncu : {(int64_t)256, (int64_t)304}) {
          GemmProblem p = dense(M, M, 64, F32, F32, false, false, 1, 1, 21845);
          p.path = path; e.ncu = ncu;
          line(p, e);
          e.ncu = 256;
        }
    }
  // ---- gemm3's item bound on the 16-bit route (9 tiles x 65535 batches > 2048 x 256 CUs), its K-tile rule
  for (int path : {0, 3, 5})
    for (int64_t ncu : {(int64_t)256, (int64_t)304, (int64_t)64}) {
      Env e; e.ncu = ncu;
      for (int64_t M : {(int64_t)512, (int64_t)768}) {
        GemmProblem p = dense(M, M, 64, BF16, BF16, false, false, 1, 1, 65535);
        p.path = path;
        line(p, e);
      }
      GemmProblem p = dense(256, 256, 4104, BF16, BF16, false, false);
      p.path = path;
      line(p, e);
      p = dense(768, 768, 3125, BF16, F32, true, true);
      p.path = path;
      line(p, e);
    }
  // ---- the environment knobs over the plain shapes, and the CU count
  for (int lib : {0, 1, 2})
    for (int g3 : {0, 1})
      for (int64_t ncu : {(int64_t)256, (int64_t)304, (int64_t)64}) {
        if (ncu != 256 && (lib != 0 || g3 != 1)) continue;
        Env e; e.lib = lib; e.g3 = g3; e.ncu = ncu;
        for (const Pair& pr : {Pair{BF16, BF16}, Pair{F32, F32}})
          for (int path : {0, 6})
            for (const S3& s : {S3{{768, 768, 25000}}, S3{{1024, 1024, 2048}}, S3{{8192, 8192, 1024}}, S3{{300, 200, 4096}}}) {
              GemmProblem p = dense(s[0], s[1], s[2], pr.in, pr.out, s[2] > 20000, s[2] > 20000);
              p.path = path;
              line(p, e);
            }
      }
  // ---- the workload's own products
  workload(BF16, 0);
  workload(F32, 0);
  workload(F32, 6);
  // ---- the cases the GPU tests run (tests/test_gemm_plan_gpu.py, tests/test_gemm_f32_gpu.py)
  {
    GemmProblem p = dense(130, 130, 2000, F32, F32, true, true);
    line(p);
    p = dense(130, 130, 2004, BF16, F32, false, false);
    line(p);
  }
  // ---- the split-K picker and the weight-gradient slab model on their own
  for (int64_t tiles : {(int64_t)1, (int64_t)9, (int64_t)54, (int64_t)256, (int64_t)257, (int64_t)1000})
    for (int64_t kt : {(int64_t)7, (int64_t)8, (int64_t)49, (int64_t)391, (int64_t)1173})
      for (int64_t ncu : {(int64_t)256, (int64_t)304, (int64_t)64})
        std::printf("pick_splits %lld %lld %lld -> %lld\n", (long long)tiles, (long long)kt, (long long)ncu,
                    (long long)pick_splits(tiles, kt, ncu));
  for (int64_t K : {(int64_t)1, (int64_t)64, (int64_t)1562, (int64_t)3125, (int64_t)25000, (int64_t)200000})
    for (const S2& mn : {S2{{128, 128}}, S2{{768, 768}}, S2{{2304, 768}}, S2{{8192, 8192}}})
      for (int64_t req : {(int64_t)0, (int64_t)7, (int64_t)100})
        std::printf("wgrad_slabs %lld %lld %lld %lld -> %lld\n", (long long)K, (long long)mn[0], (long long)mn[1], (long long)req,
                    (long long)wgrad_slabs(K, mn[0], mn[1], req));
  return 0;
}
