// xdot — device code of the fp32-on-the-bf16-pipe flash families, templated on the split count NS:
//   NS = 2  x = hi + lo,     3 MFMAs per product ("split",  fp32_mode 1; instantiated in flash_x3.hip)
//   NS = 3  x = h + m + l,   6 MFMAs per product ("split3", fp32_mode 2; instantiated in flash_x6.hip)
// The part p of x is bf16 of what the parts before it left over (the subtractions are exact in
// fp32), so three parts carry all 24 mantissa bits.  A product keeps the terms a_i·b_j with
// i + j <= NS - 1 (part i is ~2^-9i of x): NS = 2 drops lo·lo (~2^-16 |a·b|), NS = 3 drops m·l,
// l·m and l·l (<= 2^-25), far below the rounding of the fp32 accumulation.  One image plane per
// part in LDS, one register array per part for the resident fragments, P / dS split in registers.
#pragma once
#include "flash_launch.h"

namespace xdot {
namespace fa3 {

using fa::BwdArgs;
using fa::FwdArgs;
using fa::LN2;
using fa::LOG2E;
using fa::pair_max;
using fa::pair_sum;
using fa::tidx;
using fa::flag_at;
using fa::blk_store_lds;
using fa::blk_load;

typedef __attribute__((ext_vector_type(2))) __bf16 bf2;

__device__ __forceinline__ f32x16 mm(const u32x4& a, const u32x4& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// a·b of one 16-deep K step from split operands (parts 0 = hi .. NS - 1), small terms first:
// mm3 = lo·hi, hi·lo, hi·hi;  mm6 = l·h, h·l, m·m, m·h, h·m, h·h
__device__ __forceinline__ f32x16 mm3(const u32x4 (&a)[2], const u32x4 (&b)[2], f32x16 c) {
  c = mm(a[1], b[0], c);
  c = mm(a[0], b[1], c);
  return mm(a[0], b[0], c);
}
__device__ __forceinline__ f32x16 mm6(const u32x4 (&a)[3], const u32x4 (&b)[3], f32x16 c) {
  c = mm(a[2], b[0], c);
  c = mm(a[0], b[2], c);
  c = mm(a[1], b[1], c);
  c = mm(a[1], b[0], c);
  c = mm(a[0], b[1], c);
  return mm(a[0], b[0], c);
}
__device__ __forceinline__ f32x16 mmn(const u32x4 (&a)[2], const u32x4 (&b)[2], const f32x16& c) { return mm3(a, b, c); }
__device__ __forceinline__ f32x16 mmn(const u32x4 (&a)[3], const u32x4 (&b)[3], const f32x16& c) { return mm6(a, b, c); }
__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }

// two floats -> NS packed pairs: part i = bf16 of the residual the parts before it leave (the
// residuals x - h, x - h - m are exact in fp32)
template <int NS>
__device__ __forceinline__ void split_n(float x, float y, uint32_t (&p)[NS]) {
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const bf2 h = {(__bf16)x, (__bf16)y};
    p[i] = __builtin_bit_cast(uint32_t, h);
    if (i + 1 < NS) {
      x -= __builtin_bit_cast(float, p[i] << 16);
      y -= __builtin_bit_cast(float, p[i] & 0xffff0000u);
    }
  }
}
// eight floats -> one operand fragment per part
template <int NS>
__device__ __forceinline__ void split8(const float* x, u32x4 (&f)[NS]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    uint32_t p[NS];
    split_n<NS>(x[2 * t], x[2 * t + 1], p);
#pragma unroll
    for (int i = 0; i < NS; ++i) f[i][t] = p[i];
  }
}

template <int D> struct Cfg {
  static constexpr int ROW = fa::Img<D>::ROW;  // image row stride (bytes): the bf16 kernels' layout
  static constexpr int KS = D / 16;            // 16-deep K steps over the head dim
  static constexpr int DB = D / 32;            // 32-wide output blocks
  static constexpr int NC = D / 32;            // f32x4 per thread per 32-row fp32 tile (256 threads)
};

// One staged 32-row tile: NS bf16 image planes (hi, lo / h, m, l), row-major in the bf16 kernels' swizzled
// layout (fa::Img / fa::img_off: rows of ROW bytes, 16-byte chunks XOR (row >> 2) & 3).  Products
// over the head dim read it with ds_read_b128 (fa::row_frag), products over the tile index with
// the hardware transpose ds_read_b64_tr_b16 (fa::tr_frag), whose key order (k0 + 8 (j >> 2) + 4h
// + (j & 3)) is the accumulator-register order the B operands come in: one image serves both
// (the flags say which reads a kernel makes; the layout is the same).
template <int D, bool RMF, bool TRF, int NS = 2> struct Img {
  static constexpr int PLANE = 32 * Cfg<D>::ROW;  // part i at i * PLANE
  static constexpr int BYTES = (RMF || TRF) ? NS * PLANE : 0;
};

// one 32-row fp32 tile global -> registers (rows row0.., clamped to row0 + rmax) -> split images
template <int D> struct Tile {
  using CF = Cfg<D>;
  f32x4 r[CF::NC];
  __device__ __forceinline__ void load(const float* base, int64_t ld, int64_t row0, int rmax, int tid) {
#pragma unroll
    for (int i = 0; i < CF::NC; ++i) {
      const int q = tid + 256 * i, row = q / (D / 4), c = q % (D / 4);
      r[i] = *reinterpret_cast<const f32x4*>(base + (row0 + min(row, rmax)) * ld + 4 * c);
    }
  }
  template <bool RMF, bool TRF, int NS>
  __device__ __forceinline__ void store(char* img, int tid) const {
    using IL = Img<D, RMF, TRF, NS>;
#pragma unroll
    for (int i = 0; i < CF::NC; ++i) {
      const int q = tid + 256 * i, row = q / (D / 4), c = q % (D / 4);
      uint32_t p0[NS], p1[NS];
      split_n<NS>(r[i][0], r[i][1], p0);
      split_n<NS>(r[i][2], r[i][3], p1);
      const int o = fa::img_off<D>(row, c >> 1) + 8 * (c & 1);  // 4 bf16 = half a 16-byte chunk
#pragma unroll
      for (int s = 0; s < NS; ++s) *reinterpret_cast<u32x2*>(img + s * IL::PLANE + o) = u32x2{p0[s], p1[s]};
    }
  }
};

// register-resident split fragments of one 32-row block (B operand of row products):
// f[m][part] = X[row][16m + 8h .. +7]; p points at X[row][8h]
template <int D, int NS>
__device__ __forceinline__ void load_frag(u32x4 (&f)[D / 16][NS], const float* p, bool ok) {
#pragma unroll
  for (int m = 0; m < D / 16; ++m) {
    float x[8];
    const f32x4 a = ok ? *reinterpret_cast<const f32x4*>(p + 16 * m) : f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 b = ok ? *reinterpret_cast<const f32x4*>(p + 16 * m + 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      x[t] = a[t];
      x[4 + t] = b[t];
    }
    split8<NS>(x, f[m]);
  }
}

// acc[c][j] += Σ_d img[c][d] · frag[j][d]  (c = tile row: register, j = frag row: lane)
template <int D, bool RMF, bool TRF, int NS>
__device__ __forceinline__ f32x16 rowprod(const char* img, const u32x4 (&f)[D / 16][NS], f32x16 acc, int lane) {
  using IL = Img<D, RMF, TRF, NS>;
  const fa::Lanes Ln = fa::make_lanes<D>(lane);
  // NS = 3: the five small terms of every K step go into an accumulator of their own (~2^-9 of the
  // product, so its roundings are), h·h alone into `acc`: D / 16 roundings at the product's magnitude
  // instead of 6 D / 16.  Measured on scores of +-100: with one accumulator the error was 1.4..2.0x the
  // exact family's (profiles/split3.md).
  f32x16 small{};
#pragma unroll
  for (int m = 0; m < D / 16; ++m) {
    u32x4 a[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) a[s] = fa::row_frag<D>(img + s * IL::PLANE, 0, m, Ln);
    if constexpr (NS == 3) {
      small = mm(a[2], f[m][0], small);
      small = mm(a[0], f[m][2], small);
      small = mm(a[1], f[m][1], small);
      small = mm(a[1], f[m][0], small);
      small = mm(a[0], f[m][1], small);
      acc = mm(a[0], f[m][0], acc);
    } else {
      acc = mmn(a, f[m], acc);
    }
  }
  if constexpr (NS == 3) acc += small;
  return acc;
}

// out[db][d][j] += Σ_c img[c][d] · x[c][j]  (x: an accumulator tile, c its register rows)
template <int D, bool RMF, bool TRF, int NS>
__device__ __forceinline__ void trprod(const char* img, const f32x16& x, f32x16 (&out)[D / 32], int lane) {
  using IL = Img<D, RMF, TRF, NS>;
  u32x4 b[2][NS];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    float v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = x[8 * j + t];
    split8<NS>(v, b[j]);
  }
  const fa::Lanes Ln = fa::make_lanes<D>(lane);
#pragma unroll
  for (int db = 0; db < D / 32; ++db)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      u32x4 a[NS];
#pragma unroll
      for (int s = 0; s < NS; ++s) a[s] = fa::tr_frag<D>(img + s * IL::PLANE, 16 * j, 32 * db, Ln);
      out[db] = mmn(a, b[j], out[db]);
    }
}


// ------------------------------------------------------------------------------------------
// forward: 4 waves x 32 rows of one (b, h); sweeps 32-column tiles of its column split
template <int D, int NS = 2> struct FwdL {
  using Q = Img<D, true, false, NS>;
  using V = Img<D, false, true, NS>;
  static constexpr int STAGE = Q::BYTES + V::BYTES;
  static constexpr int LDS = 2 * STAGE;
  static constexpr int LDS_SB = LDS + 4 * 4096;  // + a 4-KiB transpose tile per wave (blk_store_lds)
};

// SS: store the raw scores into a.sbuf (score-buffer mode, same block format as flash_f32.hip)
// NS = 3: three planes per image, two stages = 72 KiB at D <= 96 (two workgroups per CU), 120 KiB at
// D = 128 (one)
template <int D, bool SS, int NS = 2>
__global__ __launch_bounds__(256, NS == 2 || D <= 96 ? 2 : 1) void fwd_kernel(FwdArgs a) {
  static_assert(NS == 2 || !SS, "split3 keeps no S buffer");
  using CF = Cfg<D>;
  using FL = FwdL<D, NS>;
  constexpr int DB = CF::DB;
  using fa::smem;
  const int tid = threadIdx.x, lane = tid & 63, hf = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nrb = (a.R + 127) / 128;
  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  const int rb = lin % nrb, bhs = lin / nrb;
  const int bh = bhs % (a.B * a.H), sp = bhs / (a.B * a.H);
  const int b = bh / a.H, h = bh % a.H;
  const int C = a.H * D;
  const int NKT64 = (a.T + 63) / 64, NKT32 = (a.T + 31) / 32;
  const int kt_beg = 2 * (int)((int64_t)sp * NKT64 / a.nsplit);
  const int kt_end = min(NKT32, 2 * (int)((int64_t)(sp + 1) * NKT64 / a.nsplit));
  const int r0 = rb * 128 + wave * 32, row = r0 + (lane & 31);
  const bool row_ok = row < a.R;
  const int NKT4 = (NKT64 + 3) & ~3, NRB32 = (a.R + 31) / 32;

  u32x4 kf[CF::KS][NS];
  load_frag<D, NS>(kf, reinterpret_cast<const float*>(a.rows) + ((int64_t)b * a.R + (row_ok ? row : 0)) * C + h * D + 8 * hf,
               row_ok);
  const float* qb = reinterpret_cast<const float*>(a.kc) + (int64_t)b * a.T * a.ldkv + h * D;
  const float* vb = reinterpret_cast<const float*>(a.vc) + (int64_t)b * a.T * a.ldkv + h * D;
  const float c2 = a.scale * LOG2E, NEG_INF = -__builtin_inff();
  float m_run = NEG_INF, l_run = 0.f;
  f32x16 o[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i) o[i] = f32x16{};
  // score buffer: this wave's row of 32x32 blocks (r0 < R: waves past R never store)
  // (waves past R write the dump block: uniform store counts keep the compiler's vmcnt waits exact)
  float* sbw = SS ? a.sbuf + (r0 < a.R ? ((int64_t)bh * NRB32 + (r0 >> 5)) * NKT32 * 1024 : fa::sb_dump(a.B, a.H, a.R, a.T))
                  : nullptr;
  const int sbw_step = r0 < a.R ? 1024 : 0;

  Tile<D> tq, tv;
  if (kt_beg < kt_end) {
    tq.load(qb, a.ldkv, (int64_t)kt_beg * 32, a.T - 1 - kt_beg * 32, tid);
    tv.load(vb, a.ldkv, (int64_t)kt_beg * 32, a.T - 1 - kt_beg * 32, tid);
    tq.template store<true, false, NS>(smem, tid);
    tv.template store<false, true, NS>(smem + FL::Q::BYTES, tid);
    __syncthreads();
  }
  for (int kt = kt_beg; kt < kt_end; ++kt) {
    const bool more = kt + 1 < kt_end;
    if (more) {
      tq.load(qb, a.ldkv, (int64_t)(kt + 1) * 32, a.T - 1 - (kt + 1) * 32, tid);
      tv.load(vb, a.ldkv, (int64_t)(kt + 1) * 32, a.T - 1 - (kt + 1) * 32, tid);
    }
    const char* qi = smem + ((kt - kt_beg) & 1) * FL::STAGE;
    const char* vi = qi + FL::Q::BYTES;
    int flag = r0 >= a.R ? 1 : (a.mflags ? flag_at(a.mflags, b, NRB32, NKT4, r0 >> 5, kt >> 1) : 0);
    flag = __builtin_amdgcn_readfirstlane(flag);
    f32x16 s{};
    if (flag != 1) s = rowprod<D, true, false, NS>(qi, kf, f32x16{}, lane);  // Sᵀ: col (register) x row (lane)
    // raw S, every tile (skipped tiles store zeros nobody reads): LDS writes here, the transposed
    // global stores after the PV product
    float* swl = reinterpret_cast<float*>(smem + FL::LDS) + wave * 1024;
    if constexpr (SS) fa::blk_put_lds(swl, s, lane);
    if (flag != 1) {
      const int valid = a.T - kt * 32;
      if (flag == 2 || valid < 32) {
        uint32_t w = 0;
        if (flag == 2 && row_ok) w = fa::settle((uint32_t)(a.mbits[((int64_t)b * NKT64 + (kt >> 1)) * a.R + row] >> (32 * (kt & 1))));
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = tidx(r, hf);
          if (((w >> c) & 1u) || c >= valid) s[r] = NEG_INF;
        }
      }
      float mx = NEG_INF;
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[r]);
      mx = pair_max(mx) * c2;
      const float m_new = fmaxf(m_run, mx);
      if (m_new > m_run) {
        const float alpha = ex2(m_run - m_new);  // m_run = -inf: 0
        l_run *= alpha;
#pragma unroll
        for (int i = 0; i < DB; ++i) o[i] *= alpha;
        m_run = m_new;
      }
      const float m_use = m_run == NEG_INF ? 0.f : m_run;
      float ls = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[r] = ex2(__builtin_fmaf(s[r], c2, -m_use));
        ls += s[r];
      }
      l_run += ls;
      trprod<D, false, true, NS>(vi, s, o, lane);  // Oᵀ += Vᵀ · Pᵀ
    }
    if constexpr (SS) fa::blk_flush_lds(sbw + kt * sbw_step, swl, lane);
    if (more) {
      char* nx = smem + ((kt + 1 - kt_beg) & 1) * FL::STAGE;
      tq.template store<true, false, NS>(nx, tid);
      tv.template store<false, true, NS>(nx + FL::Q::BYTES, tid);
    }
    __syncthreads();
  }

  const float l_tot = pair_sum(l_run);
  const float inv = 1.f / l_tot;
  if (!row_ok) return;
  const float lse = (m_run + __log2f(l_tot)) * LN2;
  float* op;
  if (a.nsplit == 1 && !a.force_partial) {
    op = reinterpret_cast<float*>(a.out) + ((int64_t)b * a.R + row) * C + h * D;
    if (hf == 0) a.lse[((int64_t)b * a.H + h) * a.R + row] = lse;
  } else {
    op = a.opart + (((int64_t)(a.sp0 + sp) * a.B + b) * a.R + row) * C + h * D;
    if (hf == 0) a.lpart[(((int64_t)(a.sp0 + sp) * a.B + b) * a.H + h) * a.R + row] = lse;
  }
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<f32x4*>(op + db * 32 + 8 * g + 4 * hf) =
          f32x4{o[db][4 * g] * inv, o[db][4 * g + 1] * inv, o[db][4 * g + 2] * inv, o[db][4 * g + 3] * inv};
}

// ------------------------------------------------------------------------------------------
// backward, row side: dK = scale · Σ_cols dS · Q_cols.  4 waves x 32 rows, column split.
// Two LDS stages (the next tile is stored while the current one is read: one barrier per tile).
template <int D, int NS = 2> struct RowsL {
  using Q = Img<D, true, true, NS>;
  using V = Img<D, true, false, NS>;
  static constexpr int STAGE = Q::BYTES + V::BYTES;
  static constexpr int LDS = 2 * STAGE;
};

// (NS = 3 at D = 64: the k and dO fragments are 96 VGPRs beside 32 of dK; 256 registers spill)
template <int D, int NS = 2>
__global__ __launch_bounds__(256, D <= (NS == 2 ? 64 : 32) ? 2 : 1) void bwd_rows_kernel(BwdArgs a) {
  using CF = Cfg<D>;
  using RL = RowsL<D, NS>;
  constexpr int DB = CF::DB;
  using fa::smem;
  const int tid = threadIdx.x, lane = tid & 63, hf = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nrb = (a.R + 127) / 128;
  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  const int rb = lin % nrb, bhs = lin / nrb;
  const int bh = bhs % (a.B * a.H), sp = bhs / (a.B * a.H);
  const int b = bh / a.H, h = bh % a.H;
  const int C = a.H * D;
  const int NKT64 = (a.T + 63) / 64, NKT32 = (a.T + 31) / 32;
  const int kt_beg = 2 * (int)((int64_t)sp * NKT64 / a.nsplit);
  const int kt_end = min(NKT32, 2 * (int)((int64_t)(sp + 1) * NKT64 / a.nsplit));
  const int r0 = rb * 128 + wave * 32, row = r0 + (lane & 31);
  const bool row_ok = row < a.R;
  const int NKT4 = (NKT64 + 3) & ~3, NRB32 = (a.R + 31) / 32;

  u32x4 kf[CF::KS][NS], df[CF::KS][NS];
  {
    const int64_t off = ((int64_t)b * a.R + (row_ok ? row : 0)) * C + h * D + 8 * hf;
    load_frag<D, NS>(kf, reinterpret_cast<const float*>(a.rows) + off, row_ok);
    load_frag<D, NS>(df, reinterpret_cast<const float*>(a.dout) + off, row_ok);
  }
  const int64_t li = ((int64_t)b * a.H + h) * a.R + (row_ok ? row : 0);
  const float lse2 = row_ok ? a.lse[li] * LOG2E : 0.f, dlt = row_ok ? a.delta[li] : 0.f;
  const float* qb = reinterpret_cast<const float*>(a.kc) + (int64_t)b * a.T * a.ldkv + h * D;
  const float* vb = reinterpret_cast<const float*>(a.vc) + (int64_t)b * a.T * a.ldkv + h * D;
  const float c2 = a.scale * LOG2E, NEG_INF = -__builtin_inff();
  f32x16 dk[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i) dk[i] = f32x16{};
  fa::pin_agpr(dk);  // loop-carried: AGPR-resident, no per-product copies

  Tile<D> tq, tv;
  if (kt_beg < kt_end) {
    tq.load(qb, a.ldkv, (int64_t)kt_beg * 32, a.T - 1 - kt_beg * 32, tid);
    tv.load(vb, a.ldkv, (int64_t)kt_beg * 32, a.T - 1 - kt_beg * 32, tid);
    tq.template store<true, true, NS>(smem, tid);
    tv.template store<true, false, NS>(smem + RL::Q::BYTES, tid);
    __syncthreads();
  }
  for (int kt = kt_beg; kt < kt_end; ++kt) {
    const bool more = kt + 1 < kt_end;
    if (more) {
      tq.load(qb, a.ldkv, (int64_t)(kt + 1) * 32, a.T - 1 - (kt + 1) * 32, tid);
      tv.load(vb, a.ldkv, (int64_t)(kt + 1) * 32, a.T - 1 - (kt + 1) * 32, tid);
    }
    const char* qi = smem + ((kt - kt_beg) & 1) * RL::STAGE;
    const char* vi = qi + RL::Q::BYTES;
    int flag = r0 >= a.R ? 1 : (a.mflags ? flag_at(a.mflags, b, NRB32, NKT4, r0 >> 5, kt >> 1) : 0);
    flag = __builtin_amdgcn_readfirstlane(flag);
    if (flag != 1) {
      f32x16 s = rowprod<D, true, true, NS>(qi, kf, f32x16{}, lane);    // Sᵀ  (col x row)
      f32x16 dp = rowprod<D, true, false, NS>(vi, df, f32x16{}, lane);  // dPᵀ (col x row)
      const int valid = a.T - kt * 32;
      uint32_t w = 0;
      const bool chk = flag == 2 || valid < 32;
      if (flag == 2 && row_ok) w = fa::settle((uint32_t)(a.mbits[((int64_t)b * NKT64 + (kt >> 1)) * a.R + row] >> (32 * (kt & 1))));
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float x = __builtin_fmaf(s[r], c2, -lse2);
        if (chk) {
          const int c = tidx(r, hf);
          if (((w >> c) & 1u) || c >= valid) x = NEG_INF;
        }
        s[r] = ex2(x) * (dp[r] - dlt);  // dSᵀ / scale
      }
      trprod<D, true, true, NS>(qi, s, dk, lane);  // dKᵀ += Q_colsᵀ · dSᵀ
      fa::pin_agpr(dk);
    }
    if (more) {
      char* nx = smem + ((kt + 1 - kt_beg) & 1) * RL::STAGE;
      tq.template store<true, true, NS>(nx, tid);
      tv.template store<true, false, NS>(nx + RL::Q::BYTES, tid);
    }
    __syncthreads();
  }
  if (!row_ok) return;
  float* op = (a.nsplit > 1 || a.force_partial) ? a.dpart + (((int64_t)(a.sp0 + sp) * a.B + b) * a.R + row) * C + h * D
                                                : reinterpret_cast<float*>(a.drows) + ((int64_t)b * a.R + row) * C + h * D;
  const float sc = a.scale;
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<f32x4*>(op + db * 32 + 8 * g + 4 * hf) =
          f32x4{dk[db][4 * g] * sc, dk[db][4 * g + 1] * sc, dk[db][4 * g + 2] * sc, dk[db][4 * g + 3] * sc};
}

// ------------------------------------------------------------------------------------------
// backward, gathered side: dQ_cols = scale · Σ_rows dSᵀ · K_rows, dV_cols = Σ_rows Pᵀ · dO.
// 4 waves x 32 columns of one (b, h); sweeps 32-row tiles of K_rows / dO + their lse2 / δ.
// LS (score-buffer mode): S comes from a.sbuf (prefetched one tile ahead) instead of the K·Qᵀ
// product, each block is overwritten with dS / scale for bwd_rows_ds_kernel, and dV is left to
// bwd_cols_dv_kernel (run first).  K then needs only its transposed image, dO its row-major one.
// DS (dS-only buffer mode, recompute kernel): S recomputed as without a buffer, dS stored into
// a.dsbuf for bwd_rows_ds_kernel (40 GB of score traffic per step instead of the 100 GB of the
// S + dS mode, which bounds this family's kernels)
// NS = 3 (never LS): the resident q and v fragments are 2 x 3 x D/16 x 4 VGPRs (D = 128: 192) beside
// 2 x D/32 x 16 pinned accumulator AGPRs: one workgroup per CU, 512 registers per lane
template <int D, bool LS, bool DS = LS, int NS = 2> struct ColsL {
  using K = Img<D, !LS, true, NS>;
  using DO = Img<D, true, !LS, NS>;
  static constexpr int AUX = 256;  // lse2[32], δ[32] (fp32)
  static constexpr int STAGE = K::BYTES + DO::BYTES + AUX;
  static constexpr int LDS = 2 * STAGE + (DS ? 4 * 4096 : 0);
};

template <int D, bool LS, bool DS = LS, int NS = 2>
__global__ __launch_bounds__(256, LS && D <= 96 ? 2 : 1) void bwd_cols_kernel(BwdArgs a) {
  static_assert(NS == 2 || !LS, "split3 keeps no S buffer");
  using CF = Cfg<D>;
  using KL = ColsL<D, LS, DS, NS>;
  constexpr int DB = CF::DB;
  using fa::smem;
  const int tid = threadIdx.x, lane = tid & 63, hf = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ncb = (a.T + 127) / 128;
  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  const int cb = lin % ncb, bhs = lin / ncb;
  const int bh = bhs % (a.B * a.H), sp = bhs / (a.B * a.H), ns = a.csq > 1 ? a.csq : 1;
  const int b = bh / a.H, h = bh % a.H;
  const int C = a.H * D;
  const int c0 = cb * 128 + wave * 32, col = c0 + (lane & 31);
  const bool col_ok = col < a.T;
  const int NKT64 = (a.T + 63) / 64, NKT4 = (NKT64 + 3) & ~3, NRB32 = (a.R + 31) / 32;
  const int NRT64 = (a.R + 63) / 64, TPAD = (a.T + 127) / 128 * 128;
  const int NRT = (a.R + 31) / 32;
  // row split sp of ns (BwdArgs::csq): row tiles [rt_beg, rt_end)
  const int rt_beg = (int)((int64_t)sp * NRT / ns), rt_end = (int)((int64_t)(sp + 1) * NRT / ns);

  constexpr int QS = LS ? 1 : CF::KS;
  u32x4 qf[QS][NS], vf[CF::KS][NS];
  {
    const int64_t off = ((int64_t)b * a.T + (col_ok ? col : 0)) * a.ldkv + h * D + 8 * hf;
    if constexpr (!LS) load_frag<D, NS>(qf, reinterpret_cast<const float*>(a.kc) + off, col_ok);
    load_frag<D, NS>(vf, reinterpret_cast<const float*>(a.vc) + off, col_ok);
  }
  const int NKT32 = (a.T + 31) / 32;
  const bool sown = DS && c0 < a.T;
  // every wave loads and stores every tile (waves past T: a valid block / the dump block)
  float* sbc = LS ? a.sbuf + ((int64_t)bh * NRB32 * NKT32 + min(c0 >> 5, NKT32 - 1)) * 1024 : nullptr;
  float* dsc = DS ? (a.dsbuf ? a.dsbuf : a.sbuf) +
                        (sown ? ((int64_t)bh * NRB32 * NKT32 + (c0 >> 5)) * 1024 : fa::sb_dump(a.B, a.H, a.R, a.T))
                  : nullptr;
  const int64_t dstep = sown ? (int64_t)NKT32 * 1024 : 0;
  const int64_t sstep = (int64_t)NKT32 * 1024;
  f32x16 snext{};
  if (LS && rt_beg < rt_end) snext = blk_load(sbc + rt_beg * sstep, lane);
  const float* kb = reinterpret_cast<const float*>(a.rows) + (int64_t)b * a.R * C + h * D;
  const float* db_ = reinterpret_cast<const float*>(a.dout) + (int64_t)b * a.R * C + h * D;
  const float* lse2 = a.lse2 + ((int64_t)b * a.H + h) * a.R;
  const float* dlt = a.delta + ((int64_t)b * a.H + h) * a.R;
  const float c2 = a.scale * LOG2E, NEG_INF = -__builtin_inff();
  f32x16 dq[DB], dv[LS ? 1 : DB];
#pragma unroll
  for (int i = 0; i < DB; ++i) dq[i] = f32x16{};
  if constexpr (!LS) {
#pragma unroll
    for (int i = 0; i < DB; ++i) dv[i] = f32x16{};
    fa::pin_agpr(dq);  // loop-carried: AGPR-resident, no per-product copies
    fa::pin_agpr(dv);
  }

  // row constants of a tile: lse2 (+inf past R: P = 0) and δ, by threads 0..63
  auto aux_load = [&](int rt) -> float {
    const int rr = rt * 32 + (tid & 31);
    if (tid < 32) return rr < a.R ? lse2[rr] : __builtin_inff();
    if (tid < 64) return rr < a.R ? dlt[rr] : 0.f;
    return 0.f;
  };
  auto put = [&](char* st, const Tile<D>& tk, const Tile<D>& td, float ax) {
    tk.template store<!LS, true, NS>(st, tid);
    td.template store<true, !LS, NS>(st + KL::K::BYTES, tid);
    if (tid < 64) reinterpret_cast<float*>(st + KL::K::BYTES + KL::DO::BYTES)[tid] = ax;
  };
  Tile<D> tk, td;
  float ax = 0.f;
  if (rt_beg < rt_end) {
    tk.load(kb, C, (int64_t)rt_beg * 32, a.R - 1 - rt_beg * 32, tid);
    td.load(db_, C, (int64_t)rt_beg * 32, a.R - 1 - rt_beg * 32, tid);
    ax = aux_load(rt_beg);
    put(smem, tk, td, ax);
    __syncthreads();
  }
  for (int rt = rt_beg; rt < rt_end; ++rt) {
    const bool more = rt + 1 < rt_end;
    f32x16 scur;
    if constexpr (LS) scur = snext;
    if (more) {
      tk.load(kb, C, (int64_t)(rt + 1) * 32, a.R - 1 - (rt + 1) * 32, tid);
      td.load(db_, C, (int64_t)(rt + 1) * 32, a.R - 1 - (rt + 1) * 32, tid);
      ax = aux_load(rt + 1);
      if constexpr (LS)
        snext = blk_load(sbc + (rt + 1) * sstep, lane);
    }
    const char* ki = smem + ((rt - rt_beg) & 1) * KL::STAGE;
    const char* di = ki + KL::K::BYTES;
    const float* ls = reinterpret_cast<const float*>(di + KL::DO::BYTES);  // lse2[32], δ[32]
    int flag = c0 >= a.T ? 1 : (a.mflags ? flag_at(a.mflags, b, NRB32, NKT4, rt, c0 >> 6) : 0);
    flag = __builtin_amdgcn_readfirstlane(flag);
    f32x16 s, dp;  // (skipped tiles store whatever dp holds: nobody reads those blocks)
    if (flag != 1) {
      if constexpr (LS) s = scur;                                     // S  (row x col), stored by the forward
      else s = rowprod<D, !LS, true, NS>(ki, qf, f32x16{}, lane);     // S  (row x col)
      dp = rowprod<D, true, !LS, NS>(di, vf, f32x16{}, lane);         // dP (row x col)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = tidx(r, hf);
        const float p = ex2(__builtin_fmaf(s[r], c2, -ls[i]));
        s[r] = p;
        dp[r] = p * (dp[r] - ls[32 + i]);  // dS / scale
      }
      if (flag == 2) {  // masked entries: P = dS = 0 (the unmasked loop stays select-free)
        const uint32_t w = col_ok ? fa::settle((uint32_t)(a.mbits[((int64_t)b * NRT64 + (rt >> 1)) * TPAD + col] >> (32 * (rt & 1)))) : 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if ((w >> tidx(r, hf)) & 1u) s[r] = dp[r] = 0.f;
      }
    }
    // dS, every tile: uniform store counts keep the compiler's vmcnt waits exact (LDS writes
    // before the products, the transposed global stores after them)
    float* dwl = reinterpret_cast<float*>(smem + 2 * KL::STAGE) + wave * 1024;
    if constexpr (DS) fa::blk_put_lds(dwl, dp, lane);
    if (flag != 1) {
      if constexpr (LS) {
        trprod<D, false, true, NS>(ki, dp, dq, lane);  // dQᵀ += Kᵀ · dS
      } else {
        trprod<D, true, true, NS>(di, s, dv, lane);   // dVᵀ += dOᵀ · P
        trprod<D, true, true, NS>(ki, dp, dq, lane);  // dQᵀ += Kᵀ · dS
        fa::pin_agpr(dq);
        fa::pin_agpr(dv);
      }
    }
    if constexpr (DS) fa::blk_flush_lds(dsc + rt * dstep, dwl, lane);
    if (more) put(smem + ((rt + 1 - rt_beg) & 1) * KL::STAGE, tk, td, ax);
    __syncthreads();
  }
  if (!col_ok) return;
  const int64_t prow = ((int64_t)sp * a.B + b) * a.T + col;  // row of the split partials
  float* pq = ns > 1 ? a.cpq + prow * C + h * D : reinterpret_cast<float*>(a.dkc) + ((int64_t)b * a.T + col) * a.ldg + h * D;
  float* pv = ns > 1 ? a.cpv + prow * C + h * D : reinterpret_cast<float*>(a.dvc) + ((int64_t)b * a.T + col) * a.ldg + h * D;
  const float sc = a.scale;
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      *reinterpret_cast<f32x4*>(pq + db * 32 + 8 * g + 4 * hf) =
          f32x4{dq[db][4 * g] * sc, dq[db][4 * g + 1] * sc, dq[db][4 * g + 2] * sc, dq[db][4 * g + 3] * sc};
      if constexpr (!LS)
        *reinterpret_cast<f32x4*>(pv + db * 32 + 8 * g + 4 * hf) =
            f32x4{dv[db][4 * g], dv[db][4 * g + 1], dv[db][4 * g + 2], dv[db][4 * g + 3]};
    }
}

// ------------------------------------------------------------------------------------------
// Score-buffer mode, gathered side pass 1 of 2: dV_cols = Σ_rows Pᵀ · dO with P recomputed
// elementwise from the stored S (one product per tile, dO's transposed image only).  Runs BEFORE
// bwd_cols_kernel<D, true>, which overwrites S with dS.  Stage = dO image + lse2[32].
template <int D> struct DvL {
  using DO = Img<D, false, true>;
  static constexpr int STAGE = DO::BYTES + 128;
  static constexpr int LDS = 2 * STAGE;
};

template <int D>
__global__ __launch_bounds__(256, 2) void bwd_cols_dv_kernel(BwdArgs a) {
  using CF = Cfg<D>;
  using VL = DvL<D>;
  constexpr int DB = CF::DB, NS = 2;  // an S-buffer kernel: two-way family only
  using fa::smem;
  const int tid = threadIdx.x, lane = tid & 63, hf = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ncb = (a.T + 127) / 128;
  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  const int cb = lin % ncb, bhs = lin / ncb;
  const int bh = bhs % (a.B * a.H), sp = bhs / (a.B * a.H), ns = a.csv > 1 ? a.csv : 1;
  const int b = bh / a.H, h = bh % a.H;
  const int C = a.H * D;
  const int c0 = cb * 128 + wave * 32, col = c0 + (lane & 31);
  const bool col_ok = col < a.T, sown = c0 < a.T;
  const int NKT64 = (a.T + 63) / 64, NKT4 = (NKT64 + 3) & ~3, NRB32 = (a.R + 31) / 32;
  const int NRT64 = (a.R + 63) / 64, TPAD = (a.T + 127) / 128 * 128;
  const int NRT = (a.R + 31) / 32, NKT32 = (a.T + 31) / 32;
  const int rt_beg = (int)((int64_t)sp * NRT / ns), rt_end = (int)((int64_t)(sp + 1) * NRT / ns);
  const float* sbc = a.sbuf + ((int64_t)bh * NRB32 * NKT32 + min(c0 >> 5, NKT32 - 1)) * 1024;  // valid for every wave
  const int64_t sstep = (int64_t)NKT32 * 1024;
  const float* db_ = reinterpret_cast<const float*>(a.dout) + (int64_t)b * a.R * C + h * D;
  const float* lse2 = a.lse2 + ((int64_t)b * a.H + h) * a.R;
  const float c2 = a.scale * LOG2E, NEG_INF = -__builtin_inff();
  f32x16 dv[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i) dv[i] = f32x16{};
  auto aux_load = [&](int rt) -> float {  // lse2 (+inf past R: P = 0), threads 0..31
    const int rr = rt * 32 + tid;
    return tid < 32 && rr < a.R ? lse2[rr] : __builtin_inff();
  };
  constexpr int PF = fa::SB_PF;
  Tile<D> td;
  f32x16 q[PF];
  float ax = 0.f;
  if (rt_beg < rt_end) {
    td.load(db_, C, (int64_t)rt_beg * 32, a.R - 1 - rt_beg * 32, tid);
    ax = aux_load(rt_beg);
#pragma unroll
    for (int j = 0; j < PF; ++j)
      if (rt_beg + j < rt_end) q[j] = blk_load(sbc + (rt_beg + j) * sstep, lane);
    td.template store<false, true, NS>(smem, tid);
    if (tid < 32) reinterpret_cast<float*>(smem + VL::DO::BYTES)[tid] = ax;
    __syncthreads();
  }
  fa::ring_loop<PF>(rt_beg, rt_end, [&](int rt, auto J) {
    constexpr int j = decltype(J)::value;
    const bool more = rt + 1 < rt_end;
    f32x16 s = q[j];
    if (more) {
      td.load(db_, C, (int64_t)(rt + 1) * 32, a.R - 1 - (rt + 1) * 32, tid);
      ax = aux_load(rt + 1);
    }
    if (rt + PF < rt_end) q[j] = blk_load(sbc + (rt + PF) * sstep, lane);  // every wave: uniform vmcnt
    const char* di = smem + ((rt - rt_beg) & 1) * VL::STAGE;
    const float* ls = reinterpret_cast<const float*>(di + VL::DO::BYTES);
    int flag = !sown ? 1 : (a.mflags ? flag_at(a.mflags, b, NRB32, NKT4, rt, c0 >> 6) : 0);
    flag = __builtin_amdgcn_readfirstlane(flag);
    if (flag != 1) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = ex2(__builtin_fmaf(s[r], c2, -ls[tidx(r, hf)]));
      if (flag == 2) {  // masked entries: P = 0
        const uint32_t w = col_ok ? fa::settle((uint32_t)(a.mbits[((int64_t)b * NRT64 + (rt >> 1)) * TPAD + col] >> (32 * (rt & 1)))) : 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if ((w >> tidx(r, hf)) & 1u) s[r] = 0.f;
      }
      trprod<D, false, true, NS>(di, s, dv, lane);  // dVᵀ += dOᵀ · P
    }
    if (more) {
      char* nx = smem + ((rt + 1 - rt_beg) & 1) * VL::STAGE;
      td.template store<false, true, NS>(nx, tid);
      if (tid < 32) reinterpret_cast<float*>(nx + VL::DO::BYTES)[tid] = ax;
    }
    __syncthreads();
  });
  if (!col_ok) return;
  float* pv = ns > 1 ? a.cpv + (((int64_t)sp * a.B + b) * a.T + col) * C + h * D
                     : reinterpret_cast<float*>(a.dvc) + ((int64_t)b * a.T + col) * a.ldg + h * D;
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<f32x4*>(pv + db * 32 + 8 * g + 4 * hf) =
          f32x4{dv[db][4 * g], dv[db][4 * g + 1], dv[db][4 * g + 2], dv[db][4 * g + 3]};
}

// ------------------------------------------------------------------------------------------
// Score-buffer mode, row side: dK = scale · Σ_cols dS · Q_cols with dS from the buffer the
// column kernel wrote (one product per tile; Q's transposed image only).  Same grid, column split
// and partial protocol as bwd_rows_kernel.
template <int D, int NS = 2> struct RowsDsL {
  using Q = Img<D, false, true, NS>;
  static constexpr int LDS = 2 * Q::BYTES;
};

template <int D, int NS = 2>
__global__ __launch_bounds__(256, 2) void bwd_rows_ds_kernel(BwdArgs a) {
  using CF = Cfg<D>;
  using RL = RowsDsL<D, NS>;
  constexpr int DB = CF::DB;
  using fa::smem;
  const int tid = threadIdx.x, lane = tid & 63, hf = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nrb = (a.R + 127) / 128;
  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  const int rb = lin % nrb, bhs = lin / nrb;
  const int bh = bhs % (a.B * a.H), sp = bhs / (a.B * a.H);
  const int b = bh / a.H, h = bh % a.H;
  const int C = a.H * D;
  const int NKT64 = (a.T + 63) / 64, NKT32 = (a.T + 31) / 32;
  const int kt_beg = 2 * (int)((int64_t)sp * NKT64 / a.nsplit);
  const int kt_end = min(NKT32, 2 * (int)((int64_t)(sp + 1) * NKT64 / a.nsplit));
  const int r0 = rb * 128 + wave * 32, row = r0 + (lane & 31);
  const bool row_ok = row < a.R, wave_ok = r0 < a.R;
  const int NKT4 = (NKT64 + 3) & ~3, NRB32 = (a.R + 31) / 32;
  const float* qb = reinterpret_cast<const float*>(a.kc) + (int64_t)b * a.T * a.ldkv + h * D;
  const float* sbr = (a.dsbuf ? a.dsbuf : a.sbuf) + ((int64_t)bh * NRB32 + (wave_ok ? r0 >> 5 : 0)) * NKT32 * 1024;
  f32x16 dk[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i) dk[i] = f32x16{};

  constexpr int PF = fa::SB_PF;
  Tile<D> tq;
  f32x16 q[PF];
  if (kt_beg < kt_end) {
    tq.load(qb, a.ldkv, (int64_t)kt_beg * 32, a.T - 1 - kt_beg * 32, tid);
#pragma unroll
    for (int j = 0; j < PF; ++j)
      if (kt_beg + j < kt_end) q[j] = blk_load(sbr + (int64_t)(kt_beg + j) * 1024, lane);
    tq.template store<false, true, NS>(smem, tid);
    __syncthreads();
  }
  fa::ring_loop<PF>(kt_beg, kt_end, [&](int kt, auto J) {
    constexpr int j = decltype(J)::value;
    const bool more = kt + 1 < kt_end;
    f32x16 ds = q[j];
    if (more) tq.load(qb, a.ldkv, (int64_t)(kt + 1) * 32, a.T - 1 - (kt + 1) * 32, tid);
    if (kt + PF < kt_end) q[j] = blk_load(sbr + (int64_t)(kt + PF) * 1024, lane);  // every wave: uniform vmcnt
    const char* qi = smem + ((kt - kt_beg) & 1) * RL::Q::BYTES;
    int flag = !wave_ok ? 1 : (a.mflags ? flag_at(a.mflags, b, NRB32, NKT4, r0 >> 5, kt >> 1) : 0);
    flag = __builtin_amdgcn_readfirstlane(flag);
    if (flag != 1) {
      const int valid = a.T - kt * 32;
      if (valid < 32) {  // columns past T: the column kernel's values there are not gradients
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (tidx(r, hf) >= valid) ds[r] = 0.f;
      }
      trprod<D, false, true, NS>(qi, ds, dk, lane);  // dKᵀ += Q_colsᵀ · dSᵀ
    }
    if (more) tq.template store<false, true, NS>(smem + ((kt + 1 - kt_beg) & 1) * RL::Q::BYTES, tid);
    __syncthreads();
  });
  if (!row_ok) return;
  float* op = (a.nsplit > 1 || a.force_partial) ? a.dpart + (((int64_t)(a.sp0 + sp) * a.B + b) * a.R + row) * C + h * D
                                                : reinterpret_cast<float*>(a.drows) + ((int64_t)b * a.R + row) * C + h * D;
  const float sc = a.scale;
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<f32x4*>(op + db * 32 + 8 * g + 4 * hf) =
          f32x4{dk[db][4 * g] * sc, dk[db][4 * g + 1] * sc, dk[db][4 * g + 2] * sc, dk[db][4 * g + 3] * sc};
}

}  // namespace fa3
}  // namespace xdot

// ---- the three-way instantiations (flash_x6.hip), asked by the selectors of flash_x3.hip ----------
// Empty where a (kernel, head dim) pair has no three-way kernel.  There is no S-buffer kernel.
namespace xdot {
namespace fa3 {
fa::Kern<fa::FwdArgs> fwd_kern3(int D);
fa::Kern<fa::BwdArgs> rows_kern3(int D, bool reads_ds);
fa::Kern<fa::BwdArgs> cols_kern3(int D, bool stores_ds);
}  // namespace fa3
}  // namespace xdot
