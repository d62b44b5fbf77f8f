// xdot — chunked prefill over an fp8 (OCP e4m3fn) q/v cache for gfx950: many new rows against one rank's
// cache of bytes and per-slot scales, forward only.
//
// The contract and the work split are flash_extend_kernel's (csrc/flash_extend.hip), the cache format is
// flash_decode8_kernel's (csrc/flash_decode8.hip): one workgroup per (column span, row block, batch, GATHERED
// head), a row block being rb consecutive new rows x the G row heads of the group; wave w owns the NT 16-row
// tiles w NT .. w NT + NT - 1 for the whole sweep (fragments, running (m, l) and output in registers, no merge
// after the sweep); tiles none of whose positions any row of the block can see are skipped by the 64-tile
// scan with a workgroup-uniform ballot; two LDS images, one workgroup barrier per visible tile; one span
// writes out / lse, several write the decode partial layout for flash_decode_combine.  No atomics, one
// writer per output element, a fixed summation order.
//
// What differs is how a tile travels and where the scales go:
//   bytes      a 32-column tile of q and v is 64 D bytes = 8 D chunks of 8 bytes: D / 32 chunks per thread, as
//              in the 16-bit kernel, but 8-byte global loads into half the staging registers.  A chunk is
//              widened in registers on its way into LDS (widen8: v_cvt_scalef32_pk_{bf16,f16}_fp8 at scale
//              1.0, exact) and stored as 16 bytes into the 16-bit kernel's [column][feature] image (rows of
//              2 D + 16 bytes), ONCE per tile for all four waves (the decode sweep widens per wave).  The
//              ds_read_b128 reads of the S^T operand, the ds_read_b64_tr_b16 reads of V^T and both MFMA
//              groups are the 16-bit kernel's: the rows stay 16-bit and no fp8 MFMA, which would quantise
//              them, is used.  Columns past the cache re-read the last slot (invisible).
//   scales     per column.  Held in registers across the one-tile-ahead prefetch they would cost a lane 16
//              registers per tile in flight; instead threads 0 .. 31 prefetch qscale of the next tile's 32
//              columns and threads 32 .. 63 its vscale (one register, clamped to the last slot) and store
//              them behind the tile image (256 bytes per image); after the barrier a lane reads the scales
//              of its columns 16 sub + 4 g .. + 3 with four ds_read_b128.
//   softmax    x[e] = vis ? s * (sc * sq[e]) : -inf (sc goes into the lane's 8 scales once per tile); l sums
//              the unscaled p; the P^T fragment packs p[e] * sv[e], rounded once where p alone was: scale *
//              byte never exists as a 16-bit value.
// Invisible and empty slots must hold finite bytes and scales (an empty slot: zero bytes, scale 1); a row
// that sees nothing gives NaN with lse -inf.
#include "flash_decode.h"

namespace xdot {
namespace fa {

// LDS of one workgroup: two images of (q tile, v tile, 32 q scales, 32 v scales)
template <int D> struct Ext8Cfg {
  static constexpr int NT = extend_row_tiles(D);
  static constexpr int VROW = 2 * D + 16;
  static constexpr int VTILE = DEC_TILE * VROW;
  static constexpr int OFF_SC = 2 * VTILE;
  static constexpr int IMG = OFF_SC + 2 * DEC_TILE * 4;
  static constexpr int LDS = 2 * IMG;
};

template <int DT, int D, int NT>
__global__ __launch_bounds__(256) void flash_extend8_kernel(ExtendArgs ea) {
  using T16 = typename dt_traits<DT>::T;
  using Cfg = Ext8Cfg<D>;
  const DecodeArgs& a = ea.d;
  constexpr int DK = D / 32, DN = D / 16, CH = D / 8;  // CH: 8-byte chunks of a cache row
  constexpr float NINF = -__builtin_inff();
  __shared__ __attribute__((aligned(16))) char lds[Cfg::LDS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g = lane >> 4;
  const int sp = blockIdx.x % a.nspan, rest = blockIdx.x / a.nspan;
  const int blk = rest % ea.nblk, bh = rest / ea.nblk;
  const int hg = bh % a.Hg, b = bh / a.Hg;
  const int G = a.H / a.Hg, C = a.H * D;
  const int i0 = blk * ea.rb, i1 = min(i0 + ea.rb, a.Rn);
  const float sc = a.scale * LOG2E;

  // the row fragments (B operand of S^T) and each packed row's visible position range (lo, hi]
  u32x4 rf[NT][DK];
  int lo[NT], hi[NT], oh[NT], oi[NT];
#pragma unroll
  for (int rt = 0; rt < NT; ++rt) {
    const int m = (wave * NT + rt) * 16 + n;
    const int gh = m / ea.rb, i = i0 + m - gh * ea.rb;
    const bool live = gh < G && i < i1;
    oh[rt] = live ? hg * G + gh : -1;  // -1: a padding row, never written
    oi[rt] = i;
    const char* p = reinterpret_cast<const char*>(a.rows) + (((int64_t)b * a.Rn + (live ? i : 0)) * C + (live ? oh[rt] : 0) * D + 8 * g) * 2;
#pragma unroll
    for (int dk = 0; dk < DK; ++dk)
      rf[rt][dk] = live ? *reinterpret_cast<const u32x4*>(p + dk * 64) : u32x4{0u, 0u, 0u, 0u};
    hi[rt] = live ? a.pos0 + i : -1;
    lo[rt] = a.window > 0 ? max(hi[rt] - a.window, -1) : -1;
  }
  // what any row of the block can see
  const int whi = a.pos0 + i1 - 1, wlo = a.window > 0 ? max(a.pos0 + i0 - a.window, -1) : -1;

  float mrun[NT], lrun[NT];
  f32x4 o[NT][DN];
#pragma unroll
  for (int rt = 0; rt < NT; ++rt) {
    mrun[rt] = NINF;
    lrun[rt] = 0.f;
#pragma unroll
    for (int dn = 0; dn < DN; ++dn) o[rt][dn] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const int ntiles = (a.Tcap + DEC_TILE - 1) / DEC_TILE;
  const int t0 = sp * a.span_tiles, t1 = min(t0 + a.span_tiles, ntiles);
  const int32_t* cp = a.col_pos + (int64_t)b * a.Tcap;
  const char* qb = reinterpret_cast<const char*>(a.qc) + (int64_t)b * a.Tcap * a.ldkv + hg * D;
  const char* vb = reinterpret_cast<const char*>(a.vc) + (int64_t)b * a.Tcap * a.ldkv + hg * D;
  // threads 0 .. 31 carry a q scale, 32 .. 63 a v scale (the other waves never load one)
  const float* sb = (tid < DEC_TILE ? a.qscale : a.vscale) + b * a.sc_batch + hg * a.sc_head;
  const int64_t ldb = a.ldkv;
  const int cmax = a.Tcap - 1;
  typedef const __attribute__((address_space(3))) char lds_char;

  // the visible tiles of the span in order, 64 tiles per scan; uniform over the workgroup
  int tc = t0 - 64;
  uint64_t act = 0;
  auto next_tile = [&]() -> int {
    for (;;) {
      if (act) {
        const int j = __builtin_ctzll(act);
        act &= act - 1;
        return tc + j;
      }
      tc += 64;
      if (tc >= t1) return t1;
      const int t = tc + lane;
      bool seen = false;
      if (t < t1) {
        const int c0 = t * DEC_TILE, nc = min(DEC_TILE, a.Tcap - c0);
        for (int e = 0; e < nc; ++e) {
          const int p = cp[c0 + e];
          seen |= p > wlo && p <= whi;
        }
      }
      act = __builtin_amdgcn_ballot_w64(seen);
    }
  };

  // a tile on its way from global memory to LDS: the thread's DK 8-byte chunks of the q / v rows (columns
  // past the cache re-read the last one: invisible), its scale, and the positions of the lane's 8 columns
  // (past the cache: empty)
  u32x2 gl[DK];
  float nsc = 1.f;
  int npos[8];
  auto gload = [&](int t) {
    const int c0 = t * DEC_TILE;
#pragma unroll
    for (int it = 0; it < DK; ++it) {
      const int x = it * 256 + tid, mat = x / (DEC_TILE * CH), y = x - mat * (DEC_TILE * CH), r = y / CH, ch = y - r * CH;
      gl[it] = *reinterpret_cast<const u32x2*>((mat ? vb : qb) + (int64_t)min(c0 + r, cmax) * ldb + ch * 8);
    }
    if (tid < 2 * DEC_TILE) nsc = sb[min(c0 + (tid & (DEC_TILE - 1)), cmax)];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = c0 + 16 * (e >> 2) + 4 * g + (e & 3);
      npos[e] = c < a.Tcap ? cp[c] : -1;
    }
  };

  int t = next_tile();
  if (t < t1) gload(t);
  int buf = 0;
  while (t < t1) {
    char* img = lds + buf * Cfg::IMG;
#pragma unroll
    for (int it = 0; it < DK; ++it) {
      const int x = it * 256 + tid, mat = x / (DEC_TILE * CH), y = x - mat * (DEC_TILE * CH), r = y / CH, ch = y - r * CH;
      *reinterpret_cast<u32x4*>(img + mat * Cfg::VTILE + r * Cfg::VROW + ch * 16) = widen8<DT>(gl[it][0], gl[it][1]);
    }
    if (tid < 2 * DEC_TILE) *reinterpret_cast<float*>(img + Cfg::OFF_SC + 4 * tid) = nsc;
    int pos[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) pos[e] = npos[e];
    const int tn = next_tile();
    if (tn < t1) gload(tn);  // in flight during this tile's MFMAs
    // this tile's image is complete; the other image, which the next iteration overwrites, was last read
    // before this barrier
    __syncthreads();

    f32x4 s[NT][2];
#pragma unroll
    for (int rt = 0; rt < NT; ++rt) s[rt][0] = s[rt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const char* qp = img + (16 * sub + n) * Cfg::VROW + 16 * g;
#pragma unroll
      for (int dk = 0; dk < DK; ++dk) {
        const u32x4 qf = *reinterpret_cast<const u32x4*>(qp + dk * 64);
#pragma unroll
        for (int rt = 0; rt < NT; ++rt) s[rt][sub] = mfma16<DT>::run(qf, rf[rt][dk], s[rt][sub]);
      }
    }
    // the scales of the lane's columns 16 sub + 4 g .. + 3
    float sq[8], sv[8];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const f32x4 q4 = *reinterpret_cast<const f32x4*>(img + Cfg::OFF_SC + (16 * sub + 4 * g) * 4);
      const f32x4 v4 = *reinterpret_cast<const f32x4*>(img + Cfg::OFF_SC + (DEC_TILE + 16 * sub + 4 * g) * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sq[4 * sub + j] = q4[j] * sc;
        sv[4 * sub + j] = v4[j];
      }
    }
    // online softmax per row tile -> P^T fragments
    u32x4 pf[NT];
#pragma unroll
    for (int rt = 0; rt < NT; ++rt) {
      float x[8];
      float mx = NINF;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const bool vis = pos[e] > lo[rt] && pos[e] <= hi[rt];
        x[e] = vis ? s[rt][e >> 2][e & 3] * sq[e] : NINF;
        mx = fmaxf(mx, x[e]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mnew = fmaxf(mrun[rt], mx);
      const float muse = mnew == NINF ? 0.f : mnew;  // nothing seen yet: every p is 2^-inf = 0
      const float alpha = fast_exp2(mrun[rt] - muse);
      float sum = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        x[e] = fast_exp2(x[e] - muse);
        sum += x[e];
        x[e] *= sv[e];
      }
      lrun[rt] = lrun[rt] * alpha + sum;  // the lane's share: summed over g after the sweep
      mrun[rt] = mnew;
#pragma unroll
      for (int dn = 0; dn < DN; ++dn) o[rt][dn] *= alpha;
      pf[rt] = u32x4{pack2<DT>(x[0], x[1]), pack2<DT>(x[2], x[3]), pack2<DT>(x[4], x[5]), pack2<DT>(x[6], x[7])};
    }
    lds_char* vt = (lds_char*)img + Cfg::VTILE + (4 * g + (n >> 2)) * Cfg::VROW + 8 * (n & 3);
#pragma unroll
    for (int dn = 0; dn < DN; ++dn) {
      union { struct { s16x4 a, b; } h; u32x4 u; } vf;
      vf.h.a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vt + dn * 32));
      vf.h.b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vt + 16 * Cfg::VROW + dn * 32));
#pragma unroll
      for (int rt = 0; rt < NT; ++rt) o[rt][dn] = mfma16<DT>::run(vf.u, pf[rt], o[rt][dn]);
    }
    t = tn;
    buf ^= 1;
  }

  // ---- the wave's own rows: normalise and write -----------------------------------------------------
  const bool whole = a.nspan == 1;
#pragma unroll
  for (int rt = 0; rt < NT; ++rt) {
    float lt = lrun[rt];
    lt += __shfl_xor(lt, 16, 64);
    lt += __shfl_xor(lt, 32, 64);
    if (oh[rt] < 0) continue;
    const int h = oh[rt], i = oi[rt];
    const float lse = lt > 0.f ? (mrun[rt] + __log2f(lt)) * LN2 : NINF;
    const int64_t at = ((int64_t)b * a.Rn + i) * C + h * D + 4 * g;
    if (whole) {
      const float inv = 1.f / lt;  // nothing visible: 0 * inf = NaN, like the spans' merge
#pragma unroll
      for (int dn = 0; dn < DN; ++dn) {
        const f32x4 v = o[rt][dn] * inv;
        if (a.out32) {
          *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.out) + at + dn * 16) = v;
        } else {
          const u32x2 w = {pack2<DT>(v[0], v[1]), pack2<DT>(v[2], v[3])};
          *reinterpret_cast<u32x2*>(reinterpret_cast<T16*>(a.out) + at + dn * 16) = w;
        }
      }
      if (g == 0) a.lse[((int64_t)b * a.H + h) * a.Rn + i] = lse;
    } else {
      const float inv = lt > 0.f ? 1.f / lt : 0.f;
      float* op = a.opart + (int64_t)sp * a.B * a.Rn * C + at;
#pragma unroll
      for (int dn = 0; dn < DN; ++dn) *reinterpret_cast<f32x4*>(op + dn * 16) = o[rt][dn] * inv;
      if (g == 0) a.lpart[(((int64_t)sp * a.B + b) * a.H + h) * a.Rn + i] = lse;
    }
  }
}

template <int DT, int D>
static int launch_extend8(const ExtendArgs& ea, hipStream_t st) {
  constexpr int NT = Ext8Cfg<D>::NT;
  const DecodeArgs& a = ea.d;
  if (!a.qscale || !a.vscale) return -1;
  if (ea.rb < 1 || (int64_t)ea.rb * (a.H / a.Hg) > 64 * NT || (int64_t)ea.rb * ea.nblk < a.Rn) return -1;
  hipLaunchKernelGGL((flash_extend8_kernel<DT, D, NT>), dim3((unsigned)(a.nspan * ea.nblk * a.B * a.Hg)), dim3(256), 0, st, ea);
  return a.nspan > 1 ? xdot_flash_decode_combine_launch(&a, DT, D, st) : 0;
}

}  // namespace fa
}  // namespace xdot

// the sweep of every (span, row block) of an fp8 cache (a->d.qscale / vscale set, a->d.ldkv in bytes) into
// a->d.out / lse (one span) or into a->d.opart / lpart and their merge (several); -1: no kernel for this
// dtype / head dim, no scales, or a row block the kernel does not hold
extern "C" int xdot_flash_extend8_launch(const xdot::fa::ExtendArgs* a, int dt, int D, hipStream_t st) {
  using namespace xdot;
  using namespace xdot::fa;
  if (a->d.B == 0 || a->d.Rn == 0 || a->d.H == 0) return 0;
  return for_dtype16_head_dim(dt, D, -1, [&](auto t, auto d) { return launch_extend8<decltype(t)::value, decltype(d)::value>(*a, st); });
}
