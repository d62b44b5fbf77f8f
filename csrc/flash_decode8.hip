// xdot — decode attention over an fp8 (OCP e4m3fn) q/v cache for gfx950, and the kernel that fills it.
//
// Format: a slot is 2*Hg chunks of D bytes, [q heads | v heads], and one fp32 scale per chunk kept apart in
// `scales` (B, 2*Hg, cap), slot innermost: value = scale * e4m3(byte).  An empty slot holds zero bytes and
// scale 1.  cache_quant makes a chunk from D 16-bit values x: amax = max |x| (fp32), s = amax * (1 / 448)
// (s = 1 for amax = 0), byte = rne_e4m3(x / s) with a correctly rounded division; |x / s| <= 448 (1 + 2^-23)
// rounds to at most 448, so nothing saturates.  A non-finite x makes its chunk's scale or bytes non-finite.
//
// cache_quant_kernel: a group of D / 8 lanes owns one chunk (in a slot of 4 / 8 / 16 lanes, so D = 96 leaves
// 4 lanes of 16 idle): one 16-byte load per lane, amax over the group by xor shuffles, four
// v_cvt_pk_fp8_f32, one 8-byte store per lane, and the group's first lane stores the scale.  Chunks are
// dealt to threads in memory order, rows and bytes are touched once, there are no atomics: a prefill
// append is one bandwidth-bound pass, a one-row append one small launch.
//
// flash_decode8_kernel: flash_decode_kernel's work split, statistics, output layout and partial slots
// (csrc/flash_decode.hip, csrc/flash_decode.h) with the cache operands dequantised for free:
//   rows       stay 16-bit, and the products stay v_mfma_f32_16x16x32_{bf16,f16}: every e4m3 value is
//              exact in bf16 and fp16, so the bytes are widened in registers by
//              v_cvt_scalef32_pk_{bf16,f16}_fp8 with scale 1.0 and no fp8 MFMA (which would quantise the
//              rows) is used.
//   q operand  which feature sits in which k slot of S^T is free as long as both operands agree, so a lane
//              takes 16 contiguous bytes of its column (features 64 j + 16 g .. + 15) and feeds two
//              MFMAs from them (.. + 7 and + 8 .. + 15); where D / 32 is odd (D = 32, 96) the last 32
//              features are an 8-byte load (32 (DK - 1) + 8 g .. + 7).  The row fragments are loaded once
//              in the same order.
//   scales     per column, and S^T makes a lane's columns its own registers, like their positions:
//              x[e] = vis ? s * sc * sq[e] : -inf; l sums the unscaled p; the P^T fragment packs
//              p[e] * sv[e], rounded once where p alone was.  The 16 scales of a lane are loaded at the
//              top of a visible tile, with its q bytes (they are used after the S^T products, so they are
//              no later than those): a skipped tile loads neither bytes nor scales, and no scale
//              register lives across tiles.  Columns past the cache re-read the last slot's, like q.
//   v tile     the bytes are widened on the way into the wave-private LDS image, which keeps the 16-bit
//              [column][feature] layout and the ds_read_b64_tr_b16 reads of the 16-bit kernel: half the
//              global loads and staging registers, the same LDS.  Storing bytes and reading them with
//              ds_read_b64_tr_b8 would halve the LDS too, but registers, not LDS, bound the occupancy
//              (profiles/decode_fp8.md), and the k-slot order it returns would have to be matched by a
//              cross-lane shuffle of P^T.
#include "flash_decode.h"

#include <type_traits>

namespace xdot {
namespace fa {

template <int DT, int D, int NT>
__global__ __launch_bounds__(256) void flash_decode8_kernel(DecodeArgs a) {
  using Cfg = DecCfg<D, NT>;
  // DK S^T products per sub-tile: DP pairs fed by one 16-byte q load each, and a tail where DK is odd
  constexpr int DK = D / 32, DP = DK / 2, DN = D / 16, CH = D / 16;
  constexpr bool TAIL = DK & 1;
  constexpr float NINF = -__builtin_inff();
  __shared__ __attribute__((aligned(16))) char lds[Cfg::LDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, g = lane >> 4;
  const int sp = blockIdx.x % a.nspan, bh = blockIdx.x / a.nspan;
  const int hg = bh % a.Hg, b = bh / a.Hg;
  const int G = a.H / a.Hg, M = G * a.Rn, C = a.H * D;
  const float sc = a.scale * LOG2E;

  // the row fragments in the q operand's feature order, and each packed row's visible range (lo, hi]
  u32x4 rf[NT][DK];
  int lo[NT], hi[NT];
#pragma unroll
  for (int rt = 0; rt < NT; ++rt) {
    const int m = rt * 16 + n;
    const bool live = m < M;
    const int gh = live ? m / a.Rn : 0, i = live ? m - gh * a.Rn : 0;
    const char* p = reinterpret_cast<const char*>(a.rows) + (((int64_t)b * a.Rn + i) * C + (hg * G + gh) * D) * 2;
#pragma unroll
    for (int dk = 0; dk < DK; ++dk) {
      const int f = dk < 2 * DP ? 64 * (dk >> 1) + 16 * g + 8 * (dk & 1) : 32 * dk + 8 * g;
      rf[rt][dk] = live ? *reinterpret_cast<const u32x4*>(p + f * 2) : u32x4{0u, 0u, 0u, 0u};
    }
    hi[rt] = live ? a.pos0 + i : -1;  // a padding row sees nothing
    lo[rt] = a.window > 0 ? max(hi[rt] - a.window, -1) : -1;
  }
  const int whi = a.pos0 + a.Rn - 1, wlo = a.window > 0 ? max(a.pos0 - a.window, -1) : -1;

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
  const float* qs = a.qscale + b * a.sc_batch + hg * a.sc_head;
  const float* vs = a.vscale + b * a.sc_batch + hg * a.sc_head;
  const int64_t ldb = a.ldkv;
  char* vl = lds + wave * Cfg::VTILE;
  typedef const __attribute__((address_space(3))) char lds_char;
  lds_char* vt = (lds_char*)vl + (4 * g + (n >> 2)) * Cfg::VROW + 8 * (n & 3);

  auto load_pos = [&](int t, int (&pos)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = t * DEC_TILE + 16 * (e >> 2) + 4 * g + (e & 3);
      pos[e] = (t < t1 && c < a.Tcap) ? cp[c] : -1;
    }
  };
  int pos[8], nxt[8];
  load_pos(t0 + wave, pos);
  for (int t = t0 + wave; t < t1; t += 4) {
    load_pos(t + 4, nxt);
    bool seen = false;
#pragma unroll
    for (int e = 0; e < 8; ++e) seen |= pos[e] > wlo && pos[e] <= whi;
    if (__builtin_amdgcn_ballot_w64(seen) != 0) {
      const int c0 = t * DEC_TILE, cmax = a.Tcap - 1;
      float sq[8], sv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = min(c0 + 16 * (e >> 2) + 4 * g + (e & 3), cmax);
        sq[e] = qs[c];
        sv[e] = vs[c];
      }
      // q bytes from global memory (columns past the cache re-read the last one: invisible)
      u32x4 qp[2][DP > 0 ? DP : 1];
      u32x2 qt[2];
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        const char* p = qb + (int64_t)min(c0 + 16 * sub + n, cmax) * ldb;
#pragma unroll
        for (int j = 0; j < DP; ++j) qp[sub][j] = *reinterpret_cast<const u32x4*>(p + 64 * j + 16 * g);
        if constexpr (TAIL) qt[sub] = *reinterpret_cast<const u32x2*>(p + 32 * (DK - 1) + 8 * g);
      }
      // the v tile: DK 16-byte chunks per lane, rows of CH chunks
      u32x4 vr[DK];
#pragma unroll
      for (int it = 0; it < DK; ++it) {
        const int x = it * 64 + lane, r = x / CH, ch = x - r * CH;
        vr[it] = *reinterpret_cast<const u32x4*>(vb + (int64_t)min(c0 + r, cmax) * ldb + ch * 16);
      }
      f32x4 s[NT][2];
#pragma unroll
      for (int rt = 0; rt < NT; ++rt) s[rt][0] = s[rt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int dk = 0; dk < DK; ++dk) {
          u32x4 qf;
          if (dk < 2 * DP) qf = widen8<DT>(qp[sub][dk >> 1][2 * (dk & 1)], qp[sub][dk >> 1][2 * (dk & 1) + 1]);
          else qf = widen8<DT>(qt[sub][0], qt[sub][1]);
#pragma unroll
          for (int rt = 0; rt < NT; ++rt) s[rt][sub] = mfma16<DT>::run(qf, rf[rt][dk], s[rt][sub]);
        }
      wave_sync();  // the previous tile's reads are done
#pragma unroll
      for (int it = 0; it < DK; ++it) {
        const int x = it * 64 + lane, r = x / CH, ch = x - r * CH;
        u32x4* d = reinterpret_cast<u32x4*>(vl + r * Cfg::VROW + ch * 32);
        d[0] = widen8<DT>(vr[it][0], vr[it][1]);
        d[1] = widen8<DT>(vr[it][2], vr[it][3]);
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
          x[e] = vis ? s[rt][e >> 2][e & 3] * sc * sq[e] : NINF;
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
      wave_sync();  // the tile image is complete
#pragma unroll
      for (int dn = 0; dn < DN; ++dn) {
        union { struct { s16x4 a, b; } h; u32x4 u; } vf;
        vf.h.a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vt + dn * 32));
        vf.h.b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vt + 16 * Cfg::VROW + dn * 32));
#pragma unroll
        for (int rt = 0; rt < NT; ++rt) o[rt][dn] = mfma16<DT>::run(vf.u, pf[rt], o[rt][dn]);
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) pos[e] = nxt[e];
  }
  decode_merge_waves<D, NT>(a, lds, mrun, lrun, o, sp, b, hg);
}

template <int DT, int D>
__global__ __launch_bounds__(256) void cache_quant_kernel(QuantArgs a) {
  using V8 = typename std::conditional<DT == DT_BF16, bf16x8, f16x8>::type;
  constexpr int L = D / 8, W = L <= 4 ? 4 : L <= 8 ? 8 : 16;  // lanes of a chunk, and of its slot in the wave
  const int64_t chunk = ((int64_t)blockIdx.x * 256 + threadIdx.x) / W;
  const int li = threadIdx.x % W;
  const bool live = chunk < (int64_t)a.B * a.n * a.chunks && li < L;
  const int c = (int)(chunk % a.chunks);
  const int64_t bi = chunk / a.chunks, i = bi % a.n, b = bi / a.n;
  float x[8];
  float amax = 0.f;
  if (live) {
    const char* p = reinterpret_cast<const char*>(a.rows) + (b * a.sb + i * a.sr + c * D + 8 * li) * 2;
    const V8 v = __builtin_bit_cast(V8, *reinterpret_cast<const u32x4*>(p));
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      x[e] = (float)v[e];
      amax = fmaxf(amax, fabsf(x[e]));
    }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = 0.f;
  }
#pragma unroll
  for (int o = W / 2; o >= 1; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
  const float s = amax == 0.f ? 1.f : amax * (1.f / 448.f);
  int w0 = __builtin_amdgcn_cvt_pk_fp8_f32(x[0] / s, x[1] / s, 0, false);
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(x[2] / s, x[3] / s, w0, true);
  int w1 = __builtin_amdgcn_cvt_pk_fp8_f32(x[4] / s, x[5] / s, 0, false);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(x[6] / s, x[7] / s, w1, true);
  if (live) {
    const int64_t slot = b * a.cap + a.at + i;
    *reinterpret_cast<u32x2*>(reinterpret_cast<char*>(a.qv8) + (slot * a.chunks + c) * D + 8 * li) = u32x2{(uint32_t)w0, (uint32_t)w1};
    if (li == 0) a.scales[(b * a.chunks + c) * a.cap + a.at + i] = s;
  }
}

template <int DT, int D>
static int launch_decode8(const DecodeArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)(a.nspan * a.B * a.Hg));
  switch (decode_row_tiles(a.H / a.Hg, a.Rn)) {
    case 1: hipLaunchKernelGGL((flash_decode8_kernel<DT, D, 1>), grid, dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL((flash_decode8_kernel<DT, D, 2>), grid, dim3(256), 0, st, a); break;
    case 3:  // three row tiles run as four, as in the 16-bit sweep
    case 4: hipLaunchKernelGGL((flash_decode8_kernel<DT, D, 4>), grid, dim3(256), 0, st, a); break;
    default: return -1;
  }
  return xdot_flash_decode_combine_launch(&a, DT, D, st);
}

}  // namespace fa
}  // namespace xdot

extern "C" int xdot_flash_decode8_launch(const xdot::fa::DecodeArgs* a, int dt, int D, hipStream_t st) {
  using namespace xdot;
  using namespace xdot::fa;
  if (a->B == 0 || a->Rn == 0 || a->H == 0) return 0;
  return for_dtype16_head_dim(dt, D, -1, [&](auto t, auto d) { return launch_decode8<decltype(t)::value, decltype(d)::value>(*a, st); });
}

extern "C" int xdot_cache_quant_launch(const xdot::fa::QuantArgs* a, int dt, int D, hipStream_t st) {
  using namespace xdot;
  using namespace xdot::fa;
  constexpr int none = -1;
  return for_dtype16_head_dim(dt, D, none, [&](auto t, auto d) {
    constexpr int Dc = decltype(d)::value, L = Dc / 8, W = L <= 4 ? 4 : L <= 8 ? 8 : 16;
    const int64_t threads = (int64_t)a->B * a->n * a->chunks * W;
    if (threads == 0) return 0;
    if ((threads + 255) / 256 >= (1LL << 31)) return none;
    hipLaunchKernelGGL((cache_quant_kernel<decltype(t)::value, Dc>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, *a);
    return 0;
  });
}
