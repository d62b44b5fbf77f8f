// xdot — what the decode sweeps share (csrc/flash_decode.hip: a 16-bit cache, csrc/flash_decode8.hip: an
// fp8 cache): the 16x16x32 MFMA, the LDS plan of a workgroup, and the merge of the 4 waves' running
// (m, l, o) into the workgroup's partial slot.
#pragma once
#include "flash_launch.h"

namespace xdot {
namespace fa {

template <int DT> struct mfma16;
template <> struct mfma16<DT_BF16> {
  static __device__ __forceinline__ f32x4 run(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
};
template <> struct mfma16<DT_F16> {
  static __device__ __forceinline__ f32x4 run(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
};

// fp8 caches (csrc/flash_decode8.hip, csrc/flash_extend8.hip): 4 e4m3 bytes -> 4 values of the rows' dtype
// (exact: v_cvt_scalef32_pk_{bf16,f16}_fp8 at scale 1.0), and 8 bytes -> one 16-byte MFMA operand chunk
template <int DT> __device__ __forceinline__ u32x2 widen4(uint32_t w);
template <> __device__ __forceinline__ u32x2 widen4<DT_BF16>(uint32_t w) {
  return u32x2{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false)),
               __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true))};
}
template <> __device__ __forceinline__ u32x2 widen4<DT_F16>(uint32_t w) {
  return u32x2{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, false)),
               __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, true))};
}
template <int DT> __device__ __forceinline__ u32x4 widen8(uint32_t lo, uint32_t hi) {
  const u32x2 a = widen4<DT>(lo), b = widen4<DT>(hi);
  return u32x4{a[0], a[1], b[0], b[1]};
}

// LDS of one workgroup: the 4 waves' v tiles (rows of 2 D + 16 bytes), reused after the sweep as the
// fp32 output image the waves add into ([row][D + 4]), then the per-wave and the merged (m, l)
template <int D, int NT> struct DecCfg {
  static constexpr int VROW = 2 * D + 16;
  static constexpr int VTILE = DEC_TILE * VROW;
  static constexpr int OROW = D + 4;  // floats
  static constexpr int OIMG = NT * 16 * OROW * 4;
  static constexpr int OFF_STAT = (4 * VTILE > OIMG ? 4 * VTILE : OIMG);
  static constexpr int LDS = OFF_STAT + (2 * 4 + 2) * NT * 16 * 4;
};

// order this wave's LDS accesses (the tile image is written by some lanes and read by others)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// After the sweep: merge the 4 waves' (m, l, o) through LDS (the output image overlays the v tiles) and
// write the workgroup's partial slot, the output normalised over the span and its natural-log LSE (-inf:
// nothing visible).  Lane (n = lane & 15, g = lane >> 4) holds row 16 rt + n, features 16 dn + 4 g .. + 3;
// lrun is the lane's share of l (summed over g here).  The fp8 sweep calls this; flash_decode_kernel keeps
// the same statements in its own body, where the compiler's register figures of its four-row-tile
// instantiations (profiles/decode.md) depend on them standing inline.
template <int D, int NT>
__device__ __forceinline__ void decode_merge_waves(const DecodeArgs& a, char* lds, float (&mrun)[NT], float (&lrun)[NT],
                                                   f32x4 (&o)[NT][D / 16], int sp, int b, int hg) {
  using Cfg = DecCfg<D, NT>;
  constexpr int DN = D / 16;
  constexpr float NINF = -__builtin_inff();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, g = lane >> 4;
  const int G = a.H / a.Hg, M = G * a.Rn, C = a.H * D;
  float* wm = reinterpret_cast<float*>(lds + Cfg::OFF_STAT);  // [4][NT * 16]
  float* wl = wm + 4 * NT * 16;                                // [4][NT * 16]
  float* tm = wl + 4 * NT * 16;                                // merged m, l: [NT * 16] each
  float* tl = tm + NT * 16;
  float* oimg = reinterpret_cast<float*>(lds);
#pragma unroll
  for (int rt = 0; rt < NT; ++rt) {
    lrun[rt] += __shfl_xor(lrun[rt], 16, 64);
    lrun[rt] += __shfl_xor(lrun[rt], 32, 64);
    if (g == 0) {
      wm[wave * NT * 16 + rt * 16 + n] = mrun[rt];
      wl[wave * NT * 16 + rt * 16 + n] = lrun[rt];
    }
  }
  __syncthreads();  // also: every wave is done with its v tile, which the output image overlays
#pragma unroll
  for (int rt = 0; rt < NT; ++rt) {
    float mt = NINF;
#pragma unroll
    for (int w = 0; w < 4; ++w) mt = fmaxf(mt, wm[w * NT * 16 + rt * 16 + n]);
    const float muse = mt == NINF ? 0.f : mt;
    float lt = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) lt += wl[w * NT * 16 + rt * 16 + n] * fast_exp2(wm[w * NT * 16 + rt * 16 + n] - muse);
    const float wgt = fast_exp2(mrun[rt] - muse);
#pragma unroll
    for (int dn = 0; dn < DN; ++dn) o[rt][dn] *= wgt;
    if (wave == 0 && g == 0) {
      tm[rt * 16 + n] = mt;
      tl[rt * 16 + n] = lt;
    }
  }
  // the waves add their outputs in wave order: the same sum every run
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int rt = 0; rt < NT; ++rt)
#pragma unroll
        for (int dn = 0; dn < DN; ++dn) {
          f32x4* p = reinterpret_cast<f32x4*>(oimg + (rt * 16 + n) * Cfg::OROW + dn * 16 + 4 * g);
          *p = w == 0 ? o[rt][dn] : *p + o[rt][dn];
        }
    }
    __syncthreads();
  }
  for (int idx = threadIdx.x; idx < M * (D / 4); idx += 256) {
    const int m = idx / (D / 4), c4 = idx - m * (D / 4);
    const int gh = m / a.Rn, i = m - gh * a.Rn, h = hg * G + gh;
    const float lt = tl[m], inv = lt > 0.f ? 1.f / lt : 0.f;
    const f32x4 v = *reinterpret_cast<const f32x4*>(oimg + m * Cfg::OROW + 4 * c4) * inv;
    *reinterpret_cast<f32x4*>(a.opart + (((int64_t)sp * a.B + b) * a.Rn + i) * C + h * D + 4 * c4) = lt > 0.f ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    if (c4 == 0) a.lpart[(((int64_t)sp * a.B + b) * a.H + h) * a.Rn + i] = lt > 0.f ? (tm[m] + __log2f(lt)) * LN2 : NINF;
  }
}

}  // namespace fa
}  // namespace xdot
