// xdot — rotary position embedding (RoPE) of the projected k / q, a pass of its own between the
// projection and the attention (the flash kernels know nothing about positions).
//
// Half-split pairs: in a head of width D element i pairs with i + D/2 (i < D/2), and with the
// angle t(p, i) = p * inv_freq[i] of the row's global position p
//   out[i]       = alpha * (x[i]       * cos t - x[i + D/2] * sin t)
//   out[i + D/2] = alpha * (x[i + D/2] * cos t + x[i]       * sin t)
// (`inverse` negates sin).  rope_table builds cos / sin (R, D/2) once per shape in fp64 (an fp32
// product p * inv_freq is off by ~1e-2 rad at p = 2e5), rounded once to fp32; rope_apply is the
// per-step kernel: bandwidth bound, fp32 math, one rounding to the output dtype.
#include "common.h"

#include <type_traits>

namespace xdot {

__global__ __launch_bounds__(256) void rope_table_kernel(float* __restrict__ cosb, float* __restrict__ sinb,
                                                          const double* __restrict__ inv_freq, int64_t total, int half,
                                                          int64_t offset) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int64_t row = t / half;
  const int i = (int)(t - row * half);
  const double ang = (double)(offset + row) * inv_freq[i];
  double s, c;
  sincos(ang, &s, &c);
  cosb[t] = (float)c;
  sinb[t] = (float)s;
}

// one pair: both outputs from both inputs, the same expression on every path (bitwise equal
// results whichever kernel mode a view takes)
__device__ __forceinline__ void rope_pair(float x1, float x2, float c, float s, float& o1, float& o2) {
  o1 = __builtin_fmaf(-x2, s, x1 * c);
  o2 = __builtin_fmaf(x1, s, x2 * c);
}

// A lane owns one chunk of V consecutive pair indices of one row: it loads the chunk's table
// fragment once (alpha folded in) and walks the (batch, head) pairs dealt to its blockIdx.y, so
// the fragment is reused from registers.  Per head it loads BOTH halves before it stores either
// (in-place calls), and no two lanes touch the same element.
//   MODE 1: V = 16 bytes of elements, aligned 16-byte loads / stores; D/2 % V == 0
//   MODE 2: the same chunks with 2-byte-aligned 16-byte vectors, the last partial chunk scalar
//   MODE 0: V = 1, scalar
template <int DT, int MODE>
__global__ __launch_bounds__(256) void rope_apply_kernel(RopeArgs a) {
  using T = typename dt_traits<DT>::T;
  constexpr int V = MODE == 0 ? 1 : 16 / (int)sizeof(T);
  using Vec = typename std::conditional<MODE == 1, u32x4, u32x4_ua>::type;
  const int half = a.D >> 1;
  const int nchunk = (half + V - 1) / V;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)a.R * nchunk) return;
  const int64_t row = t / nchunk;
  const int i0 = (int)(t - row * nchunk) * V;
  const int nv = half - i0 < V ? half - i0 : V;  // < V only on MODE 2's last chunk
  const float sgn = a.inverse ? -a.alpha : a.alpha;
  float c[V], s[V];
  const float* cp = a.cos + row * half + i0;
  const float* sp = a.sin + row * half + i0;
  if constexpr (MODE == 1) {
#pragma unroll
    for (int e = 0; e < V; e += 4) {
      const f32x4 cv = *reinterpret_cast<const f32x4*>(cp + e);
      const f32x4 sv = *reinterpret_cast<const f32x4*>(sp + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        c[e + j] = cv[j] * a.alpha;
        s[e + j] = sv[j] * sgn;
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      c[e] = e < nv ? cp[e] * a.alpha : 0.f;
      s[e] = e < nv ? sp[e] * sgn : 0.f;
    }
  }
  const T* xrow = reinterpret_cast<const T*>(a.x) + row * a.xs_r + i0;
  T* orow = reinterpret_cast<T*>(a.out) + row * a.os_r + i0;
  const int nbh = a.B * a.H, gy = (int)gridDim.y;
  auto xptr = [&](int bh) { return xrow + (bh / a.H) * a.xs_b + (int64_t)(bh % a.H) * a.D; };
  auto optr = [&](int bh) { return orow + (bh / a.H) * a.os_b + (int64_t)(bh % a.H) * a.D; };
  union Frag { Vec u; T e[V]; };
  auto rotate = [&](const Frag& v1, const Frag& v2, T* q1) {
    Frag w1, w2;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      float o1, o2;
      rope_pair((float)v1.e[e], (float)v2.e[e], c[e], s[e], o1, o2);
      w1.e[e] = (T)o1;
      w2.e[e] = (T)o2;
    }
    *reinterpret_cast<Vec*>(q1) = w1.u;
    *reinterpret_cast<Vec*>(q1 + half) = w2.u;
  };
  if (MODE != 0 && nv == V) {
    // NB (batch, head) pairs per trip, all their loads issued before the first store: with x
    // and out possibly the same buffer the compiler cannot move a load above a store itself,
    // and one pair per trip leaves a lane waiting out a memory round trip per head.  The heads
    // of one trip are neighbours in the row, so a wave uses whole cache lines at once
    constexpr int NB = 4;
    for (int bh = blockIdx.y; bh < nbh; bh += NB * gy) {
      Frag f1[NB], f2[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const T* p = xptr(bh + j * gy < nbh ? bh + j * gy : bh);
        f1[j].u = *reinterpret_cast<const Vec*>(p);
        f2[j].u = *reinterpret_cast<const Vec*>(p + half);
      }
#pragma unroll
      for (int j = 0; j < NB; ++j)
        if (bh + j * gy < nbh) rotate(f1[j], f2[j], optr(bh + j * gy));
    }
    return;
  }
  for (int bh = blockIdx.y; bh < nbh; bh += gy) {
    const T* p1 = xptr(bh);
    T* q1 = optr(bh);
    float x1[V], x2[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      if (e < nv) {
        x1[e] = (float)p1[e];
        x2[e] = (float)p1[half + e];
      }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) {
      if (e < nv) {
        float o1, o2;
        rope_pair(x1[e], x2[e], c[e], s[e], o1, o2);
        q1[e] = (T)o1;
        q1[half + e] = (T)o2;
      }
    }
  }
}

template <int DT>
static int rope_apply_launch_dt(const RopeArgs& a, int mode, hipStream_t st) {
  const int half = a.D / 2;
  const int V = mode == 0 ? 1 : 16 / dt_traits<DT>::kBytes;
  if (mode == 1 && half % V) return -1;
  const int64_t nchunk = (half + V - 1) / V;
  const int64_t gx = ((int64_t)a.R * nchunk + 255) / 256;
  if (gx >= (1LL << 31)) return -1;
  // several waves on every CU (256 CUs, 4 waves per workgroup).  A lane walks the (batch, head)
  // pairs of its row itself while the rows alone fill the GPU: the heads of a row share cache
  // lines, and dealing them to workgroups of their own measured slower at R = 25000 (21.7 vs
  // 15.9 us).  Only short row counts (a rank's R = 3125) spread them over blockIdx.y
  const int64_t nbh = (int64_t)a.B * a.H;
  int64_t gy = (512 + gx - 1) / gx;
  gy = gy < 1 ? 1 : (gy > nbh ? nbh : gy);
  if (gy > 65535) gy = 65535;
  const dim3 grid((unsigned)gx, (unsigned)gy);
  if (mode == 1) hipLaunchKernelGGL((rope_apply_kernel<DT, 1>), grid, dim3(256), 0, st, a);
  else if (mode == 2) hipLaunchKernelGGL((rope_apply_kernel<DT, 2>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((rope_apply_kernel<DT, 0>), grid, dim3(256), 0, st, a);
  return 0;
}

}  // namespace xdot

extern "C" int xdot_rope_table_launch(float* cosb, float* sinb, const double* inv_freq, int R, int half, int64_t offset,
                                      hipStream_t st) {
  using namespace xdot;
  if (R < 0 || half < 1 || offset < 0 || offset + (int64_t)R > 2147483647LL) return -1;
  const int64_t total = (int64_t)R * half;
  if (total == 0) return 0;
  const int64_t g = (total + 255) / 256;
  if (g >= (1LL << 31)) return -1;
  hipLaunchKernelGGL(rope_table_kernel, dim3((unsigned)g), dim3(256), 0, st, cosb, sinb, inv_freq, total, half, offset);
  return 0;
}

extern "C" int xdot_rope_apply_launch(const xdot::RopeArgs* a, int dt, int mode, hipStream_t st) {
  using namespace xdot;
  if (a->B < 0 || a->R < 0 || a->H < 1 || a->D < 2 || (a->D & 1) || mode < 0 || mode > 2) return -1;
  if (a->B == 0 || a->R == 0) return 0;
  if (dt == DT_BF16) return rope_apply_launch_dt<DT_BF16>(*a, mode, st);
  if (dt == DT_F16) return rope_apply_launch_dt<DT_F16>(*a, mode, st);
  if (dt == DT_F32) return rope_apply_launch_dt<DT_F32>(*a, mode, st);
  return -1;
}
