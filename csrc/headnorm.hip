// xdot — QK-norm: RMSNorm over each head's D features of the projected k / q with a learnable (D,)
// gain, fused with the rotary pass of csrc/rope.hip (same pairs, same table, same expression).
//
//   r    = rsqrt(mean_j x[j]^2 + eps)           per (batch, row, head)
//   y[i] = x[i] * r * w[i]
//   out  = alpha * rotate(y)                    (rotation only with a table)
//
// Ownership is rope_apply_kernel's: a lane owns one chunk of V pair indices of one head row, i.e.
// x[i0, i0 + V) and x[D/2 + i0, D/2 + i0 + V) (V = 16 bytes of elements), lane 0 also the last
// element of an odd D.  The ceil(D/2V) lanes of a head row sit in a lane group of G lanes (the next
// power of two; idle lanes hold zeros), which reduces with __shfl_xor.  Order of operations, the
// same on the vector and the scalar path (a view's results do not depend on its alignment):
//   lane:   ss = fma(x, x, ss) over its first-half elements in order, then its second-half ones,
//           then the odd tail; group: log2 G butterfly levels; r = rsqrtf(ss * (1/D) + eps)
//   y = (x * r) * w; with a table rope_pair(y1, y2, cos * alpha, sin * alpha), without it
//   (x * r) * (w * alpha); one rounding to the output dtype.
// Backward, with gy = alpha * rotate^-1(g), xh = x * r, gw = gy * w:
//   dx[i] = r * (gw[i] - xh[i] * mean_j(gw[j] xh[j])),   dw[i] = sum over (b, row, head) gy[i] xh[i]
// dw is deterministic: a lane adds its head rows in loop order, a workgroup adds its lane groups in
// index order through LDS into ONE fp32 (D,) partial, and headnorm_dw_kernel adds the partials in a
// fixed order.  No atomics.
#include "common.h"

namespace xdot {

// (as csrc/rope.hip: the one expression of a rotated pair)
__device__ __forceinline__ void hn_rope_pair(float x1, float x2, float c, float s, float& o1, float& o2) {
  o1 = __builtin_fmaf(-x2, s, x1 * c);
  o2 = __builtin_fmaf(x1, s, x2 * c);
}

template <typename T> struct HnFrag {
  static constexpr int V = 16 / (int)sizeof(T);
  union { u32x4_ua u; T e[V]; };
};

// the chunk [p, p + nv) of a head row half: one 16-byte vector when whole, else element by element
template <typename T, bool VEC>
__device__ __forceinline__ void hn_load(HnFrag<T>& f, const T* p, int nv) {
  constexpr int V = HnFrag<T>::V;
  if (VEC && nv == V) {
    f.u = *reinterpret_cast<const u32x4_ua*>(p);
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e) f.e[e] = e < nv ? p[e] : (T)0.f;
  }
}
template <typename T, bool VEC>
__device__ __forceinline__ void hn_store(const HnFrag<T>& f, T* p, int nv) {
  constexpr int V = HnFrag<T>::V;
  if (VEC && nv == V) {
    *reinterpret_cast<u32x4_ua*>(p) = f.u;
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e)
      if (e < nv) p[e] = f.e[e];
  }
}

template <typename T> __device__ __forceinline__ float hn_gain(const HeadNormArgs& a, int i) {
  return a.w_f32 ? reinterpret_cast<const float*>(a.w)[i] : (float)reinterpret_cast<const T*>(a.w)[i];
}

__device__ __forceinline__ float hn_group_sum(float v, int G) {
  for (int o = G >> 1; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// what a lane keeps of its position: chunk start, valid pairs, whether it owns the odd tail
struct HnLane { int i0, nv, tail; };

template <int V> __device__ __forceinline__ HnLane hn_lane(const HeadNormArgs& a, int ch) {
  const int half = a.D >> 1;
  HnLane l;
  l.i0 = ch * V;
  const int left = half - l.i0;
  l.nv = left < 0 ? 0 : (left < V ? left : V);
  l.tail = (a.D & 1) && ch == 0;
  return l;
}

template <int DT, bool VEC, bool ROT>
__global__ __launch_bounds__(256) void headnorm_fwd_kernel(HeadNormArgs a, int G) {
  using T = typename dt_traits<DT>::T;
  using Frag = HnFrag<T>;
  constexpr int V = Frag::V;
  const int half = a.D >> 1;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = t / G;
  if (row >= a.R) return;  // whole lane groups leave together
  const HnLane l = hn_lane<V>(a, (int)(t & (G - 1)));
  float w1[V], w2[V], c[V], s[V], wt = 0.f;
#pragma unroll
  for (int e = 0; e < V; ++e) {
    w1[e] = e < l.nv ? hn_gain<T>(a, l.i0 + e) : 0.f;
    w2[e] = e < l.nv ? hn_gain<T>(a, half + l.i0 + e) : 0.f;
    if constexpr (ROT) {
      c[e] = e < l.nv ? a.cos[row * half + l.i0 + e] * a.alpha : 0.f;
      s[e] = e < l.nv ? a.sin[row * half + l.i0 + e] * a.alpha : 0.f;
    } else {
      w1[e] *= a.alpha;
      w2[e] *= a.alpha;
    }
  }
  if (l.tail) wt = hn_gain<T>(a, a.D - 1) * a.alpha;
  const T* xrow = reinterpret_cast<const T*>(a.x) + row * a.xs_r;
  T* orow = reinterpret_cast<T*>(a.out) + row * a.os_r;
  T* save = reinterpret_cast<T*>(a.save);
  const int nbh = a.B * a.H, gy = (int)gridDim.y;
  // NB (batch, head) pairs per trip, all their loads issued before the first store (out may be x;
  // as rope_apply_kernel)
  constexpr int NB = 2;
  for (int bh0 = blockIdx.y; bh0 < nbh; bh0 += NB * gy) {
    Frag f1[NB], f2[NB];
    T xt[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int bh = bh0 + j * gy < nbh ? bh0 + j * gy : bh0;
      const T* p = xrow + (bh / a.H) * a.xs_b + (int64_t)(bh % a.H) * a.D;
      hn_load<T, VEC>(f1[j], p + l.i0, l.nv);
      hn_load<T, VEC>(f2[j], p + half + l.i0, l.nv);
      xt[j] = l.tail ? p[a.D - 1] : (T)0.f;
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int bh = bh0 + j * gy;
      if (bh >= nbh) break;  // (uniform over the workgroup)
      const int b = bh / a.H, h = bh % a.H;
      const int64_t hrow = ((int64_t)b * a.R + row) * a.H + h;
      if (save != nullptr) {
        T* sp = save + hrow * a.D;
        hn_store<T, VEC>(f1[j], sp + l.i0, l.nv);
        hn_store<T, VEC>(f2[j], sp + half + l.i0, l.nv);
        if (l.tail) sp[a.D - 1] = xt[j];
      }
      float ss = 0.f;
#pragma unroll
      for (int e = 0; e < V; ++e) ss = __builtin_fmaf((float)f1[j].e[e], (float)f1[j].e[e], ss);
#pragma unroll
      for (int e = 0; e < V; ++e) ss = __builtin_fmaf((float)f2[j].e[e], (float)f2[j].e[e], ss);
      ss = __builtin_fmaf((float)xt[j], (float)xt[j], ss);
      ss = hn_group_sum(ss, G);
      const float r = rsqrtf(__builtin_fmaf(ss, a.inv_d, a.eps));
      Frag o1, o2;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float y1 = ((float)f1[j].e[e] * r) * w1[e], y2 = ((float)f2[j].e[e] * r) * w2[e];
        if constexpr (ROT) {
          float q1, q2;
          hn_rope_pair(y1, y2, c[e], s[e], q1, q2);
          o1.e[e] = (T)q1;
          o2.e[e] = (T)q2;
        } else {
          o1.e[e] = (T)y1;
          o2.e[e] = (T)y2;
        }
      }
      T* q = orow + b * a.os_b + (int64_t)h * a.D;
      hn_store<T, VEC>(o1, q + l.i0, l.nv);
      hn_store<T, VEC>(o2, q + half + l.i0, l.nv);
      if (l.tail) q[a.D - 1] = (T)(((float)xt[j] * r) * wt);
      if ((t & (G - 1)) == 0) a.rstd[hrow] = r;
    }
  }
}

// LDS of the backward: one (D,) row of accumulators per lane group, rows_per_wg = 256 / G of them.
// xdot_headnorm_plan admits D / 2 <= V G (G <= 64: one wave reduces a head row), so D <= 2 V G + 1 and
// rows_per_wg * D <= 256 * 2 V + 256 / G <= 512 V + 256 floats, V <= 8 (16-bit elements)
constexpr int kHnMaxV = 8;
constexpr int kHnLds = 512 * kHnMaxV + 256;
static_assert(16 / dt_traits<DT_BF16>::kBytes <= kHnMaxV && 16 / dt_traits<DT_F16>::kBytes <= kHnMaxV &&
                  16 / dt_traits<DT_F32>::kBytes <= kHnMaxV,
              "kHnLds is sized for at most kHnMaxV elements per 16-byte vector");

template <int DT, bool VEC, bool ROT>
__global__ __launch_bounds__(256) void headnorm_bwd_kernel(HeadNormArgs a, int G) {
  using T = typename dt_traits<DT>::T;
  using Frag = HnFrag<T>;
  constexpr int V = Frag::V;
  __shared__ float lds[kHnLds];
  const int half = a.D >> 1;
  const int rpw = 256 / G, grp = threadIdx.x / G;
  const HnLane l = hn_lane<V>(a, threadIdx.x & (G - 1));
  float w1[V], w2[V], acc1[V], acc2[V], wt = 0.f, acct = 0.f;
#pragma unroll
  for (int e = 0; e < V; ++e) {
    w1[e] = e < l.nv ? hn_gain<T>(a, l.i0 + e) : 0.f;
    w2[e] = e < l.nv ? hn_gain<T>(a, half + l.i0 + e) : 0.f;
    acc1[e] = acc2[e] = 0.f;
  }
  if (l.tail) wt = hn_gain<T>(a, a.D - 1);
  const int nbh = a.B * a.H, gy = (int)gridDim.y;
  const int64_t nrg = ((int64_t)a.R + rpw - 1) / rpw;
  for (int64_t rg = blockIdx.x; rg < nrg; rg += gridDim.x) {
    const int64_t row = rg * rpw + grp;
    if (row >= a.R) continue;  // a whole lane group
    float c[V], s[V];
    if constexpr (ROT) {
#pragma unroll
      for (int e = 0; e < V; ++e) {  // the inverse rotation: -sin
        c[e] = e < l.nv ? a.cos[row * half + l.i0 + e] * a.alpha : 0.f;
        s[e] = e < l.nv ? a.sin[row * half + l.i0 + e] * -a.alpha : 0.f;
      }
    }
    const T* xrow = reinterpret_cast<const T*>(a.x) + row * a.xs_r;
    const T* grow = reinterpret_cast<const T*>(a.g) + row * a.gs_r;
    T* orow = reinterpret_cast<T*>(a.out) + row * a.os_r;
    for (int bh = blockIdx.y; bh < nbh; bh += gy) {
      const int b = bh / a.H, h = bh % a.H;
      const T* xp = xrow + b * a.xs_b + (int64_t)h * a.D;
      const T* gp = grow + b * a.gs_b + (int64_t)h * a.D;
      Frag x1, x2, g1, g2, o1, o2;
      hn_load<T, VEC>(x1, xp + l.i0, l.nv);
      hn_load<T, VEC>(x2, xp + half + l.i0, l.nv);
      hn_load<T, VEC>(g1, gp + l.i0, l.nv);
      hn_load<T, VEC>(g2, gp + half + l.i0, l.nv);
      const float xt = l.tail ? (float)xp[a.D - 1] : 0.f, gt = l.tail ? (float)gp[a.D - 1] : 0.f;
      const float r = a.rstd[((int64_t)b * a.R + row) * a.H + h];
      float gy1[V], gy2[V], xh1[V], xh2[V], p = 0.f;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        if constexpr (ROT) {
          hn_rope_pair((float)g1.e[e], (float)g2.e[e], c[e], s[e], gy1[e], gy2[e]);
        } else {
          gy1[e] = (float)g1.e[e] * a.alpha;
          gy2[e] = (float)g2.e[e] * a.alpha;
        }
        xh1[e] = (float)x1.e[e] * r;
        xh2[e] = (float)x2.e[e] * r;
      }
      const float gyt = gt * a.alpha, xht = xt * r;
#pragma unroll
      for (int e = 0; e < V; ++e) p = __builtin_fmaf(gy1[e] * w1[e], xh1[e], p);
#pragma unroll
      for (int e = 0; e < V; ++e) p = __builtin_fmaf(gy2[e] * w2[e], xh2[e], p);
      p = __builtin_fmaf(gyt * wt, xht, p);
      const float m = hn_group_sum(p, G) * a.inv_d;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        o1.e[e] = (T)(__builtin_fmaf(-xh1[e], m, gy1[e] * w1[e]) * r);
        o2.e[e] = (T)(__builtin_fmaf(-xh2[e], m, gy2[e] * w2[e]) * r);
        acc1[e] = __builtin_fmaf(gy1[e], xh1[e], acc1[e]);
        acc2[e] = __builtin_fmaf(gy2[e], xh2[e], acc2[e]);
      }
      acct = __builtin_fmaf(gyt, xht, acct);
      T* q = orow + b * a.os_b + (int64_t)h * a.D;
      hn_store<T, VEC>(o1, q + l.i0, l.nv);
      hn_store<T, VEC>(o2, q + half + l.i0, l.nv);
      if (l.tail) q[a.D - 1] = (T)(__builtin_fmaf(-xht, m, gyt * wt) * r);
    }
  }
  // the workgroup's partial: lane groups added in index order
  float* mine = lds + grp * a.D;
#pragma unroll
  for (int e = 0; e < V; ++e) {
    if (e < l.nv) {
      mine[l.i0 + e] = acc1[e];
      mine[half + l.i0 + e] = acc2[e];
    }
  }
  if (l.tail) mine[a.D - 1] = acct;
  __syncthreads();
  float* part = a.part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * a.D;
  for (int i = threadIdx.x; i < a.D; i += 256) {
    float v = lds[i];
    for (int k = 1; k < rpw; ++k) v += lds[k * a.D + i];
    part[i] = v;
  }
}

// dw[i] = the partials of column i added in a fixed order: 32 strided chains p = j, j + 32, ...
// (independent loads), then the 32 chain sums in order; one rounding to the output dtype
template <typename TO>
__global__ __launch_bounds__(1024) void headnorm_dw_kernel(const float* __restrict__ part, TO* __restrict__ dw, int nparts,
                                                            int D) {
  __shared__ float lds[32][33];
  const int i = blockIdx.x * 32 + threadIdx.x, j = threadIdx.y;
  float v = 0.f;
  if (i < D)
    for (int p = j; p < nparts; p += 32) v += part[(int64_t)p * D + i];
  lds[j][threadIdx.x] = v;
  __syncthreads();
  if (j == 0 && i < D) {
    float sum = lds[0][threadIdx.x];
    for (int k = 1; k < 32; ++k) sum += lds[k][threadIdx.x];
    dw[i] = (TO)sum;
  }
}

template <int DT>
static int headnorm_launch_dt(const HeadNormArgs& a, bool bwd, int vec, hipStream_t st) {
  HeadNormPlan p;
  // the only way to the kernels: they rely on the plan's G (a power of two <= 64 that divides 256)
  if (xdot_headnorm_plan(a.B, a.R, a.H, a.D, dt_traits<DT>::kBytes, &p)) return -1;
  const bool rot = a.cos != nullptr;
  const dim3 grid(bwd ? p.bwd_gx : p.fwd_gx, bwd ? p.bwd_gy : p.fwd_gy);
#define XDOT_HN_LAUNCH(K)                                                                             \
  do {                                                                                                \
    if (vec && rot) hipLaunchKernelGGL((K<DT, true, true>), grid, dim3(256), 0, st, a, p.G);           \
    else if (vec) hipLaunchKernelGGL((K<DT, true, false>), grid, dim3(256), 0, st, a, p.G);            \
    else if (rot) hipLaunchKernelGGL((K<DT, false, true>), grid, dim3(256), 0, st, a, p.G);            \
    else hipLaunchKernelGGL((K<DT, false, false>), grid, dim3(256), 0, st, a, p.G);                    \
  } while (0)
  if (bwd) XDOT_HN_LAUNCH(headnorm_bwd_kernel);
  else XDOT_HN_LAUNCH(headnorm_fwd_kernel);
#undef XDOT_HN_LAUNCH
  return 0;
}

static int headnorm_launch(const HeadNormArgs* a, bool bwd, int dt, int vec, hipStream_t st) {
  if (a->B < 0 || a->R < 0 || a->H < 1 || a->D < 1) return -1;
  if (a->cos != nullptr && (a->D & 1)) return -1;
  if (a->B == 0 || a->R == 0) return 0;
  if (dt == DT_BF16) return headnorm_launch_dt<DT_BF16>(*a, bwd, vec, st);
  if (dt == DT_F16) return headnorm_launch_dt<DT_F16>(*a, bwd, vec, st);
  if (dt == DT_F32) return headnorm_launch_dt<DT_F32>(*a, bwd, vec, st);
  return -1;
}

}  // namespace xdot

extern "C" int xdot_headnorm_plan(int B, int R, int H, int D, int esize, xdot::HeadNormPlan* p) {
  if (B < 1 || R < 1 || H < 1 || D < 1 || (esize != 2 && esize != 4)) return -1;
  const int V = 16 / esize;
  const int nchunk = D / 2 < V ? 1 : (D / 2 + V - 1) / V;
  int G = 1;
  while (G < nchunk) G <<= 1;
  if (G > 64) return -1;  // a head row is reduced inside one wave
  p->G = G;
  p->rows_per_wg = 256 / G;
  const int64_t nbh = (int64_t)B * H;
  const int64_t nrg = ((int64_t)R + p->rows_per_wg - 1) / p->rows_per_wg;
  if (nrg >= (1LL << 31)) return -1;
  // as rope_apply_launch_dt: the rows alone fill the GPU at long R (a lane walks the heads of its
  // row, which share cache lines); only short row counts spread the heads over blockIdx.y
  auto heads = [&](int64_t gx) {
    int64_t gy = (512 + gx - 1) / gx;
    gy = gy < 1 ? 1 : (gy > nbh ? nbh : gy);
    return (int)(gy > 65535 ? 65535 : gy);
  };
  p->fwd_gx = (int)nrg;
  p->fwd_gy = heads(nrg);
  // the backward's workgroups walk the row groups, so that at most 1024 (D,) partials are written
  p->bwd_gx = (int)(nrg > 1024 ? 1024 : nrg);
  p->bwd_gy = heads(p->bwd_gx);
  return 0;
}

extern "C" int xdot_headnorm_fwd_launch(const xdot::HeadNormArgs* a, int dt, int vec, hipStream_t st) {
  return xdot::headnorm_launch(a, false, dt, vec, st);
}

extern "C" int xdot_headnorm_bwd_launch(const xdot::HeadNormArgs* a, int dt, int vec, hipStream_t st) {
  if (a->part == nullptr) return -1;
  return xdot::headnorm_launch(a, true, dt, vec, st);
}

extern "C" int xdot_headnorm_dw_launch(const float* part, void* dw, int nparts, int D, int dto, hipStream_t st) {
  using namespace xdot;
  if (nparts < 1 || D < 1) return -1;
  const dim3 grid((D + 31) / 32), block(32, 32);
  if (dto == DT_F32) hipLaunchKernelGGL(headnorm_dw_kernel<float>, grid, block, 0, st, part, (float*)dw, nparts, D);
  else if (dto == DT_BF16) hipLaunchKernelGGL(headnorm_dw_kernel<__bf16>, grid, block, 0, st, part, (__bf16*)dw, nparts, D);
  else if (dto == DT_F16) hipLaunchKernelGGL(headnorm_dw_kernel<_Float16>, grid, block, 0, st, part, (_Float16*)dw, nparts, D);
  else return -1;
  return 0;
}
