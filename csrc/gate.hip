// xdot — gated attention: a query-dependent sigmoid gate on the merged attention output, before the
// output projection (Qiu et al. 2025; Qwen3-Next):
//   o' = o * sigmoid(g)        o: (B, R, H*D), g: (B, R, H*D) (elementwise) or (B, R, H) (headwise:
//                              one value per head row, broadcast over its D features)
// The flash kernels know nothing about it: every forward path ends in a finished o and every backward
// starts from do, and the gate is one pass each way on those tensors.  The sigmoid is evaluated in a
// form that cannot overflow or cancel, from e = exp(-|g|) <= 1 and r = 1 / (1 + e):
//   sigma = g >= 0 ? r : e r,     sigma' = e r^2      (never sigma - sigma^2, never 1.f - sigma)
// gate_apply  (one launch, out of place: the attention keeps its own o for delta) is a plain IEEE
//   product: NaN in o stays NaN, g = -inf gives +-0, g = +inf gives o bit for bit.
// gate_backward (one launch): do = do' * sigma (may be written over do'), and
//   elementwise  dg = do' * o * sigma'
//   headwise     dg = (sum over the head's D features of do' * o) * sigma', the sum in fp32 in a fixed
//                order inside ONE wave (no atomics: bitwise reproducible), rounded once.
// Both are bandwidth bound: fp32 math, one rounding to the tensor dtype, 16-byte loads and stores
// where D, the strides and the pointers allow (VEC), one element per lane step otherwise.
#include "common.h"

namespace xdot {

__device__ __forceinline__ void gate_sigmoid(float g, float& e, float& r, float& sig) {
  e = expf(-fabsf(g));
  r = 1.f / (1.f + e);
  sig = g >= 0.f ? r : e * r;
}

// a * sigma as the IEEE product gives it, sigma >= 0: a zero result carries a's sign whatever the
// compiler makes of the product (a mixed-precision fma with a +0 addend turns -0 into +0)
__device__ __forceinline__ float gate_mul(float a, float sig) {
  const float p = a * sig;
  return p == 0.f ? __builtin_copysignf(0.f, a) : p;
}

// one lane step: 16 bytes (VEC) or one element
template <typename T, bool VEC> struct GateFrag;
template <typename T> struct GateFrag<T, true> {
  static constexpr int V = 16 / (int)sizeof(T);
  union { u32x4 u; T e[V]; };
  __device__ __forceinline__ void load(const T* p) { u = *reinterpret_cast<const u32x4*>(p); }
  __device__ __forceinline__ void store(T* p) const { *reinterpret_cast<u32x4*>(p) = u; }
};
template <typename T> struct GateFrag<T, false> {
  static constexpr int V = 1;
  T e[1];
  __device__ __forceinline__ void load(const T* p) { e[0] = *p; }
  __device__ __forceinline__ void store(T* p) const { *p = e[0]; }
};

// The L lanes li = 0 .. L-1 of one head row (any L <= 64, consecutive lanes of one wave): lane 0 gets
// their sum, by halving: lanes [half, w) are added onto lanes [0, w - half), w -> half = ceil(w / 2).
// A fixed order for a given L; at most 6 levels.  Every lane of the wave executes it.
__device__ __forceinline__ float gate_row_sum(float v, int li, int L) {
  for (int w = L; w > 1;) {
    const int half = (w + 1) >> 1;
    const float t = __shfl_down(v, half, kWave);
    if (li + half < w) v += t;
    w = half;
  }
  return v;
}

// Lane layout of csrc/sink.hip: a head row (b, row, h) is nch = D / V lane steps, L = min(nch, 64)
// lanes of ONE wave own it (a lane walks steps li, li + L, ...), G = 64 / L head rows sit side by
// side in a wave, and a wave takes U such groups.  The 64 % L lanes left over idle on item 0.
struct GateItem {
  int64_t o, y, g, d;  // element offsets of the head row in o, y, g (headwise: of its one value), dy
  bool on;
};
__device__ __forceinline__ GateItem gate_item(const GateArgs& a, int64_t u, int64_t items, bool lane_on) {
  GateItem it;
  it.on = lane_on && u < items;
  const int64_t uu = it.on ? u : 0;
  const int h = (int)(uu % a.H);
  const int64_t br = uu / a.H;
  const int64_t b = br / a.R, row = br - b * a.R;
  it.o = b * a.os_b + row * a.os_r + (int64_t)h * a.D;
  it.y = b * a.ys_b + row * a.ys_r + (int64_t)h * a.D;
  it.d = b * a.ds_b + row * a.ds_r + (int64_t)h * a.D;
  it.g = b * a.gs_b + row * a.gs_r + (a.headwise ? (int64_t)h : (int64_t)h * a.D);
  return it;
}

template <int DT, bool VEC>
__global__ __launch_bounds__(256) void gate_apply_kernel(GateArgs a) {
  using T = typename dt_traits<DT>::T;
  using Frag = GateFrag<T, VEC>;
  constexpr int V = Frag::V;
  constexpr int U = 4;
  const int nch = a.D / V;
  const int L = nch < kWave ? nch : kWave;
  const int G = kWave / L;
  const int lane = threadIdx.x & (kWave - 1);
  const int grp = lane / L;
  const bool lane_on = grp < G;
  const int li = lane_on ? lane - grp * L : 0;
  const int64_t items = (int64_t)a.B * a.R * a.H;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t u0 = wave * (int64_t)(U * G) + (lane_on ? grp : 0);
  const T* op = reinterpret_cast<const T*>(a.o);
  const T* gp = reinterpret_cast<const T*>(a.g);
  T* yp = reinterpret_cast<T*>(a.y);
  GateItem it[U];
#pragma unroll
  for (int i = 0; i < U; ++i) it[i] = gate_item(a, u0 + (int64_t)i * G, items, lane_on);
  auto apply = [&](const Frag& f, const Frag& gf, float hsig, T* q) {
    Frag w;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float sig = hsig;
      if (!a.headwise) {
        float e, r;
        gate_sigmoid((float)gf.e[k], e, r, sig);
      }
      w.e[k] = (T)gate_mul((float)f.e[k], sig);
    }
    w.store(q);
  };
  if (nch <= kWave) {
    // one step per lane: the U loads are issued before the first store
    Frag f[U], gf[U];
    float gh[U];
#pragma unroll
    for (int i = 0; i < U; ++i) {
      f[i].load(op + it[i].o + li * V);  // (past the end: item 0)
      if (a.headwise) gh[i] = (float)gp[it[i].g];
      else gf[i].load(gp + it[i].g + li * V);
    }
#pragma unroll
    for (int i = 0; i < U; ++i) {
      if (!it[i].on) continue;
      float e, r, sig = 0.f;
      if (a.headwise) gate_sigmoid(gh[i], e, r, sig);
      apply(f[i], gf[i], sig, yp + it[i].y + li * V);
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < U; ++i) {
    if (!it[i].on) continue;
    float e, r, sig = 0.f;
    if (a.headwise) gate_sigmoid((float)gp[it[i].g], e, r, sig);
    for (int j = li; j < nch; j += L) {
      Frag f, gf;
      f.load(op + it[i].o + j * V);
      if (!a.headwise) gf.load(gp + it[i].g + j * V);
      apply(f, gf, sig, yp + it[i].y + j * V);
    }
  }
}

// y = do (strides ys; may be the memory of dy), dg contiguous: (B, R, H*D) or (B, R, H)
template <int DT, bool VEC>
__global__ __launch_bounds__(256) void gate_backward_kernel(GateArgs a) {
  using T = typename dt_traits<DT>::T;
  using Frag = GateFrag<T, VEC>;
  constexpr int V = Frag::V;
  constexpr int U = 2;
  const int nch = a.D / V;
  const int L = nch < kWave ? nch : kWave;
  const int G = kWave / L;
  const int lane = threadIdx.x & (kWave - 1);
  const int grp = lane / L;
  const bool lane_on = grp < G;
  const int li = lane_on ? lane - grp * L : 0;
  const int64_t items = (int64_t)a.B * a.R * a.H;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t u0 = wave * (int64_t)(U * G) + (lane_on ? grp : 0);
  const T* op = reinterpret_cast<const T*>(a.o);
  const T* gp = reinterpret_cast<const T*>(a.g);
  const T* dp = reinterpret_cast<const T*>(a.dy);
  T* yp = reinterpret_cast<T*>(a.y);
  T* dgp = reinterpret_cast<T*>(a.dg);
  const int64_t C = (int64_t)a.H * a.D;
  GateItem it[U];
  int64_t dgo[U];  // element offset of the head row in the contiguous dg
#pragma unroll
  for (int i = 0; i < U; ++i) {
    const int64_t u = u0 + (int64_t)i * G;
    it[i] = gate_item(a, u, items, lane_on);
    const int64_t uu = it[i].on ? u : 0;
    dgo[i] = a.headwise ? uu : (uu / a.H) * C + (uu % a.H) * (int64_t)a.D;
  }
  // one lane step: do = dy * sigma stored, dg stored (elementwise) or dy * o added to acc (headwise)
  auto step = [&](const Frag& d, const Frag& f, const Frag& gf, float hsig, T* qdo, T* qdg, float& acc) {
    Frag w, wg;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float dy = (float)d.e[k], o = (float)f.e[k];
      float sig = hsig;
      if (!a.headwise) {
        float e, r;
        gate_sigmoid((float)gf.e[k], e, r, sig);
        wg.e[k] = (T)(dy * o * (e * r * r));
      } else {
        acc += dy * o;
      }
      w.e[k] = (T)gate_mul(dy, sig);
    }
    w.store(qdo);
    if (!a.headwise) wg.store(qdg);
  };
  if (nch <= kWave) {
    // one step per lane; every load is issued before the first store (do may overwrite dy)
    Frag d[U], f[U], gf[U];
    float gh[U];
#pragma unroll
    for (int i = 0; i < U; ++i) {
      d[i].load(dp + it[i].d + li * V);
      f[i].load(op + it[i].o + li * V);
      if (a.headwise) gh[i] = (float)gp[it[i].g];
      else gf[i].load(gp + it[i].g + li * V);
    }
#pragma unroll
    for (int i = 0; i < U; ++i) {
      float e = 0.f, r = 0.f, sig = 0.f, acc = 0.f;
      if (a.headwise) gate_sigmoid(gh[i], e, r, sig);
      if (it[i].on) step(d[i], f[i], gf[i], sig, yp + it[i].y + li * V, dgp + dgo[i] + li * V, acc);
      if (a.headwise) {  // (all 64 lanes take part in the shuffles)
        const float tot = gate_row_sum(acc, li, L);
        if (it[i].on && li == 0) dgp[dgo[i]] = (T)(tot * (e * r * r));
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < U; ++i) {
    float e = 0.f, r = 0.f, sig = 0.f, acc = 0.f;
    if (a.headwise) gate_sigmoid((float)gp[it[i].g], e, r, sig);
    if (it[i].on) {
      for (int j = li; j < nch; j += L) {
        Frag d, f, gf;
        d.load(dp + it[i].d + j * V);
        f.load(op + it[i].o + j * V);
        if (!a.headwise) gf.load(gp + it[i].g + j * V);
        step(d, f, gf, sig, yp + it[i].y + j * V, dgp + dgo[i] + j * V, acc);
      }
    }
    if (a.headwise) {
      const float tot = gate_row_sum(acc, li, L);
      if (it[i].on && li == 0) dgp[dgo[i]] = (T)(tot * (e * r * r));
    }
  }
}

template <int DT, bool VEC>
static int gate_launch_dt(const GateArgs& a, bool bwd, hipStream_t st) {
  constexpr int V = VEC ? 16 / dt_traits<DT>::kBytes : 1;
  if (a.D % V) return -1;
  const int nch = a.D / V;
  const int L = nch < kWave ? nch : kWave;
  const int64_t per_wave = (bwd ? 2 : 4) * (kWave / L);  // U * G head rows
  const int64_t items = (int64_t)a.B * a.R * a.H;
  const int64_t waves = (items + per_wave - 1) / per_wave;
  const int64_t gx = (waves + 3) / 4;
  if (gx >= (1LL << 31)) return -1;
  if (bwd) hipLaunchKernelGGL((gate_backward_kernel<DT, VEC>), dim3((unsigned)gx), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((gate_apply_kernel<DT, VEC>), dim3((unsigned)gx), dim3(256), 0, st, a);
  return 0;
}

static int gate_launch(const GateArgs& a, int dt, int vec, bool bwd, hipStream_t st) {
  if (a.B < 0 || a.R < 0 || a.H < 1 || a.D < 1 || (a.headwise != 0 && a.headwise != 1)) return -1;
  if (a.B == 0 || a.R == 0) return 0;
  if (!a.o || !a.g || !a.y || (bwd && (!a.dy || !a.dg))) return -1;
  if (dt == DT_BF16) return vec ? gate_launch_dt<DT_BF16, true>(a, bwd, st) : gate_launch_dt<DT_BF16, false>(a, bwd, st);
  if (dt == DT_F16) return vec ? gate_launch_dt<DT_F16, true>(a, bwd, st) : gate_launch_dt<DT_F16, false>(a, bwd, st);
  if (dt == DT_F32) return vec ? gate_launch_dt<DT_F32, true>(a, bwd, st) : gate_launch_dt<DT_F32, false>(a, bwd, st);
  return -1;
}

}  // namespace xdot

extern "C" int xdot_gate_apply_launch(const xdot::GateArgs* a, int dt, int vec, hipStream_t st) {
  return xdot::gate_launch(*a, dt, vec, false, st);
}

extern "C" int xdot_gate_backward_launch(const xdot::GateArgs* a, int dt, int vec, hipStream_t st) {
  return xdot::gate_launch(*a, dt, vec, true, st);
}
