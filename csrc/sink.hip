// xdot — attention sinks: one learnable logit s_h per row head that joins the softmax denominator
// and carries no value (StreamingLLM / gpt-oss).  The logit is NOT scaled by 1/sqrt(d): it is
// appended after mask and scale.  The flash kernels know nothing about it: every forward path ends
// in a normalised out (B, R, H*D) and a natural-log lse (B, H, R), and the sink is a fold on that
// pair, in place:
//   lse' = logaddexp(lse, s_h) = max(lse, s_h) + log1p(exp(-|lse - s_h|))
//   out' = g * out,  g = exp(lse - lse') = sigmoid(lse - s_h)
// A fully masked row (lse = -inf; the flash kernels write NaN into out there) gets out' = 0 by
// SELECTION and lse' = s_h exactly.  s_h = -inf writes nothing: out and lse stay as they are, bit
// for bit.  The unchanged backward kernels on (out', lse') give dk, dq, dv; the sink's own gradient
// is the small reduction
//   ds_h = -sum_{b, r} exp(s_h - lse'[b, h, r]) * delta'[b, h, r],  delta' = rowsum(dO . out')
// summed in a fixed order (no atomics: bitwise reproducible).  Both kernels are bandwidth bound:
// fp32 math, 16-byte loads and stores, one rounding to the tensor dtype.
#include "common.h"

namespace xdot {

__device__ __forceinline__ float sink_load(const void* p, int dt, int h) {
  if (dt == DT_F32) return reinterpret_cast<const float*>(p)[h];
  if (dt == DT_BF16) return (float)reinterpret_cast<const __bf16*>(p)[h];
  return (float)reinterpret_cast<const _Float16*>(p)[h];
}

// (g, lse') of one row from (lse, s), s > -inf.  e = exp(-|x|) <= 1, so nothing overflows at any
// |x|; lse = -inf gives e = 0, g = 0 and lse' = s + 0 = s exactly
__device__ __forceinline__ void sink_gate(float l, float s, float& g, float& l2) {
  const float x = l - s;
  const float e = expf(-fabsf(x));
  const float r = 1.f / (1.f + e);
  g = x >= 0.f ? r : e * r;
  l2 = fmaxf(l, s) + log1pf(e);
}

// A head row (b, row, h) is D / V 16-byte chunks.  L = min(D / V, 64) lanes of ONE wave own it (a
// lane walks chunks li, li + L, ...), G = 64 / L head rows sit side by side in a wave, and a wave
// takes U such groups.  lse is updated in place: every lane of the head row loads its lse with one
// instruction, and lane 0 of the group stores lse' afterwards -- the readers and the writer of one
// element are lanes of one wave in program order, and no other wave touches it.
template <int DT>
__global__ __launch_bounds__(256) void sink_fold_kernel(SinkArgs a) {
  using T = typename dt_traits<DT>::T;
  constexpr int V = 16 / (int)sizeof(T);
  constexpr int U = 4;
  union Frag { u32x4 u; T e[V]; };
  const int nch = a.D / V;
  const int L = nch < kWave ? nch : kWave;
  const int G = kWave / L;
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / L, li = lane - g * L;
  if (g >= G) return;  // 64 % L idle lanes (no cross-lane operation below)
  const int64_t items = (int64_t)a.B * a.R * a.H;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t u0 = wave * (int64_t)(U * G) + g;
  T* optr[U];
  float* lptr[U];
  float l[U], s[U];
  bool on[U];
#pragma unroll
  for (int i = 0; i < U; ++i) {
    const int64_t u = u0 + (int64_t)i * G;
    on[i] = u < items;
    const int64_t uu = on[i] ? u : 0;
    const int h = (int)(uu % a.H);
    const int64_t br = uu / a.H;
    const int64_t b = br / a.R, row = br - b * a.R;
    optr[i] = reinterpret_cast<T*>(a.out) + b * a.os_b + row * a.os_r + (int64_t)h * a.D;
    lptr[i] = a.lse + (b * a.H + h) * (int64_t)a.R + row;
    s[i] = sink_load(a.sinks, a.s_dt, h);
    l[i] = *lptr[i];
    on[i] = on[i] && s[i] != -__builtin_inff();  // no sink on this head: nothing is written
  }
  auto fold = [&](const Frag& f, float gate, bool dead, T* q) {
    Frag w;
#pragma unroll
    for (int e = 0; e < V; ++e) w.e[e] = dead ? (T)0.f : (T)(gate * (float)f.e[e]);
    *reinterpret_cast<u32x4*>(q) = w.u;
  };
  if (nch <= kWave) {
    // one chunk per lane: the U loads are issued before the first store (in place, the compiler
    // may not move a load above a store itself)
    Frag f[U];
#pragma unroll
    for (int i = 0; i < U; ++i) f[i].u = *reinterpret_cast<const u32x4*>(optr[i] + li * V);  // (past the end: item 0)
#pragma unroll
    for (int i = 0; i < U; ++i) {
      if (!on[i]) continue;
      float gate, l2;
      sink_gate(l[i], s[i], gate, l2);
      fold(f[i], gate, l[i] == -__builtin_inff(), optr[i] + li * V);
      if (li == 0) *lptr[i] = l2;
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < U; ++i) {
    if (!on[i]) continue;
    float gate, l2;
    sink_gate(l[i], s[i], gate, l2);
    const bool dead = l[i] == -__builtin_inff();
    for (int j = li; j < nch; j += L) {
      Frag f;
      f.u = *reinterpret_cast<const u32x4*>(optr[i] + j * V);
      fold(f, gate, dead, optr[i] + j * V);
    }
    if (li == 0) *lptr[i] = l2;
  }
}

template <int DT>
static int sink_fold_launch_dt(const SinkArgs& a, hipStream_t st) {
  constexpr int V = 16 / dt_traits<DT>::kBytes;
  if (a.D % V) return -1;
  const int nch = a.D / V;
  const int L = nch < kWave ? nch : kWave;
  const int64_t per_wave = 4 * (kWave / L);  // U * G head rows
  const int64_t items = (int64_t)a.B * a.R * a.H;
  const int64_t waves = (items + per_wave - 1) / per_wave;
  const int64_t gx = (waves + 3) / 4;
  if (gx >= (1LL << 31)) return -1;
  hipLaunchKernelGGL((sink_fold_kernel<DT>), dim3((unsigned)gx), dim3(256), 0, st, a);
  return 0;
}

// ---- ds ------------------------------------------------------------------------------------------
constexpr int kSinkChunk = 1024;  // (b, r) elements of one head per workgroup: 4 per thread

// the 256 threads' values -> their sum in thread 0, in a fixed order: the xor butterfly inside each
// wave, then the four waves in wave order
__device__ __forceinline__ float sink_block_sum(float v, float* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// workgroup (c, h): elements [c * 1024, (c + 1) * 1024) of head h's B * R rows (i = b * R + r)
__global__ __launch_bounds__(256) void sink_grad_part_kernel(SinkGradArgs a) {
  __shared__ float sh[4];
  const int h = blockIdx.y;
  const float s = sink_load(a.sinks, a.s_dt, h);
  const int64_t n = (int64_t)a.B * a.R;
  const int64_t base = (int64_t)blockIdx.x * kSinkChunk + threadIdx.x;
  float d[4], l[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = base + k * 256;
    const int64_t ii = i < n ? i : 0;
    const int64_t b = ii / a.R, r = ii - b * a.R;
    const int64_t at = (b * a.H + h) * (int64_t)a.R + r;
    d[k] = a.delta[at];
    l[k] = a.lse[at];
  }
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    // s = -inf: no sink, no gradient (and no exp(-inf + inf)); else lse' >= s: the weight is <= 1
    const bool live = base + k * 256 < n && s != -__builtin_inff();
    acc += live ? expf(s - l[k]) * d[k] : 0.f;
  }
  const float tot = sink_block_sum(acc, sh);
  if (threadIdx.x == 0) a.part[(int64_t)h * a.nparts + blockIdx.x] = tot;
}

// workgroup h: ds_h = -(the nparts partials of head h, thread t taking t, t + 256, ... in order)
__global__ __launch_bounds__(256) void sink_grad_sum_kernel(SinkGradArgs a) {
  __shared__ float sh[4];
  const int h = blockIdx.x;
  float acc = 0.f;
  for (int p = threadIdx.x; p < a.nparts; p += 256) acc += a.part[(int64_t)h * a.nparts + p];
  const float tot = sink_block_sum(acc, sh);
  if (threadIdx.x == 0) a.ds[h] = -tot;
}

}  // namespace xdot

extern "C" int xdot_sink_fold_launch(const xdot::SinkArgs* a, int dt, hipStream_t st) {
  using namespace xdot;
  if (a->B < 0 || a->R < 0 || a->H < 1 || a->D < 1 || a->s_dt < DT_F32 || a->s_dt > DT_F16) return -1;
  if (a->B == 0 || a->R == 0) return 0;
  if (dt == DT_BF16) return sink_fold_launch_dt<DT_BF16>(*a, st);
  if (dt == DT_F16) return sink_fold_launch_dt<DT_F16>(*a, st);
  if (dt == DT_F32) return sink_fold_launch_dt<DT_F32>(*a, st);
  return -1;
}

extern "C" int xdot_sink_grad_parts(int B, int R) {
  const int64_t n = (int64_t)B * R;
  const int64_t p = (n + xdot::kSinkChunk - 1) / xdot::kSinkChunk;
  return p < 1 ? 1 : (p >= (1LL << 31) ? -1 : (int)p);
}

extern "C" int xdot_sink_grad_launch(const xdot::SinkGradArgs* a, hipStream_t st) {
  using namespace xdot;
  // (an empty (B, R) has nothing to read: the caller returns zeros)
  if (a->B < 1 || a->R < 1 || a->H < 1 || a->H > 65535 || a->s_dt < DT_F32 || a->s_dt > DT_F16) return -1;
  if (a->nparts != xdot_sink_grad_parts(a->B, a->R)) return -1;
  hipLaunchKernelGGL(sink_grad_part_kernel, dim3((unsigned)a->nparts, (unsigned)a->H), dim3(256), 0, st, *a);
  hipLaunchKernelGGL(sink_grad_sum_kernel, dim3((unsigned)a->H), dim3(256), 0, st, *a);
  return 0;
}
