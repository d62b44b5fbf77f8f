// xdot — decode attention for gfx950: a few new rows against one rank's q/v cache, forward only.
//
// The cache is a bag of (position, q, v) slots: `col_pos` (B, Tcap) holds each slot's global position, -1
// for an empty one, and the kernel evaluates visibility from it (no packed mask): slot c is visible to new
// row i (position p_i = pos0 + i) iff 0 <= col_pos[c] <= p_i and (window == 0 or col_pos[c] > p_i - window),
// which is StructuredMask(causal=True, window=w) for a cache filled in any order.
//
// Work split: one workgroup per (column span, batch, GATHERED head).  The G * Rn rows (g, i) of the G row
// heads that read this gathered head are packed into the M dimension of v_mfma_f32_16x16x32 tiles (NT row
// tiles of 16, NT <= 4), so every q / v byte of the span leaves HBM once for the whole group.  The kernel
// is bound by bandwidth: each of the 4 waves sweeps its own 32-column tiles of the span (tile t of the span
// belongs to wave t % 4) with its own running (m, l, o) and no workgroup barrier per tile; the waves merge
// once at the end through LDS and the workgroup writes one fp32 partial slot (opart / lpart, the layout of
// the forward's split partials), merged over the spans by flash_decode_combine below.
//
// Per tile and wave, with n = lane & 15, g = lane >> 4:
//   positions  the lane's 8 columns 16 sub + 4 g + j (sub < 2, j < 4), loaded one tile ahead; a tile none
//              of whose positions any row can see is skipped before its q / v loads are issued.
//   S^T        = q . rows^T per 16-column sub-tile: the A operand (column 16 sub + n, features 32 dk + 8 g
//              .. + 7) is a 16-byte global load straight into the operand layout, the B operand the row
//              fragments held in registers.  The lane ends with row n and the columns above: the softmax
//              statistics of a row live in the 4 lanes n, n + 16, n + 32, n + 48.
//   O^T        += V^T . P^T: k slot 8 g + e is column 4 g + e (e < 4) / 16 + 4 g + e - 4, so P^T is the
//              lane's own 8 probabilities (no cross-lane move) and V^T comes from the wave-private
//              [column][feature] LDS image of the v tile through two ds_read_b64_tr_b16 per 16 features.
//              The lane ends with row n and features 16 dn + 4 g .. + 3: the same row as its statistics.
#include "flash_decode.h"

namespace xdot {
namespace fa {

template <int DT, int D, int NT>
__global__ __launch_bounds__(256) void flash_decode_kernel(DecodeArgs a) {
  using Cfg = DecCfg<D, NT>;
  constexpr int DK = D / 32, DN = D / 16, CH = D / 8;
  constexpr float NINF = -__builtin_inff();
  __shared__ __attribute__((aligned(16))) char lds[Cfg::LDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, g = lane >> 4;
  const int sp = blockIdx.x % a.nspan, bh = blockIdx.x / a.nspan;
  const int hg = bh % a.Hg, b = bh / a.Hg;
  const int G = a.H / a.Hg, M = G * a.Rn, C = a.H * D;
  const float sc = a.scale * LOG2E;

  // the row fragments (B operand of S^T) and each packed row's visible position range (lo, hi]
  u32x4 rf[NT][DK];
  int lo[NT], hi[NT];
#pragma unroll
  for (int rt = 0; rt < NT; ++rt) {
    const int m = rt * 16 + n;
    const bool live = m < M;
    const int gh = live ? m / a.Rn : 0, i = live ? m - gh * a.Rn : 0;
    const char* p = reinterpret_cast<const char*>(a.rows) + (((int64_t)b * a.Rn + i) * C + (hg * G + gh) * D + 8 * g) * 2;
#pragma unroll
    for (int dk = 0; dk < DK; ++dk)
      rf[rt][dk] = live ? *reinterpret_cast<const u32x4*>(p + dk * 64) : u32x4{0u, 0u, 0u, 0u};
    hi[rt] = live ? a.pos0 + i : -1;  // a padding row sees nothing
    lo[rt] = a.window > 0 ? max(hi[rt] - a.window, -1) : -1;
  }
  // what any row of the launch can see
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
  const char* qb = reinterpret_cast<const char*>(a.qc) + ((int64_t)b * a.Tcap * a.ldkv + hg * D) * 2;
  const char* vb = reinterpret_cast<const char*>(a.vc) + ((int64_t)b * a.Tcap * a.ldkv + hg * D) * 2;
  const int64_t ldb = a.ldkv * 2;
  char* vl = lds + wave * Cfg::VTILE;
  typedef const __attribute__((address_space(3))) char lds_char;
  lds_char* vt = (lds_char*)vl + (4 * g + (n >> 2)) * Cfg::VROW + 8 * (n & 3);

  // positions of the lane's 8 columns of tile t (past the cache: empty)
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
      // q fragments from global memory (columns past the cache re-read the last one: invisible)
      u32x4 qf[2][DK];
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        const char* p = qb + (int64_t)min(c0 + 16 * sub + n, cmax) * ldb + 16 * g;
#pragma unroll
        for (int dk = 0; dk < DK; ++dk) qf[sub][dk] = *reinterpret_cast<const u32x4*>(p + dk * 64);
      }
      // the v tile: DN 16-byte chunks per lane, rows of CH chunks
      u32x4 vr[DN];
#pragma unroll
      for (int it = 0; it < DN; ++it) {
        const int x = it * 64 + lane, r = x / CH, ch = x - r * CH;
        vr[it] = *reinterpret_cast<const u32x4*>(vb + (int64_t)min(c0 + r, cmax) * ldb + ch * 16);
      }
      f32x4 s[NT][2];
#pragma unroll
      for (int rt = 0; rt < NT; ++rt) s[rt][0] = s[rt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int dk = 0; dk < DK; ++dk)
#pragma unroll
          for (int rt = 0; rt < NT; ++rt) s[rt][sub] = mfma16<DT>::run(qf[sub][dk], rf[rt][dk], s[rt][sub]);
      wave_sync();  // the previous tile's reads are done
#pragma unroll
      for (int it = 0; it < DN; ++it) {
        const int x = it * 64 + lane, r = x / CH, ch = x - r * CH;
        *reinterpret_cast<u32x4*>(vl + r * Cfg::VROW + ch * 16) = vr[it];
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
          x[e] = vis ? s[rt][e >> 2][e & 3] * sc : NINF;
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

  // ---- merge the 4 waves --------------------------------------------------------------------------
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
  // one partial slot: the output normalised over the span and its natural-log LSE (-inf: nothing visible)
  for (int idx = threadIdx.x; idx < M * (D / 4); idx += 256) {
    const int m = idx / (D / 4), c4 = idx - m * (D / 4);
    const int gh = m / a.Rn, i = m - gh * a.Rn, h = hg * G + gh;
    const float lt = tl[m], inv = lt > 0.f ? 1.f / lt : 0.f;
    const f32x4 v = *reinterpret_cast<const f32x4*>(oimg + m * Cfg::OROW + 4 * c4) * inv;
    *reinterpret_cast<f32x4*>(a.opart + (((int64_t)sp * a.B + b) * a.Rn + i) * C + h * D + 4 * c4) = lt > 0.f ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    if (c4 == 0) a.lpart[(((int64_t)sp * a.B + b) * a.H + h) * a.Rn + i] = lt > 0.f ? (tm[m] + __log2f(lt)) * LN2 : NINF;
  }
}

// Merge the spans' partial slots: one workgroup per (batch, new row, row head).  flash_fwd_combine gives a
// thread all slots of its 4 outputs, which serialises the hundred-odd spans of a long cache; here the 256
// threads are D / 4 columns x NG slot groups, each group sums every NG-th slot, and the groups are added
// in a fixed order.  lse = log sum_s e^{lse_s}, O = sum_s e^{lse_s - lse} O_s; a row no span saw comes out
// NaN with lse -inf like the forward kernels' fully masked rows.  out32: fp32 output (the wire format of
// the cross-rank merge) instead of the rows' dtype.
template <int DT, int D>
__global__ __launch_bounds__(256) void flash_decode_combine(DecodeArgs a) {
  using T16 = typename dt_traits<DT>::T;
  constexpr int C4 = D / 4, NG = 256 / C4;
  constexpr float NINF = -__builtin_inff();
  __shared__ float red[4];
  __shared__ f32x4 accs[NG][C4];
  __shared__ float sums[NG];
  const int tid = threadIdx.x;
  const int h = blockIdx.x % a.H, bi = blockIdx.x / a.H, i = bi % a.Rn, b = bi / a.Rn;
  const int C = a.H * D;
  const int64_t lstride = (int64_t)a.B * a.H * a.Rn, ostride = (int64_t)a.B * a.Rn * C;
  const float* lp = a.lpart + ((int64_t)b * a.H + h) * a.Rn + i;
  float mx = NINF;
  for (int s = tid; s < a.nspan; s += 256) mx = fmaxf(mx, lp[s * lstride]);
  mx = wave_max(mx);
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const int c4 = tid % C4, grp = tid / C4;
  if (grp < NG) {
    const float* op = a.opart + ((int64_t)b * a.Rn + i) * C + h * D + 4 * c4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float sum = 0.f;
    for (int s = grp; s < a.nspan; s += NG) {
      const float l = lp[s * lstride];
      if (l == NINF) continue;
      const float w = __expf(l - mx);
      sum += w;
      acc += w * *reinterpret_cast<const f32x4*>(op + s * ostride);
    }
    accs[grp][c4] = acc;
    if (c4 == 0) sums[grp] = sum;
  }
  __syncthreads();
  if (tid < C4) {
    f32x4 acc = accs[0][tid];
    float sum = sums[0];
#pragma unroll
    for (int q = 1; q < NG; ++q) {
      acc += accs[q][tid];
      sum += sums[q];
    }
    const f32x4 v = acc * (1.f / sum);  // sum == 0 (nothing visible anywhere): NaN output, -inf lse
    const int64_t at = ((int64_t)b * a.Rn + i) * C + h * D + 4 * tid;
    if (a.out32) {
      *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.out) + at) = v;
    } else {
      u32x2 w = {pack2<DT>(v[0], v[1]), pack2<DT>(v[2], v[3])};
      *reinterpret_cast<u32x2*>(reinterpret_cast<T16*>(a.out) + at) = w;
    }
    if (tid == 0) a.lse[((int64_t)b * a.H + h) * a.Rn + i] = mx + __logf(sum);
  }
}

template <int DT, int D, int NT>
static void launch_decode_nt(const DecodeArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((flash_decode_kernel<DT, D, NT>), dim3((unsigned)(a.nspan * a.B * a.Hg)), dim3(256), 0, st, a);
}

template <int DT, int D>
static int launch_decode(const DecodeArgs& a, hipStream_t st) {
  const int nt = decode_row_tiles(a.H / a.Hg, a.Rn);
  switch (nt) {
    case 1: launch_decode_nt<DT, D, 1>(a, st); break;
    case 2: launch_decode_nt<DT, D, 2>(a, st); break;
    case 3:  // three row tiles run as four (the fourth is padding: MFMAs the memory stream hides)
    case 4: launch_decode_nt<DT, D, 4>(a, st); break;
    default: return -1;
  }
  hipLaunchKernelGGL((flash_decode_combine<DT, D>), dim3((unsigned)(a.B * a.Rn * a.H)), dim3(256), 0, st, a);
  return 0;
}

}  // namespace fa
}  // namespace xdot

// the merge of a->opart / a->lpart over the spans alone (the fp8 sweep of flash_decode8.hip feeds it)
extern "C" int xdot_flash_decode_combine_launch(const xdot::fa::DecodeArgs* a, int dt, int D, hipStream_t st) {
  using namespace xdot;
  using namespace xdot::fa;
  return for_dtype16_head_dim(dt, D, -1, [&](auto t, auto d) {
    hipLaunchKernelGGL((flash_decode_combine<decltype(t)::value, decltype(d)::value>), dim3((unsigned)(a->B * a->Rn * a->H)),
                       dim3(256), 0, st, *a);
    return 0;
  });
}

// the span sweep into a->opart / a->lpart, then the merge into a->out / a->lse; -1: no kernel for this
// dtype / head dim / G * Rn
extern "C" int xdot_flash_decode_launch(const xdot::fa::DecodeArgs* a, int dt, int D, hipStream_t st) {
  using namespace xdot;
  using namespace xdot::fa;
  if (a->B == 0 || a->Rn == 0 || a->H == 0) return 0;
  return for_dtype16_head_dim(dt, D, -1, [&](auto t, auto d) { return launch_decode<decltype(t)::value, decltype(d)::value>(*a, st); });
}
