// xdot — decode attention over a PAGED q/v cache for gfx950: a ragged batch of sequences, each a few new
// rows against its own pages of one shared pool, forward only.
//
// Layout: the pool is P pages of S slots ((P, S, ldkv) rows, `q` and `v` the two halves of a slot as in the
// dense cache), `pool_pos` (P, S) the global position of each slot (-1: empty), `table` (B, maxp) the page
// of each logical block of each sequence (-1: a hole), `npages` (B,) the table entries in use and `pos0`
// (B,) the position of each sequence's first new row (negative: the sequence is inactive, its rows see
// nothing).  table, npages and pos0 are read HERE, on the device: the host never waits for them, and the
// same launch serves the next step of a generation loop once they are updated in place.  Visibility is the
// dense kernel's rule per sequence: slot visible to row i of sequence b iff 0 <= pos <= pos0[b] + i and
// (window == 0 or pos > pos0[b] + i - window).
//
// S is a multiple of DEC_TILE (32, 64, 128, 256), so every 32-column tile lies in one page and is full:
// none of the dense sweep's clamps against the end of the cache remain.
//
// Work split: flash_decode_kernel's (csrc/flash_decode.hip): one workgroup per (column span, sequence,
// gathered head), the G * Rn rows of the group in NT 16-row v_mfma_f32_16x16x32 tiles, tile t of a span
// swept by wave t % 4 with its own (m, l, o), one merge of the waves at the end (decode_merge_waves), the
// spans merged by flash_decode_combine.  The grid is planned on the host from the table's width alone
// (plan_decode_paged), the spans are cut per sequence HERE: sequence b has nt_b = npages[b] * (S / 32)
// tiles and uses spans of max(8, ceil(nt_b / nspan)) tiles, so its work is spread evenly over as many of
// the nspan workgroups as it can feed at 8 tiles each; the others write an empty partial slot (lse -inf,
// which the combine skips) and leave.
//
// Data movement: the page of a tile is the same for the whole wave, so with the wave index made uniform
// the table entry is a scalar load.  The sweep keeps a three-deep chain in flight per wave, so that the
// indirection is never waited for: the table entry of the wave's tile after next, the positions of its next
// tile, q / v of the current one.  A tile whose entry is a hole or lies outside [0, P) (the table is device
// content nobody validated: such an entry gives an unspecified result, never an access outside the pool),
// or none of whose positions any row can see, is skipped before its q / v loads are issued.  q goes from
// global memory straight into the S^T operand layout, v through the wave-private LDS image and
// ds_read_b64_tr_b16, under the DecCfg LDS plan: see csrc/flash_decode.hip for the lane maps.
#include "flash_decode.h"

namespace xdot {
namespace fa {

template <int DT, int D, int NT>
__global__ __launch_bounds__(256) void flash_paged_kernel(PagedArgs pa) {
  using Cfg = DecCfg<D, NT>;
  constexpr int DK = D / 32, DN = D / 16, CH = D / 8;
  constexpr float NINF = -__builtin_inff();
  __shared__ __attribute__((aligned(16))) char lds[Cfg::LDS];
  const DecodeArgs& a = pa.d;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = lane & 15, g = lane >> 4;
  const int sp = blockIdx.x % a.nspan, bh = blockIdx.x / a.nspan;
  const int hg = bh % a.Hg, b = bh / a.Hg;
  const int G = a.H / a.Hg, M = G * a.Rn, C = a.H * D;
  const float sc = a.scale * LOG2E;

  // this sequence's span: tiles [t0, t1) of its npages * (S / 32)
  const int tsh = __builtin_ctz(pa.S) - 5, tmask = (1 << tsh) - 1;  // log2 of the tiles of a page
  const int p0 = pa.pos0v[b];
  const int ntl = min(max(pa.npages[b], 0), pa.maxp) << tsh;
  const int len = max(8, (ntl + a.nspan - 1) / a.nspan);
  const int t0 = sp * len, t1 = min(t0 + len, ntl);
  if (p0 < 0 || t0 >= ntl) {  // nothing to sweep (the whole workgroup agrees): an empty partial slot
    for (int idx = threadIdx.x; idx < M * (D / 4); idx += 256) {
      const int m = idx / (D / 4), c4 = idx - m * (D / 4);
      const int gh = m / a.Rn, i = m - gh * a.Rn, h = hg * G + gh;
      *reinterpret_cast<f32x4*>(a.opart + (((int64_t)sp * a.B + b) * a.Rn + i) * C + h * D + 4 * c4) = f32x4{0.f, 0.f, 0.f, 0.f};
      if (c4 == 0) a.lpart[(((int64_t)sp * a.B + b) * a.H + h) * a.Rn + i] = NINF;
    }
    return;
  }

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
    hi[rt] = live ? p0 + i : -1;  // a padding row sees nothing
    lo[rt] = a.window > 0 ? max(hi[rt] - a.window, -1) : -1;
  }
  // what any row of this sequence can see
  const int whi = p0 + a.Rn - 1, wlo = a.window > 0 ? max(p0 - a.window, -1) : -1;

  float mrun[NT], lrun[NT];
  f32x4 o[NT][DN];
#pragma unroll
  for (int rt = 0; rt < NT; ++rt) {
    mrun[rt] = NINF;
    lrun[rt] = 0.f;
#pragma unroll
    for (int dn = 0; dn < DN; ++dn) o[rt][dn] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const int32_t* tb = pa.table + (int64_t)b * pa.maxp;
  const char* qb = reinterpret_cast<const char*>(a.qc) + hg * D * 2;
  const char* vb = reinterpret_cast<const char*>(a.vc) + hg * D * 2;
  const int64_t ldb = a.ldkv * 2;
  char* vl = lds + wave * Cfg::VTILE;
  typedef const __attribute__((address_space(3))) char lds_char;
  lds_char* vt = (lds_char*)vl + (4 * g + (n >> 2)) * Cfg::VROW + 8 * (n & 3);

  // the pool slot of tile t's first column (wave-uniform: a scalar load of the table entry); -1: past the
  // span, a hole, or an entry outside the pool
  auto tile_slot = [&](int t) -> int {
    if (t >= t1) return -1;
    const int pg = tb[t >> tsh];
    return (unsigned)pg < (unsigned)pa.P ? pg * pa.S + ((t & tmask) << 5) : -1;
  };
  // positions of the lane's 8 columns of the tile at slot s0 (no tile: empty)
  auto load_pos = [&](int s0, int (&pos)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) pos[e] = s0 >= 0 ? a.col_pos[s0 + 16 * (e >> 2) + 4 * g + (e & 3)] : -1;
  };
  int cur = tile_slot(t0 + wave), nx1 = tile_slot(t0 + wave + 4);
  int pos[8], nxt[8];
  load_pos(cur, pos);
  for (int t = t0 + wave; t < t1; t += 4) {
    const int nx2 = tile_slot(t + 8);
    load_pos(nx1, nxt);
    bool seen = false;
#pragma unroll
    for (int e = 0; e < 8; ++e) seen |= pos[e] > wlo && pos[e] <= whi;
    if (__builtin_amdgcn_ballot_w64(seen) != 0) {  // cur >= 0 here: a tile without a page has no position
      // q fragments from global memory
      u32x4 qf[2][DK];
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        const char* p = qb + (int64_t)(cur + 16 * sub + n) * ldb + 16 * g;
#pragma unroll
        for (int dk = 0; dk < DK; ++dk) qf[sub][dk] = *reinterpret_cast<const u32x4*>(p + dk * 64);
      }
      // the v tile: DN 16-byte chunks per lane, rows of CH chunks
      u32x4 vr[DN];
#pragma unroll
      for (int it = 0; it < DN; ++it) {
        const int x = it * 64 + lane, r = x / CH, ch = x - r * CH;
        vr[it] = *reinterpret_cast<const u32x4*>(vb + (int64_t)(cur + r) * ldb + ch * 16);
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
    cur = nx1;
    nx1 = nx2;
  }
  decode_merge_waves<D, NT>(a, lds, mrun, lrun, o, sp, b, hg);
}

template <int DT, int D>
static int launch_paged(const PagedArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)(a.d.nspan * a.d.B * a.d.Hg));
  switch (decode_row_tiles(a.d.H / a.d.Hg, a.d.Rn)) {
    case 1: hipLaunchKernelGGL((flash_paged_kernel<DT, D, 1>), grid, dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL((flash_paged_kernel<DT, D, 2>), grid, dim3(256), 0, st, a); break;
    case 3:  // three row tiles run as four, as in the dense sweep
    case 4: hipLaunchKernelGGL((flash_paged_kernel<DT, D, 4>), grid, dim3(256), 0, st, a); break;
    default: return -1;
  }
  return xdot_flash_decode_combine_launch(&a.d, DT, D, st);
}

}  // namespace fa
}  // namespace xdot

// the paged span sweep into a->d.opart / lpart, then the merge into a->d.out / lse; -1: no kernel for this
// dtype / head dim / G * Rn / page size
extern "C" int xdot_flash_paged_launch(const xdot::fa::PagedArgs* a, int dt, int D, hipStream_t st) {
  using namespace xdot;
  using namespace xdot::fa;
  if (a->d.B == 0 || a->d.Rn == 0 || a->d.H == 0) return 0;
  if (!paged_page_size_ok(a->S) || a->P <= 0 || a->maxp <= 0 || a->d.nspan <= 0) return -1;
  return for_dtype16_head_dim(dt, D, -1, [&](auto t, auto d) { return launch_paged<decltype(t)::value, decltype(d)::value>(*a, st); });
}
