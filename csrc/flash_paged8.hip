// xdot — decode attention over a PAGED fp8 (OCP e4m3fn) q/v cache for gfx950, and the kernel that fills it:
// the ragged batch of csrc/flash_paged.hip over the bytes and per-slot scales of csrc/flash_decode8.hip.
//
// Format: the pool is P pages of S slots.  `qv` (P, S, 2*Hg*D) bytes, a slot [q heads | v heads]; `scales`
// (P, 2*Hg, S) fp32, slot innermost WITHIN A PAGE (rows 0..Hg-1 the q heads, Hg..2*Hg-1 the v heads): value =
// scale * e4m3(byte); pool_pos, table, npages and pos0 as in the 16-bit pool.  An empty slot holds zero bytes
// and scale 1.  The page is the outer dimension of `scales` so that the 32 scales of one tile of one head
// are 128 contiguous bytes: a tile never leaves its page (S is a multiple of 32).
//
// flash_paged8_kernel: flash_paged_kernel's work split and indirection (one workgroup per (span, sequence,
// gathered head), spans cut per sequence from npages[b], a wave-uniform table entry two tiles ahead and the
// positions one tile ahead, holes / entries outside [0, P) / inactive sequences / unseen tiles skipped before
// any byte or scale is loaded, an empty partial from a starved workgroup) around flash_decode8_kernel's
// operands (16-bit rows and v_mfma_f32_16x16x32_{bf16,f16}; q bytes in 16-byte loads feeding two MFMAs with
// an 8-byte tail where D / 32 is odd; v bytes widened on the way into the wave-private LDS image read by
// ds_read_b64_tr_b16; x = vis ? s * sc * sq : -inf, P^T packs p * sv, l sums the unscaled p).  Two things
// differ from the dense fp8 sweep:
//   full tiles  every tile is whole, so none of the min(c, cmax) clamps remain: addresses are cur + constant.
//   scales      a lane's eight columns 16 (e >> 2) + 4 g + (e & 3) are two runs of four consecutive slots, and
//               with the slot innermost their sq and sv are two 16-byte loads each where the dense layout
//               ((B, 2*Hg, cap), clamped columns) takes sixteen 4-byte ones.  They are issued with the tile's q
//               bytes and used after the S^T products: no scale register lives across tiles.
//
// cache_quant_paged_kernel: cache_quant_kernel's lane grouping and arithmetic (a group of D / 8 lanes per
// chunk, xor-shuffle amax, s = amax / 448, correctly rounded division, v_cvt_pk_fp8_f32) with a scatter: row
// i goes to the flat slot slots[i] = page * S + slot of the pool, its scale to scales[page, chunk, slot] and
// its position to pool_pos: a one-token step of the whole batch, or a ragged prefill, is one launch.  A slot
// index outside [0, P * S) is skipped.  Rows and bytes are touched once, there are no atomics; duplicate
// slots in one call are unspecified.
#include "flash_decode.h"

#include <type_traits>

namespace xdot {
namespace fa {

template <int DT, int D, int NT>
__global__ __launch_bounds__(256) void flash_paged8_kernel(PagedArgs pa) {
  using Cfg = DecCfg<D, NT>;
  // DK S^T products per sub-tile: DP pairs fed by one 16-byte q load each, and a tail where DK is odd
  constexpr int DK = D / 32, DP = DK / 2, DN = D / 16, CH = D / 16;
  constexpr bool TAIL = DK & 1;
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
  const int ssh = __builtin_ctz(pa.S), tsh = ssh - 5, tmask = (1 << tsh) - 1;  // log2 of the slots / tiles of a page
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
  const char* qb = reinterpret_cast<const char*>(a.qc) + hg * D;
  const char* vb = reinterpret_cast<const char*>(a.vc) + hg * D;
  // the lane's first scale of a tile at slot 0 of page 0: + page * sc_batch + slot in the page
  const float* qs = a.qscale + hg * a.sc_head + 4 * g;
  const float* vs = a.vscale + hg * a.sc_head + 4 * g;
  const int64_t ldb = a.ldkv;
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
      // the lane's 8 scales of q and of v: two runs of four consecutive slots of the tile's page
      const int64_t so = (int64_t)(cur >> ssh) * a.sc_batch + (cur & (pa.S - 1));
      const f32x4 sq0 = *reinterpret_cast<const f32x4*>(qs + so), sq1 = *reinterpret_cast<const f32x4*>(qs + so + 16);
      const f32x4 sv0 = *reinterpret_cast<const f32x4*>(vs + so), sv1 = *reinterpret_cast<const f32x4*>(vs + so + 16);
      // q bytes from global memory
      u32x4 qp[2][DP > 0 ? DP : 1];
      u32x2 qt[2];
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        const char* p = qb + (int64_t)(cur + 16 * sub + n) * ldb;
#pragma unroll
        for (int j = 0; j < DP; ++j) qp[sub][j] = *reinterpret_cast<const u32x4*>(p + 64 * j + 16 * g);
        if constexpr (TAIL) qt[sub] = *reinterpret_cast<const u32x2*>(p + 32 * (DK - 1) + 8 * g);
      }
      // the v tile: DK 16-byte chunks per lane, rows of CH chunks
      u32x4 vr[DK];
#pragma unroll
      for (int it = 0; it < DK; ++it) {
        const int x = it * 64 + lane, r = x / CH, ch = x - r * CH;
        vr[it] = *reinterpret_cast<const u32x4*>(vb + (int64_t)(cur + r) * ldb + ch * 16);
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
          x[e] = vis ? s[rt][e >> 2][e & 3] * sc * (e < 4 ? sq0[e & 3] : sq1[e & 3]) : NINF;
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
          x[e] *= e < 4 ? sv0[e & 3] : sv1[e & 3];
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
__global__ __launch_bounds__(256) void cache_quant_paged_kernel(QuantPagedArgs a) {
  using V8 = typename std::conditional<DT == DT_BF16, bf16x8, f16x8>::type;
  constexpr int L = D / 8, W = L <= 4 ? 4 : L <= 8 ? 8 : 16;  // lanes of a chunk, and of its slot in the wave
  const int64_t chunk = ((int64_t)blockIdx.x * 256 + threadIdx.x) / W;
  const int li = threadIdx.x % W;
  const bool row = chunk < (int64_t)a.N * a.chunks;
  const int c = (int)(chunk % a.chunks);
  const int64_t i = chunk / a.chunks;
  const int slot = row ? a.slots[i] : -1;
  const bool live = (unsigned)slot < (unsigned)a.nslots && li < L;  // a slot outside the pool is skipped
  float x[8];
  float amax = 0.f;
  if (live) {
    const char* p = reinterpret_cast<const char*>(a.rows) + (i * a.sr + c * D + 8 * li) * 2;
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
    *reinterpret_cast<u32x2*>(reinterpret_cast<char*>(a.qv8) + ((int64_t)slot * a.chunks + c) * D + 8 * li) = u32x2{(uint32_t)w0, (uint32_t)w1};
    if (li == 0) {
      const int pg = slot / a.S, sl = slot - pg * a.S;
      a.scales[((int64_t)pg * a.chunks + c) * a.S + sl] = s;
      if (c == 0) a.pool_pos[slot] = a.positions[i];
    }
  }
}

template <int DT, int D>
static int launch_paged8(const PagedArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)(a.d.nspan * a.d.B * a.d.Hg));
  switch (decode_row_tiles(a.d.H / a.d.Hg, a.d.Rn)) {
    case 1: hipLaunchKernelGGL((flash_paged8_kernel<DT, D, 1>), grid, dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL((flash_paged8_kernel<DT, D, 2>), grid, dim3(256), 0, st, a); break;
    case 3:  // three row tiles run as four, as in the dense sweep
    case 4: hipLaunchKernelGGL((flash_paged8_kernel<DT, D, 4>), grid, dim3(256), 0, st, a); break;
    default: return -1;
  }
  return xdot_flash_decode_combine_launch(&a.d, DT, D, st);
}

}  // namespace fa
}  // namespace xdot

// the paged fp8 span sweep into a->d.opart / lpart, then the merge into a->d.out / lse; -1: no kernel for this
// dtype / head dim / G * Rn / page size, or no scales
extern "C" int xdot_flash_paged8_launch(const xdot::fa::PagedArgs* a, int dt, int D, hipStream_t st) {
  using namespace xdot;
  using namespace xdot::fa;
  if (a->d.B == 0 || a->d.Rn == 0 || a->d.H == 0) return 0;
  if (!paged_page_size_ok(a->S) || a->P <= 0 || a->maxp <= 0 || a->d.nspan <= 0 || !a->d.qscale || !a->d.vscale) return -1;
  return for_dtype16_head_dim(dt, D, -1, [&](auto t, auto d) { return launch_paged8<decltype(t)::value, decltype(d)::value>(*a, st); });
}

extern "C" int xdot_cache_quant_paged_launch(const xdot::fa::QuantPagedArgs* a, int dt, int D, hipStream_t st) {
  using namespace xdot;
  using namespace xdot::fa;
  constexpr int none = -1;
  if (!paged_page_size_ok(a->S) || a->nslots <= 0 || a->nslots % a->S != 0) return none;
  return for_dtype16_head_dim(dt, D, none, [&](auto t, auto d) {
    constexpr int Dc = decltype(d)::value, L = Dc / 8, W = L <= 4 ? 4 : L <= 8 ? 8 : 16;
    const int64_t threads = (int64_t)a->N * a->chunks * W;
    if (threads == 0) return 0;
    if ((threads + 255) / 256 >= (1LL << 31)) return none;
    hipLaunchKernelGGL((cache_quant_paged_kernel<decltype(t)::value, Dc>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, *a);
    return 0;
  });
}
