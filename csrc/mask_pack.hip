// xdot — compress the module's boolean attention mask (B, R, T) for the flash kernels.
//
// The reference materialises the expanded mask for every head and applies it with a full
// masked_fill pass over the (B, H, R, T) scores (reference: distributed_dot_product/
// module.py:47-50, :66).  Here the mask is read ONCE per forward (R*T bytes, shared by all
// heads and by the backward) and turned into
//   bits  (B, NKT, R) uint64 : bit k of word (kt, r) = mask[b, r, 64*kt + k] (kt-major: the
//         producer's stores and the row kernels' per-tile DMAs of 128/256 rows are contiguous)
//   bitsT (B, NRT, Tpad) uint64: the same bits column-major per 64-row tile (backward
//         column kernel: one word per lane covers its column's 64 rows)
//   flags (B, ceil(R/32), NKT4) uint8, NKT4 = NKT rounded up to 4: per 32-row x 64-col tile,
//         0 = nothing masked, 1 = everything masked (tile skipped), 2 = partial (bits applied
//         per element).  Rows are padded to 4 bytes so the kernels fetch a tile's flag with a
//         wave-uniform scalar load (s_load_dword), which does not wait on the vector-memory
//         counter that tracks their prefetched K/V tiles.
// An all-False mask (the reference example/benchmark) therefore costs the kernels nothing.
//
// mask_gen_kernel writes the same three tensors from a description of the mask (causal /
// sliding window / key lengths: xdot.StructuredMask) without any (B, R, T) input; both kernels
// share everything that follows a lane's two 64-bit words (mask_words_out).
#include "common.h"

namespace xdot {

// One wave per 64-row x 128-column block of one batch.  The wave reads the block with
// coalesced 8-byte lane pieces (8 lanes cover 64 contiguous bytes of a row; 8-byte loads when
// rows are 8-byte aligned, e.g. T = 25000, 4-byte or byte loads otherwise), packs every 8 bool bytes to one byte (4 bytes -> 4 bits with one
// 32-bit multiply), regroups the bytes per row through 1 KiB of LDS so lane i holds row i's
// two 64-bit words (a row-per-lane read of the mask was TA-bound: 64 cache lines per load
// instruction), stores them (bits), turns each set
// of 64 row words into 64 column words with a 6-step butterfly transpose across lanes (bits_t)
// and derives the 32-row flags with ballots.  Column tiles kt in [NKT, KT_ALL) only write padding.
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int m) {
  const uint32_t lo = __shfl_xor((uint32_t)v, m, 64), hi = __shfl_xor((uint32_t)(v >> 32), m, 64);
  return ((uint64_t)hi << 32) | lo;
}

// 4 bool bytes (each 0 or 1: torch's bool storage) -> 4 bits, byte k -> bit k
__device__ __forceinline__ uint32_t pack4(uint32_t x) { return (x * 0x10204080u) >> 28; }

// The part both producers share, entered once lane i holds row i's two 64-bit words of the
// block (rows past R: zero): the kt-major bits store, the 32-row flag ballots and the 6-step
// butterfly transpose into bits_t.
__device__ __forceinline__ void mask_words_out(const uint64_t (&wv)[2], uint64_t* __restrict__ bits,
                                               uint64_t* __restrict__ bt, uint8_t* __restrict__ flags, int lane, int b,
                                               int rt, int kt0, int R, int T, int NKT, int NKT4, int NRT, int Tpad) {
  const int r = rt * 64 + lane;
  const bool row_ok = r < R;
  if (row_ok && kt0 < NKT) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (kt0 + h < NKT) bits[((int64_t)b * NKT + kt0 + h) * R + r] = wv[h];  // kt-major: coalesced
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int kt = kt0 + h;
    uint64_t w = wv[h];
    // flags of the two 32-row halves (rows past R count as neither)
    if (kt < NKT4) {
      const int n = kt < NKT ? min(64, T - kt * 64) : 0;
      const uint64_t full = n == 64 ? ~0ull : ((1ull << n) - 1);
      const uint64_t any = __ballot(w != 0);
      const uint64_t all = __ballot(!row_ok || w == full);
      if ((lane & 31) == 0) {
        const int half = lane >> 5, rb = rt * 2 + half;
        if (rb < (R + 31) / 32) {
          const uint32_t a = (uint32_t)(any >> (32 * half)), l = (uint32_t)(all >> (32 * half));
          flags[((int64_t)b * ((R + 31) / 32) + rb) * NKT4 + kt] = kt >= NKT ? 1 : (a == 0 ? 0 : (l == 0xffffffffu ? 1 : 2));
        }
      }
    }
    // 64 x 64 bit transpose: lane c ends up with column c (bit i = row i)
    if (kt * 64 < Tpad) {
      const uint64_t M[6] = {0x00000000ffffffffull, 0x0000ffff0000ffffull, 0x00ff00ff00ff00ffull,
                             0x0f0f0f0f0f0f0f0full, 0x3333333333333333ull, 0x5555555555555555ull};
#pragma unroll
      for (int s = 0; s < 6; ++s) {
        const int j = 32 >> s;
        const uint64_t o = shfl_xor64(w, j);
        w = (lane & j) ? (((o >> j) & M[s]) | (w & ~M[s])) : ((w & M[s]) | ((o & M[s]) << j));
      }
      bt[((int64_t)b * NRT + rt) * Tpad + (int64_t)kt * 64 + lane] = w;
    }
  }
}

__global__ __launch_bounds__(256) void mask_pack_kernel(const uint8_t* __restrict__ m, uint64_t* __restrict__ bits,
                                                         uint64_t* __restrict__ bt, uint8_t* __restrict__ flags,
                                                         int B, int R, int T, int NKT, int NKT4, int NRT, int Tpad,
                                                         int KT_ALL, int va) {
  const int lane = threadIdx.x & 63;
  const int KT2 = (KT_ALL + 1) / 2;
  const int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blk >= (int64_t)B * NRT * KT2) return;  // whole waves exit together
  const int kt0 = (int)(blk % KT2) * 2;
  const int64_t brt = blk / KT2;
  const int rt = (int)(brt % NRT), b = (int)(brt / NRT);
  const int r = rt * 64 + lane;
  const bool row_ok = r < R;
  uint64_t wv[2] = {0, 0};
  __shared__ __attribute__((aligned(16))) uint8_t stage[4][64 * 16];  // per wave: 64 rows x 128 bits
  uint8_t* sw = stage[threadIdx.x >> 6];
  const int c0 = kt0 * 64;
  if (kt0 < NKT && c0 + 128 <= T) {
    // coalesced: instruction (i, j) reads rows 8i..8i+7, bytes 64j..64j+63 of the block
    // (8 lanes x 8 B contiguous per row); each lane packs its 8 bytes to one byte in LDS
    uint64_t x[16];
    const int lr = lane >> 3, lc = (lane & 7) * 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int rr = rt * 64 + 8 * i + lr;
      const uint8_t* p = m + ((int64_t)b * R + min(rr, R - 1)) * T + c0 + lc;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const uint8_t* q = p + 64 * j;
        uint64_t v;
        if (va == 8) {
          v = *reinterpret_cast<const uint64_t*>(q);
        } else if (va == 4) {  // rows 4-byte aligned (T % 8 == 4, e.g. T = 12500)
          v = (uint64_t)*reinterpret_cast<const uint32_t*>(q) | ((uint64_t)*reinterpret_cast<const uint32_t*>(q + 4) << 32);
        } else {               // odd row strides: byte loads, still 64 contiguous bytes per 8 lanes
          v = 0;
#pragma unroll
          for (int e = 0; e < 8; ++e) v |= (uint64_t)q[e] << (8 * e);
        }
        x[2 * i + j] = rr < R ? v : 0ull;
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const uint64_t v = x[2 * i + j];
        sw[(8 * i + lr) * 16 + 8 * j + (lane & 7)] = (uint8_t)(pack4((uint32_t)v) | (pack4((uint32_t)(v >> 32)) << 4));
      }
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): wave-private staging
    __builtin_amdgcn_wave_barrier();
    const u32x4 q = *reinterpret_cast<const u32x4*>(sw + lane * 16);
    wv[0] = ((uint64_t)q[1] << 32) | q[0];
    wv[1] = ((uint64_t)q[3] << 32) | q[2];
  } else if (row_ok && kt0 < NKT) {
    const uint8_t* p = m + ((int64_t)b * R + r) * T + c0;
    const int n = min(128, T - c0);
    for (int k = 0; k < n; ++k) wv[k >> 6] |= (uint64_t)(p[k] != 0) << (k & 63);
  }
  mask_words_out(wv, bits, bt, flags, lane, b, rt, kt0, R, T, NKT, NKT4, NRT, Tpad);
}

// The same three outputs from a DESCRIPTION of the mask (xdot.StructuredMask) instead of a
// (B, R, T) tensor: nothing R x T sized is read.  Row r of the block is global row
// gr = row_off + r; its unmasked global columns are one interval [lo, hi]:
//   causal      hi = gr                      window w    lo = gr - (w - 1), and without causal
//   lengths     hi = min(hi, lengths[b] - 1)             hi = gr + (w - 1)
// The packed columns are a concatenation of `nseg` runs (packed_start, length, global_start)
// of consecutive global columns (global_start < 0: a run that is masked whatever the row), so
// within a run the interval is again an interval of packed columns: every word starts as "all
// of its columns below T masked" and each overlapping run clears one shifted range of ones.
//
// Documents (DOCS; starts: n sorted int32 global positions per batch, row stride `dstride`, 0 for
// one shared table): the row's own document is the interval [s[k-1], s[k] - 1] with k the number
// of starts <= gr (s[-1] = 0, s[n] = infinity), cut into [lo, hi].  Every 128-column block of the
// same 64 rows repeats the search, and a binary search is a chain of log2 n dependent loads, so
// the wave searches together: k0, the count for its first row, by a 64-ary search (each lane
// loads one sample, a ballot counts them: one load per factor 64 of n), then ONE load of the 64
// starts that follow.  Unless all 64 are <= the wave's last row, they are every start that
// separates two of its rows, and each lane counts those <= its own row in registers.  Otherwise
// (64 or more documents begin inside the tile: one-row or empty documents) the last row's count k1
// is searched the same way and a lane bisects [k0, k1] in memory.  Whatever the table holds,
// every index read is in [0, n) and every search shrinks its range, so an unsorted (unvalidated
// device) table gives an unspecified mask, not a fault.  Without DOCS the code is what it was.
//
// Row runs (ROWS; rows: `nrow` runs (local_start, length, global_start) of consecutive global rows
// that tile [0, R), built and checked by the host): local row r is global row global_start +
// (r - local_start) of the run that holds it, in place of row_off + r (a rank whose rows are not
// one range: the zigzag layout's two chunks).  The interval arithmetic is per lane already.  The
// wave's document search is not: it takes the tile's 64 rows for the consecutive global rows
// [g0, g1].  A tile inside one run keeps it, with g0 / g1 from its run.  A tile that holds a run
// boundary (at most one per boundary) has rows from far-apart ranges: every lane bisects the whole
// table for its own row and the hull is left open.  Without ROWS the code is what it was.

constexpr int64_t kNoBound = (int64_t)1 << 60;  // (the run arithmetic below stays in range)

// first i in [a, e) with s[i] > x, else e: one lane's bisection
__device__ __forceinline__ int doc_upper(const int* __restrict__ s, int a, int e, int64_t x) {
  while (a < e) {
    const int m = a + ((e - a) >> 1);
    if ((int64_t)s[m] <= x) a = m + 1; else e = m;
  }
  return a;
}

// the same for wave-uniform a, e, x, by all 64 lanes of the wave together
__device__ __forceinline__ int doc_upper_wave(const int* __restrict__ s, int a, int e, int64_t x, int lane) {
  while (e - a > 64) {
    // 64 chunks of `step`; lane j samples the last element of chunk j: chunks wholly <= x are passed
    const int step = (e - a + 63) >> 6;
    const int64_t p = (int64_t)a + (int64_t)(lane + 1) * step - 1;
    const int c = __popcll(__ballot(p < e && (int64_t)s[p < e ? p : a] <= x));
    const int64_t a2 = (int64_t)a + (int64_t)c * step;
    e = (int)min(a2 + step - 1, (int64_t)e);  // that chunk's sample is > x (or past the end)
    a = (int)min(a2, (int64_t)e);
  }
  const int i = a + lane;
  return a + __popcll(__ballot(i < e && (int64_t)s[i < e ? i : 0] <= x));  // (n > 0: s[0] exists)
}

// global row of local row r (rows outside every run, past R: a position nobody uses)
template <bool ROWS>
__device__ __forceinline__ int64_t run_row(const int* __restrict__ rows, int nrow, int64_t row_off, int r) {
  if (!ROWS) return row_off + r;
  int64_t g = 0;
  for (int s = 0; s < nrow; ++s) {  // wave-uniform loads
    const int ls = rows[3 * s], len = rows[3 * s + 1];
    if (r >= ls && r - ls < len) g = (int64_t)rows[3 * s + 2] + (r - ls);
  }
  return g;
}

template <bool DOCS, bool ROWS>
__global__ __launch_bounds__(256) void mask_gen_kernel(uint64_t* __restrict__ bits, uint64_t* __restrict__ bt,
                                                        uint8_t* __restrict__ flags, const int* __restrict__ lengths,
                                                        const int* __restrict__ segs, int nseg, int causal,
                                                        int64_t window, int64_t row_off, int B, int R, int T, int NKT,
                                                        int NKT4, int NRT, int Tpad, int KT_ALL,
                                                        const int* __restrict__ starts, int n, int64_t dstride,
                                                        const int* __restrict__ rows, int nrow) {
  const int lane = threadIdx.x & 63;
  const int KT2 = (KT_ALL + 1) / 2;
  const int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blk >= (int64_t)B * NRT * KT2) return;  // whole waves exit together
  const int kt0 = (int)(blk % KT2) * 2;
  const int64_t brt = blk / KT2;
  const int rt = (int)(brt % NRT), b = (int)(brt / NRT);
  const int r = rt * 64 + lane;
  uint64_t wv[2] = {0, 0};
  const int64_t c0 = (int64_t)kt0 * 64;
  const int64_t grow = run_row<ROWS>(rows, nrow, row_off, r);  // this lane's global row
  // the lane's own document [dlo, dhi], and the hull of the wave's documents [wlo, whi]: global
  // columns outside the hull are masked in every row of the wave
  int64_t dlo = 0, dhi = kNoBound, wlo = 0, whi = kNoBound;
  if (DOCS && (int64_t)__builtin_amdgcn_readfirstlane(kt0) * 64 < T) {  // all 64 lanes enter (ballots, shuffles)
    const int rtu = __builtin_amdgcn_readfirstlane(rt), bu = __builtin_amdgcn_readfirstlane(b);
    const int* __restrict__ ds = starts + (int64_t)bu * dstride;
    int64_t g0 = row_off + (int64_t)rtu * 64, g1 = row_off + min(rtu * 64 + 63, R - 1);
    bool one_run = true;  // wave-uniform: the tile's rows are the consecutive global rows [g0, g1]
    if (ROWS) {
      const int r0 = rtu * 64, r1 = min(rtu * 64 + 63, R - 1);
      one_run = false;
      for (int s = 0; s < nrow; ++s) {
        const int ls = rows[3 * s], len = rows[3 * s + 1];
        if (r0 >= ls && r1 >= r0 && r1 - ls < len) {
          one_run = true;
          g0 = (int64_t)rows[3 * s + 2] + (r0 - ls);
          g1 = g0 + (r1 - r0);
        }
      }
    }
    // rows past R: bounds nobody uses
    const int64_t gr = ROWS ? (one_run ? g0 + lane : grow) : row_off + r;
    if (ROWS && !one_run) {  // a run boundary inside the tile: per-lane rows, no hull
      const int k = doc_upper(ds, 0, n, gr);
      dlo = k > 0 ? (int64_t)ds[k - 1] : 0;
      dhi = k < n ? (int64_t)ds[k] - 1 : kNoBound;
    } else {
      const int k0 = doc_upper_wave(ds, 0, n, g0, lane);
      if (k0 > 0) wlo = ds[k0 - 1];
      const int i = k0 + lane;
      const int v = ds[i < n ? i : 0];  // lane j: start k0 + j
      const int cnt = __popcll(__ballot(i < n && (int64_t)v <= g1));
      if (cnt < 64) {  // the starts in (g0, g1] are lanes 0 .. cnt - 1; k1 = k0 + cnt
        if (k0 + cnt < n) whi = (int64_t)__builtin_amdgcn_readlane(v, cnt) - 1;
        int k = 0;  // of them, those <= gr
        for (int j = 0; j < cnt; ++j) k += (int64_t)__builtin_amdgcn_readlane(v, j) <= gr;
        k = min(k, cnt);
        const int below = __shfl(v, max(k - 1, 0), 64), above = __shfl(v, min(k, 63), 64);
        dlo = k > 0 ? (int64_t)below : wlo;
        dhi = k < cnt ? (int64_t)above - 1 : whi;
      } else {
        const int k1 = doc_upper_wave(ds, k0 + 64, n, g1, lane);
        if (k1 < n) whi = (int64_t)ds[k1] - 1;
        const int k = doc_upper(ds, k0, k1, gr);
        dlo = k > 0 ? (int64_t)ds[k - 1] : 0;
        dhi = k < n ? (int64_t)ds[k] - 1 : kNoBound;
      }
    }
  }
  if (r < R && c0 < T) {
    const int64_t gr = grow;
    int64_t lo = 0, hi = kNoBound;
    if (causal) hi = gr;
    if (window > 0) {
      lo = gr - (window - 1);
      if (!causal) hi = gr + (window - 1);
    }
    if (lengths != nullptr) hi = min(hi, (int64_t)lengths[b] - 1);
    if (DOCS) {
      lo = max(lo, dlo);
      hi = min(hi, dhi);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t nc = min((int64_t)64, T - (c0 + 64 * h));
      wv[h] = nc >= 64 ? ~0ull : (nc > 0 ? (1ull << nc) - 1 : 0ull);
    }
    for (int s = 0; s < nseg; ++s) {  // wave-uniform
      const int64_t ps = segs[3 * s], len = segs[3 * s + 1], gs = segs[3 * s + 2];
      if (gs < 0 || ps + len <= c0 || ps >= c0 + 128) continue;
      // the run's part of this block, in global columns, against the hull of the wave's documents
      if (DOCS && (gs + (min(ps + len, c0 + 128) - 1 - ps) < wlo || gs + (max(ps, c0) - ps) > whi)) continue;
      // unmasked packed columns of this run: global [lo, hi] moved by (ps - gs), cut to the run
      const int64_t a = max(ps, lo - gs + ps), e = min(ps + len - 1, hi - gs + ps);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int64_t p0 = c0 + 64 * h;
        const int64_t a_ = max(a, p0), e_ = min(e, p0 + 63);
        if (a_ <= e_) {
          const int cnt = (int)(e_ - a_ + 1);  // 1..64
          wv[h] &= ~((cnt == 64 ? ~0ull : (1ull << cnt) - 1) << (int)(a_ - p0));
        }
      }
    }
  }
  mask_words_out(wv, bits, bt, flags, lane, b, rt, kt0, R, T, NKT, NKT4, NRT, Tpad);
}

}  // namespace xdot

extern "C" int xdot_mask_pack_launch(const uint8_t* mask, uint64_t* bits, uint64_t* bt, uint8_t* flags, int B, int R,
                                     int T, hipStream_t st) {
  using namespace xdot;
  const int NKT = (T + 63) / 64, NKT4 = (NKT + 3) & ~3, NRT = (R + 63) / 64, Tpad = (T + 127) / 128 * 128;
  const int KT_ALL = max(NKT4, Tpad / 64);
  // widest load every row start satisfies (the kernel reads each row's 128-column block as
  // 8-byte lane pieces; narrower alignment splits them, the access pattern stays coalesced)
  const uintptr_t base = reinterpret_cast<uintptr_t>(mask);
  const int va = (T % 8 == 0 && (base & 7) == 0) ? 8 : (T % 4 == 0 && (base & 3) == 0) ? 4 : 1;
  const int64_t nblk = (int64_t)B * NRT * ((KT_ALL + 1) / 2);
  if (nblk == 0) return 0;
  hipLaunchKernelGGL(mask_pack_kernel, dim3((unsigned)((nblk + 3) / 4)), dim3(256), 0, st, mask, bits, bt, flags, B, R, T,
                     NKT, NKT4, NRT, Tpad, KT_ALL, va);
  return 0;
}

// lengths: (B,) int32 or null; segs: (nseg, 3) int32 (packed_start, length, global_start) covering
// [0, T); window <= 0: none; starts: nstarts sorted int32 document starts per batch (batch b's at
// starts + b * starts_stride, stride 0: one shared table) or null; rows: (nrows, 3) int32 (local_start,
// length, global_start) tiling [0, R) in place of row_off, or null
extern "C" int xdot_mask_gen_launch(uint64_t* bits, uint64_t* bt, uint8_t* flags, const int* lengths, const int* segs,
                                    int nseg, int causal, int64_t window, int64_t row_off, int B, int R, int T,
                                    const int* starts, int nstarts, int64_t starts_stride, const int* rows, int nrows,
                                    hipStream_t st) {
  using namespace xdot;
  const int NKT = (T + 63) / 64, NKT4 = (NKT + 3) & ~3, NRT = (R + 63) / 64, Tpad = (T + 127) / 128 * 128;
  const int KT_ALL = max(NKT4, Tpad / 64);
  const int64_t nblk = (int64_t)B * NRT * ((KT_ALL + 1) / 2);
  if (nblk == 0) return 0;
  const bool docs = starts != nullptr && nstarts > 0;
  const bool runs = rows != nullptr && nrows > 0;
  auto kern = runs ? (docs ? mask_gen_kernel<true, true> : mask_gen_kernel<false, true>)
                   : (docs ? mask_gen_kernel<true, false> : mask_gen_kernel<false, false>);
  hipLaunchKernelGGL(kern, dim3((unsigned)((nblk + 3) / 4)), dim3(256), 0, st, bits, bt, flags, lengths, segs, nseg, causal,
                     window, row_off, B, R, T, NKT, NKT4, NRT, Tpad, KT_ALL, starts, nstarts, starts_stride, rows,
                     runs ? nrows : 0);
  return 0;
}
