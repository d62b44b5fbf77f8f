// xdot — grid planning of the flash kernels: how many column / row splits a launch takes and whether
// it runs on the head-heavy grid.  Host-only arithmetic over standard headers (plain g++ compiles it:
// tests/test_flash_plan.py); the occupancy figures the models are fed with come from the kernels' files.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace xdot {
namespace fa {

// An integer environment knob, read per call (tests and A/B runs switch it inside one process):
// unset / empty / "auto" -> -1 (the model decides), else atoi clamped to [lo, hi].
inline int env_int(const char* name, int lo, int hi = INT32_MAX) {
  const char* e = std::getenv(name);
  if (!e || !*e || !std::strcmp(e, "auto")) return -1;
  return std::max(lo, std::min(hi, std::atoi(e)));
}

// XDOT_F32_HEAVY: 0 = uniform splits for the exact-fp32 forward and fused column pass (default 1:
// the head-heavy grid where the round model prefers it)
inline bool f32_heavy() {
  const char* e = std::getenv("XDOT_F32_HEAVY");
  return !(e && e[0] == '0');
}

// Column split of the row-block grid.  Every workgroup of a flash kernel does the same
// work, so the launch runs in ceil(workgroups / slots) equal rounds (slots = 2 per CU x 256
// CUs) and a last round that is barely occupied costs a whole round: T = 25000, H = 8 gives
// 1568 row blocks = 3.06 rounds -> 24 % idle.  Pick the split s (<= 8, >= 8 column tiles per
// split) minimising rounds(s) x (tiles / s + fixed per-workgroup cost ~ 8 tiles: prologue,
// epilogue, the combine pass); ties keep fewer splits.
inline int pick_split(int64_t blocks, int64_t T, int64_t slots, int64_t req) {
  const int64_t nkt = (T + 63) / 64;
  if (req > 0) return (int)std::max<int64_t>(1, std::min<int64_t>(req, nkt));
  int best = 1;
  double best_cost = 1e300;
  for (int s = 1; s <= 8; ++s) {
    if (s > 1 && nkt / s < 8) break;
    const int64_t rounds = (blocks * s + slots - 1) / slots;
    const double cost = (double)rounds * ((double)nkt / s + 8.0);
    if (cost < best_cost * 0.985) { best_cost = cost; best = s; }
  }
  return best;
}

// Column splits of the row-side backward kernel.  It runs concurrently with the gathered-side
// kernel (which has stream priority and owns the GPU while it runs): splitting the row kernel's
// column sweep until its workgroups are no longer than the column kernel's (36 vs 48 MFMAs per
// 64-tile step; R/64 tiles per column workgroup) lets it pack into that kernel's tail instead of
// running a long tail of its own.  Measured at the N = 8 rank shape (R = 3125, T = 25000, one
// MI355X, cols||rows): 2 splits 0.989, 3: 0.943, 4: 0.911, 6: 0.888 ms (profiles/r3_masked.md).
inline int rows_split(int64_t B, int64_t R, int64_t T, int64_t H) {
  const int64_t nkt = (T + 63) / 64, nrt = (R + 63) / 64;
  const int base = pick_split(((R + 127) / 128) * B * H, T, 512, 0);
  int64_t conc = (nkt * 36 + nrt * 48 - 1) / (nrt * 48);
  conc = std::min<int64_t>(8, std::max<int64_t>(1, std::min<int64_t>(conc, nkt / 8)));
  return std::max(base, (int)conc);
}

// Rounds of a row-side backward launch: its row blocks x column splits over the resident slots of
// the instantiation that runs it (workgroups per CU x CUs: 512 for the two-per-CU kernel, 768 for
// the three-per-CU one).  rows_split above stays the split of both: the split fixes the order of
// the partial sums, and a launch gives the same bits whichever instantiation runs it.
inline int64_t rows_rounds(int64_t B, int64_t R, int64_t H, int64_t nsplit, int wgs_per_cu, int cus = 256) {
  const int64_t wgs = ((R + 127) / 128) * B * H * std::max<int64_t>(1, nsplit);
  const int64_t slots = std::max<int64_t>(1, (int64_t)wgs_per_cu * cus);
  return (wgs + slots - 1) / slots;
}

// Workgroups per CU of a pre-scaled 16-bit row-side launch with D <= 96: 2 (the software-pipelined
// kernel) or 3 (the plain-body kernel, csrc/flash_bwd.hip).  req: XDOT_ROWS_WPC (-1 = auto, 2, 3);
// occ3: what the three-per-CU instantiation reports as resident (fewer than 3: there is no such
// launch).  auto: profiles/rows_3wg.md.
constexpr bool ROWS_WPC3_AUTO = true;
inline int rows_wpc(int64_t B, int64_t R, int64_t H, int64_t nsplit, int req, int occ3, int cus = 256) {
  if (occ3 < 3 || req == 2) return 2;
  if (req == 3) return 3;
  // a round of three per CU holds 1.5x the workgroups: it has to need fewer rounds to be considered
  if (rows_rounds(B, R, H, nsplit, 3, cus) >= rows_rounds(B, R, H, nsplit, 2, cus)) return 2;
  return ROWS_WPC3_AUTO ? 3 : 2;
}

// Row splits of a column-side launch: W workgroups of `nrt` 32-row tiles each, `slots` of them
// resident at once.  Fewest splits minimising ceil(W s / slots) / s (the idle share of the last
// round), each split >= 16 tiles, at most `maxs` splits, `per` charged per extra split (partials +
// their sum).  The kernels go through the csplit_* models below.
inline int pick_csplit(int64_t W, int nrt, int slots, int maxs, double per) {
  int best = 1;
  double bc = 1e300;
  for (int s = 1; s <= maxs && (s == 1 || nrt / s >= 16); ++s) {
    const double c = (double)((W * s + slots - 1) / slots) / s * (1.0 + per * (s - 1));
    if (c < bc * 0.98) {
      bc = c;
      best = s;
    }
  }
  return best;
}

// The split models of the occupancy-planned kernels: W unsplit workgroups, n tiles (32 wide) of the
// split dimension, `slots` = resident workgroups of the kernel over the whole GPU.
// Column side (fp32 and wide row splits of the dQ / dV / recompute passes): up to 4 splits at 2 %
// each (fp32 partials of the whole gathered-side gradient per split).
inline int csplit_cols(int64_t W, int n, int slots) { return pick_csplit(W, n, slots, 4, 0.02); }
// The exact-fp32 forward's workgroups are long (a 32-column fp32 tile is ~16x a 16-bit one), so a
// split costs little beside a part-full last round: up to 32 splits at 0.1 % each (the N=8 rank's 200
// row blocks: 19 splits fill five rounds of 768 slots instead of 7 splits in two part-full ones).
inline int csplit_f32_fwd(int64_t W, int n, int slots) { return pick_csplit(W, n, slots, 32, 0.001); }
// fp32 row side and split-bf16 forward: up to 8 splits at 0.4 % each (their partials are ~1 % of an
// fp32 kernel's time).  The fused exact-fp32 column pass is priced the same: a split costs it two
// fp32 partial copies of the gathered-side gradient (~0.06 ms at T = 25000), its last-round tail
// ~1.4 ms at 4 splits.
inline int csplit_f32_rows(int64_t W, int n, int slots) { return pick_csplit(W, n, slots, 8, 0.004); }
// Wide (D > 128) forward and row side: partials of a wide 16-bit kernel cost ~1 % per split.
inline int csplit_wide_rows(int64_t W, int n, int slots) { return pick_csplit(W, n, slots, 8, 0.01); }

// Head-heavy grid (the 16-bit and exact-fp32 forward over column tiles, the fused exact-fp32
// column pass over row tiles; whole-GPU launches).  A uniform split makes every block pay the
// partial writes and a combine pass, and still ends on a part-full round: at N=1 (1568 row
// blocks, 512 slots) the 16-bit forward's auto split is 3 -> 10 rounds of 1/3 blocks plus a 3-slot
// combine.  Instead each XCD (S slots, blockIdx % 8) runs its blocks whole and splits only its
// last `rem` blocks into enough pieces to fill one more round; only those tail blocks go through
// partials and the (compact) combine.  Chosen when the round model says it beats the uniform
// split; -> (whole, rem, split) per XCD, or false.
// W: unsplit workgroups; ntiles: 64-wide tiles of the split dimension; S: resident workgroups per
// XCD (64: 32 CUs x 2 for the 16-bit forward; occupancy x CUs / 8 for the fp32 kernels); su: the
// uniform split to beat (>= 1)
inline bool head_heavy_plan(int64_t W, int64_t ntiles, int64_t S, int su, int* whole, int* rem, int* split) {
  if (W % 8 || S <= 0 || su <= 0) return false;
  const int64_t m = W / 8, full = m / S, r = m % S;
  if (r == 0 || full == 0) return false;
  const double cu = (double)((W * su + 8 * S - 1) / (8 * S)) * ((double)ntiles / su + 8.0);
  double best = 1e300;
  int bs = 0;
  for (int s = 1; s <= 16; ++s) {
    if (s > 1 && ntiles / s < 8) break;
    const double c = (double)full * ((double)ntiles + 8.0) + (double)((r * s + S - 1) / S) * ((double)ntiles / s + 8.0);
    if (c < best * 0.985) { best = c; bs = s; }
  }
  if (bs < 2 || best >= cu * 0.97) return false;
  *whole = (int)(full * S); *rem = (int)r; *split = bs;
  return true;
}

}  // namespace fa
}  // namespace xdot
