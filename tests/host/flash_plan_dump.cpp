// Dumps the flash kernels' grid planner (csrc/flash_plan.h) over a fixed case table, one line per
// case: tests/test_flash_plan.py compiles this with plain g++ and compares the output with
// tests/golden/flash_plan.txt, which was recorded from the functions as they stood before they
// moved into the header.  `flash_plan_dump env NAME lo hi` prints env_int(NAME, lo, hi) instead.
#include "flash_plan.h"

#include <cstdio>

using namespace xdot::fa;

static void heavy_line(const char* tag, int64_t W, int64_t ntiles, int64_t S, int su) {
  int whole = 0, rem = 0, split = 0;
  if (head_heavy_plan(W, ntiles, S, su, &whole, &rem, &split))
    std::printf("%s %lld %lld %lld %d -> %d %d %d\n", tag, (long long)W, (long long)ntiles, (long long)S, su, whole, rem, split);
  else
    std::printf("%s %lld %lld %lld %d -> no\n", tag, (long long)W, (long long)ntiles, (long long)S, su);
}

int main(int argc, char** argv) {
  if (argc == 5 && !std::strcmp(argv[1], "env")) {
    std::printf("%d\n", env_int(argv[2], std::atoi(argv[3]), std::atoi(argv[4])));
    return 0;
  }
  const int64_t blocks[] = {8, 200, 392, 520, 776, 1568, 12504};
  const int64_t Ts[] = {64, 512, 1024, 3125, 25000, 200000};
  const int64_t slots[] = {256, 512, 768};
  const int64_t reqs[] = {0, 1, 3, 8, 100};
  const int64_t Ss[] = {32, 64, 96};
  const int sus[] = {0, 1, 2, 4};
  for (int64_t b : blocks)
    for (int64_t T : Ts)
      for (int64_t sl : slots)
        for (int64_t req : reqs)
          std::printf("pick_split %lld %lld %lld %lld -> %d\n", (long long)b, (long long)T, (long long)sl, (long long)req,
                      pick_split(b, T, sl, req));
  // the forward's form: tiles of 64 columns; su 0 = the 16-bit forward's own uniform split
  for (int64_t b : blocks)
    for (int64_t T : Ts)
      for (int64_t S : Ss)
        for (int su : sus) heavy_line("heavy_fwd", b, (T + 63) / 64, S, su > 0 ? su : pick_split(b, T, 8 * S, 0));
  // the fused column pass's form: tiles of 64 rows, the uniform split never below 1
  for (int64_t b : blocks)
    for (int64_t n : {(int64_t)8, (int64_t)32, (int64_t)391})
      for (int64_t S : Ss)
        for (int sq : sus) heavy_line("heavy_cols", b, n, S, std::max(sq, 1));
  for (int64_t B : {(int64_t)1, (int64_t)2})
    for (int64_t R : {(int64_t)64, (int64_t)3125, (int64_t)25000})
      for (int64_t T : Ts)
        for (int64_t H : {(int64_t)1, (int64_t)8})
          std::printf("rows_split %lld %lld %lld %lld -> %d\n", (long long)B, (long long)R, (long long)T, (long long)H,
                      rows_split(B, R, T, H));
  const struct { int maxs; double per; } models[] = {{4, 0.02}, {8, 0.004}, {32, 0.001}, {8, 0.01}};
  for (int64_t b : blocks)
    for (int64_t T : Ts)
      for (int64_t sl : slots)
        for (const auto& m : models)
          std::printf("pick_csplit %lld %d %lld %d %g -> %d\n", (long long)b, (int)((T + 31) / 32), (long long)sl, m.maxs,
                      m.per, pick_csplit(b, (int)((T + 31) / 32), (int)sl, m.maxs, m.per));
  // the spot values tests/test_flash_plan.py asserts literally
  std::printf("pick_csplit 200 782 768 32 0.001 -> %d\n", pick_csplit(200, 782, 768, 32, 0.001));
  std::printf("pick_csplit 776 32 768 32 0.001 -> %d\n", pick_csplit(776, 32, 768, 32, 0.001));
  // the named models the kernel files call (each pick_csplit with its own cap and price per split)
  const struct { const char* name; int (*fn)(int64_t, int, int); } named[] = {
      {"csplit_cols", csplit_cols}, {"csplit_f32_fwd", csplit_f32_fwd}, {"csplit_f32_rows", csplit_f32_rows},
      {"csplit_wide_rows", csplit_wide_rows}};
  for (const auto& m : named)
    for (int64_t b : blocks)
      for (int64_t T : Ts)
        for (int64_t sl : slots)
          std::printf("%s %lld %d %lld -> %d\n", m.name, (long long)b, (int)((T + 31) / 32), (long long)sl,
                      m.fn(b, (int)((T + 31) / 32), (int)sl));
  return 0;
}
