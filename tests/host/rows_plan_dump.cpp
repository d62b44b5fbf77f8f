// `rows_plan_dump rounds B R H nsplit wgs_per_cu` prints rows_rounds(...), `rows_plan_dump wpc B R H
// nsplit req occ3` prints rows_wpc(...) of csrc/flash_plan.h (tests/test_flash_rows_plan.py).
#include "flash_plan.h"

#include <cstdio>

using namespace xdot::fa;

int main(int argc, char** argv) {
  if (argc != 7 && argc != 8) return 2;
  const int64_t B = std::atoll(argv[2]), R = std::atoll(argv[3]), H = std::atoll(argv[4]), ns = std::atoll(argv[5]);
  if (!std::strcmp(argv[1], "rounds") && argc == 7)
    std::printf("%lld\n", (long long)rows_rounds(B, R, H, ns, std::atoi(argv[6])));
  else if (!std::strcmp(argv[1], "wpc") && argc == 8)
    std::printf("%d\n", rows_wpc(B, R, H, ns, std::atoi(argv[6]), std::atoi(argv[7])));
  else
    return 2;
  return 0;
}
