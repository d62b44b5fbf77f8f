// Runs the strided-row-view rule (csrc/row_view.h) over the cases on stdin, one per line, and prints one
// line per case: tests/test_row_view.py compiles this with plain g++ and states what it expects.
//   B R C s0 s1 s2 avail esize base written   ->  "ok sb sr vec lo hi", or the error's name
//   pair i j                                  ->  "pair <disjoint> <same_view>" of the i-th and j-th case
#include "row_view.h"

#include <cinttypes>
#include <cstdio>
#include <vector>

int main() {
  static const char* const names[] = {"ok", "inner_stride", "negative_stride", "rows_overlap", "out_of_bounds"};
  std::vector<xdot::RowView> seen;
  char line[256];
  while (std::fgets(line, sizeof line, stdin)) {
    unsigned i = 0, j = 0;
    if (std::sscanf(line, "pair %u %u", &i, &j) == 2) {
      if (i >= seen.size() || j >= seen.size()) return 2;
      std::printf("pair %d %d\n", (int)xdot::disjoint(seen[i], seen[j]), (int)xdot::same_view(seen[i], seen[j]));
      continue;
    }
    int64_t B, R, C, st[3], avail, esize;
    uint64_t base;
    int written;
    if (std::sscanf(line, "%" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64
                          " %" SCNu64 " %d",
                    &B, &R, &C, &st[0], &st[1], &st[2], &avail, &esize, &base, &written) != 10)
      return 2;
    xdot::RowView v;
    const auto err = xdot::row_view(B, R, C, st, avail, esize, (uintptr_t)base, written != 0, &v);
    seen.push_back(v);
    if (err != xdot::RowViewErr::ok)
      std::printf("%s\n", names[(int)err]);
    else
      std::printf("ok %" PRId64 " %" PRId64 " %d %" PRIu64 " %" PRIu64 "\n", v.sb, v.sr, (int)v.vec, (uint64_t)v.lo, (uint64_t)v.hi);
  }
  return 0;
}
