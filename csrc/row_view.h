// xdot — the one rule for a strided row operand of the row-wise ops (rope, headnorm, sink, gate): a
// (B, R, C) view with unit inner stride and any non-negative row / batch strides, inside its storage
// (the q half of a packed [q | v] buffer, a rank slot of the gather buffer, a padded batch).
// Host-only integer arithmetic over standard headers (plain g++ compiles it: tests/test_row_view.py);
// bindings_common.h wraps it for tensors and turns the error codes into messages.
#pragma once
#include <cstdint>

namespace xdot {

// batch / row strides in elements (0 for a dimension of size 1), whether the base and both strides are
// on the 16-byte grid, and the bytes [lo, hi) the view spans
struct RowView { int64_t sb, sr; bool vec; uintptr_t lo, hi; };

enum class RowViewErr { ok, inner_stride, negative_stride, rows_overlap, out_of_bounds };

// `stride`: the view's three strides in elements; `avail_elems`: elements from `base` to the end of the
// storage; `written`: every (b, row) is written, so two of them may not share memory.  An empty view
// passes with no stride checks (nothing is launched on it).  An extent past int64 is out of bounds
inline RowViewErr row_view(int64_t B, int64_t R, int64_t C, const int64_t stride[3], int64_t avail_elems, int64_t esize,
                           uintptr_t base, bool written, RowView* v) {
  *v = RowView{0, 0, true, base, base};
  if (B == 0 || R == 0 || C == 0) return RowViewErr::ok;
  if (C != 1 && stride[2] != 1) return RowViewErr::inner_stride;
  const int64_t sb = B > 1 ? stride[0] : 0, sr = R > 1 ? stride[1] : 0;
  if (sb < 0 || sr < 0) return RowViewErr::negative_stride;
  int64_t rows = 0, batches = 0, n = 0;  // elements one batch spans; offset of the last batch; all of it
  const bool fits = !__builtin_mul_overflow(R - 1, sr, &rows) && !__builtin_add_overflow(rows, C, &rows) &&
                    !__builtin_mul_overflow(B - 1, sb, &batches) && !__builtin_add_overflow(batches, rows, &n);
  if (written && fits && !((R == 1 || sr >= C) && (B == 1 || sb >= rows))) return RowViewErr::rows_overlap;
  if (!fits || n > avail_elems) return RowViewErr::out_of_bounds;
  const int64_t V = 16 / esize;
  *v = RowView{sb, sr, (base & 15) == 0 && sb % V == 0 && sr % V == 0, base, base + (uintptr_t)n * (uintptr_t)esize};
  return RowViewErr::ok;
}

inline bool disjoint(const RowView& a, const RowView& b) { return a.hi <= b.lo || b.hi <= a.lo; }

// the same base and the same strides: an output in place over its input
inline bool same_view(const RowView& a, const RowView& b) { return a.lo == b.lo && a.sb == b.sb && a.sr == b.sr; }

}  // namespace xdot
