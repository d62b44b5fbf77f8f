"""Attention masks given as a description (causal / sliding window / key lengths) instead of a
dense ``(B, R, T)`` boolean tensor.

The flash kernels consume a packed mask (:class:`xdot.ops.flash.PackedMask`);
``csrc/mask_pack.hip`` generates it straight from a :class:`StructuredMask`
(:func:`xdot.ops.flash.generate_mask`), so nothing ``R x T`` sized is ever built.  Paths that
only take a dense mask (the torch reference paths, CPU tensors, ``impl="materialized"``) get
:meth:`StructuredMask.dense` once at their entry: those DO allocate the ``(B, R, T)`` tensor.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple, Union

import torch

Segment = Tuple[int, int, int]  # (packed_start, length, global_start); global_start -1: always masked


class StructuredMask:
    """``StructuredMask(causal=False, window=None, lengths=None, row_offset=None, doc_starts=None)``

    True = masked, as everywhere in this package.  With ``gr = row_offset + r`` the global index
    of local row ``r`` and ``gc`` the global column in ``[0, T)``, an element is masked iff

    * ``causal`` and ``gc > gr``, or
    * ``window = w`` (int >= 1) and ``gc < gr - (w - 1)`` -- without ``causal`` also
      ``gc > gr + (w - 1)`` --, or
    * ``lengths`` is given and ``gc >= lengths[b]``, or
    * ``doc_starts`` is given and ``doc(gc) != doc(gr)``, with ``doc(x)`` the number of entries
      ``<= x``: several documents packed back to back into one sequence do not attend across
      their boundaries.

    ``doc_starts``: the global positions at which a new document begins, in non-decreasing order:
    ``(n,)`` shared by the batch or ``(B, n)``, an integer tensor or a (nested) sequence of ints
    (:meth:`from_doc_lengths` takes the documents' lengths instead).  Position 0 begins a
    document whether listed or not; a repeated entry is an empty document (so rows of different
    document counts are padded by repeating the last start, or with ``T``); entries ``>= T`` have
    no effect; ``n = 0`` is one document.  A tensor is kept by reference like ``lengths``.  The
    order and sign of a host sequence or CPU tensor are checked at construction; the CONTENT OF A
    DEVICE TENSOR IS NOT VALIDATED (that would need a host synchronisation): the kernel stays in
    bounds and terminates whatever it holds, but the mask of an unsorted table is unspecified.
    Entries are read as int32, clamped to ``[0, 2^31 - 1]``.

    ``lengths``: a ``(B,)`` integer tensor (kept by reference: a device tensor is read by the
    kernel with no host synchronisation, and an in-place edit re-generates the cached packed
    mask) or a sequence of ints.  ``row_offset=None``: this rank's rows, resolved by the attention
    entry points from the communicator and their ``layout`` (``rank * R`` onward for the contiguous
    one, the rank's two chunks for ``"zigzag"``: :mod:`xdot.parallel.layout`).  An explicit
    ``row_offset`` says the rows are consecutive, so it contradicts ``layout="zigzag"``.

    The object is immutable and is not a tensor; pass it where a mask tensor goes
    (``attn_mask`` of :class:`xdot.DistributedDotProductAttn`, ``mask`` of
    :func:`xdot.seq_parallel_attention` / the ring ops)."""

    __slots__ = ("causal", "window", "lengths", "row_offset", "doc_starts", "_T", "_rows", "_cols", "_bound",
                 "__weakref__")

    def __init__(self, causal: bool = False, window: Optional[int] = None,
                 lengths: Union[None, torch.Tensor, Sequence[int]] = None, row_offset: Optional[int] = None,
                 doc_starts: Union[None, torch.Tensor, Sequence[int], Sequence[Sequence[int]]] = None):
        if window is not None:
            if isinstance(window, bool) or not isinstance(window, int):
                raise TypeError(f"StructuredMask: window must be an int or None, got {type(window).__name__}")
            if window < 1:
                raise ValueError(f"StructuredMask: window must be >= 1, got {window}")
        if lengths is not None:
            if not isinstance(lengths, torch.Tensor):
                lengths = torch.tensor([int(x) for x in lengths], dtype=torch.int64)
            if lengths.dim() != 1 or lengths.is_floating_point() or lengths.is_complex() or lengths.dtype == torch.bool:
                raise ValueError("StructuredMask: lengths must be a (B,) integer tensor or a sequence of ints")
        if row_offset is not None:
            row_offset = int(row_offset)
            if row_offset < 0:
                raise ValueError(f"StructuredMask: row_offset must be >= 0, got {row_offset}")
        if doc_starts is not None:
            doc_starts = _check_doc_starts(doc_starts)
        s = object.__setattr__
        s(self, "causal", bool(causal))
        s(self, "window", window)
        s(self, "lengths", lengths)
        s(self, "row_offset", row_offset)
        s(self, "doc_starts", doc_starts)
        s(self, "_T", None)      # global column count, set on the copies bind() hands out
        s(self, "_rows", None)   # there too: the row runs when the rows are not one run from row_offset
        s(self, "_cols", None)   # and the global index of every gathered column when not the identity
        s(self, "_bound", {})

    def __setattr__(self, name, value):
        raise AttributeError("StructuredMask is immutable")

    def __repr__(self):
        ln = None if self.lengths is None else f"<{self.lengths.numel()} lengths on {self.lengths.device}>"
        ds = "" if self.doc_starts is None else (f", doc_starts=<{tuple(self.doc_starts.shape)} starts on "
                                                 f"{self.doc_starts.device}>")
        return (f"StructuredMask(causal={self.causal}, window={self.window}, lengths={ln}, "
                f"row_offset={self.row_offset}{ds})")

    @classmethod
    def from_doc_lengths(cls, doc_lengths, **kw) -> "StructuredMask":
        """The mask of documents of the given lengths packed back to back from position 0:
        ``doc_lengths`` is ``(n,)`` or ``(B, n)`` (tensor or sequence), ``doc_starts`` its exclusive
        cumulative sum along the last axis, computed with torch ops on the device the lengths
        live on (no host synchronisation).  Other arguments pass through."""
        if "doc_starts" in kw:
            raise TypeError("StructuredMask.from_doc_lengths: doc_starts is computed from doc_lengths")
        dl = _check_doc_starts(doc_lengths, what="doc_lengths", order=False)
        return cls(doc_starts=torch.cumsum(dl, dim=-1) - dl, **kw)

    @property
    def _version(self):
        """What :class:`xdot.ops.flash.MaskCache` compares (``==``) besides the object's identity:
        it changes with an in-place write to ``lengths`` or to ``doc_starts``."""
        v = 0 if self.lengths is None else self.lengths._version
        return v if self.doc_starts is None else (v, self.doc_starts._version)

    def check(self, B: int) -> None:
        if self.lengths is not None and self.lengths.numel() != B:
            raise ValueError(f"StructuredMask: lengths has {self.lengths.numel()} entries, the batch is {B}")
        if self.doc_starts is not None and self.doc_starts.dim() == 2 and self.doc_starts.size(0) != B:
            raise ValueError(f"StructuredMask: doc_starts has {self.doc_starts.size(0)} rows, the batch is {B}")

    def bind(self, rows, T: int, cols=None) -> "StructuredMask":
        """The description with its rows resolved and the global column count ``T`` noted: the
        object the cached packed masks are keyed on.  ``rows``: this rank's first row (used only
        where the object has no ``row_offset``) or its row runs ``[(local_start, length,
        global_start)]``; one run is the same as its ``global_start``.  ``cols``: ``(key, index)``,
        the global index of every gathered column (int ``(T,)``) and a hashable name for it, when
        the gathered side is not in global order (None).  The same arguments give the same object
        back."""
        runs = None
        if isinstance(rows, (list, tuple)):
            runs = tuple((int(a), int(b), int(c)) for a, b, c in rows)
            if len(runs) == 1 and runs[0][0] == 0:
                rows, runs = runs[0][2], None
            elif self.row_offset is not None:
                raise ValueError(f"StructuredMask: row_offset={self.row_offset} says the rows are consecutive, "
                                 f"the layout gives the runs {list(runs)}")
        ro = None if runs is not None else (int(rows) if self.row_offset is None else self.row_offset)
        key = (ro if runs is None else runs, int(T)) + (() if cols is None else (cols[0],))
        b = self._bound.get(key)
        if b is None:
            if len(self._bound) >= 8:
                self._bound.pop(next(iter(self._bound)))
            b = StructuredMask(self.causal, self.window, self.lengths, ro, self.doc_starts)
            object.__setattr__(b, "_T", int(T))
            object.__setattr__(b, "_rows", runs)
            if cols is not None:
                object.__setattr__(b, "_cols", cols[1].reshape(-1).to("cpu", torch.int32))
            self._bound[key] = b
        return b

    def device_lengths(self, device) -> Optional[torch.Tensor]:
        """``lengths`` as the kernel reads them: contiguous int32 on ``device`` (no host sync for a
        device tensor)."""
        if self.lengths is None:
            return None
        ln = self.lengths.to(device=device, non_blocking=True)
        return ln.clamp(min=0, max=2**31 - 1).to(torch.int32).contiguous()

    def device_doc_starts(self, device) -> Optional[torch.Tensor]:
        """``doc_starts`` as the kernel reads them: contiguous int32 ``(n,)`` or ``(B, n)`` on
        ``device``, clamped to ``[0, 2^31 - 1]`` (no host sync for a device tensor); None when
        there are none (``n = 0`` included)."""
        if self.doc_starts is None or self.doc_starts.numel() == 0:
            return None
        ds = self.doc_starts.to(device=device, non_blocking=True)
        return ds.clamp(min=0, max=2**31 - 1).to(torch.int32).contiguous()

    def dense(self, B: int, R: int, T: int, row_offset: Optional[int] = None, device=None) -> torch.Tensor:
        """The equivalent ``(B, R, T)`` boolean tensor, built with plain torch ops (it allocates
        ``B * R * T`` bytes).  ``row_offset`` is used where the object has none."""
        ro = self.row_offset if self.row_offset is not None else row_offset
        if ro is None:
            self.check(B)
            raise ValueError("StructuredMask.dense: row_offset is not set")
        return self.dense_at(B, int(ro) + torch.arange(R, device=device, dtype=torch.int64),
                             torch.arange(T, device=device, dtype=torch.int64), device)

    def dense_at(self, B: int, row_index, col_index, device=None) -> torch.Tensor:
        """The dense oracle at arbitrary positions: the ``(B, R, T)`` boolean tensor whose element
        ``(b, r, t)`` is the mask of global row ``row_index[r]`` against global column
        ``col_index[t]`` (integer tensors or sequences; a negative column is masked in every
        row).  ``row_offset`` plays no part.  Plain torch ops; allocates ``B * R * T`` bytes."""
        self.check(B)
        gr = torch.as_tensor(row_index).to(device=device, dtype=torch.int64).reshape(-1)
        gc = torch.as_tensor(col_index).to(device=device, dtype=torch.int64).reshape(-1)
        R, T = gr.numel(), gc.numel()
        gr, gc = gr.view(R, 1), gc.view(1, T)
        m = torch.zeros(R, T, dtype=torch.bool, device=device)
        if self.causal:
            m |= gc > gr
        if self.window is not None:
            m |= gc < gr - (self.window - 1)
            if not self.causal:
                m |= gc > gr + (self.window - 1)
        m |= gc < 0
        m = m.unsqueeze(0).expand(B, R, T)
        if self.lengths is not None:
            m = m | (gc.view(1, 1, T) >= self.lengths.to(device=device, dtype=torch.int64).view(B, 1, 1))
        if self.doc_starts is not None and self.doc_starts.numel() > 0:
            ds = self.doc_starts.to(device=device, dtype=torch.int64).contiguous()
            lead = ds.shape[:-1]  # () shared, (B,) per batch
            doc_r = torch.searchsorted(ds, gr.view(R).expand(*lead, R).contiguous(), right=True)
            doc_c = torch.searchsorted(ds, gc.view(T).expand(*lead, T).contiguous(), right=True)
            m = m | (doc_r.unsqueeze(-1) != doc_c.unsqueeze(-2))
        return m.contiguous()


class GatheredColumns:
    """A dense ``(B, R, T)`` mask tensor whose columns are in GLOBAL order while the gathered side
    is not (``layout="zigzag"``): what the kernel paths carry in place of the tensor.
    :func:`xdot.ops.flash.prepare_mask_cached` selects ``cols`` (the global index of every gathered
    column) before the launch's own column view, and caches the packed result on the tensor."""

    __slots__ = ("tensor", "cols", "key")

    def __init__(self, tensor: torch.Tensor, cols: torch.Tensor, key):
        self.tensor, self.cols, self.key = tensor, cols, key

    def select(self, m: torch.Tensor) -> torch.Tensor:
        return m.index_select(-1, self.cols.to(m.device))


def _check_doc_starts(x, what: str = "doc_starts", order: bool = True) -> torch.Tensor:
    """``doc_starts`` (or the lengths they come from) as an integer tensor of rank 1 or 2; what a
    host sequence or CPU tensor holds is checked (sign, ``order``: non-decreasing), what a device
    tensor holds is not (no host synchronisation)."""
    if not isinstance(x, torch.Tensor):
        try:
            x = torch.as_tensor(x)
        except (TypeError, ValueError, RuntimeError) as e:
            raise ValueError(f"StructuredMask: {what} must be an integer tensor or a (nested) sequence of ints: {e}")
        if x.numel() == 0:  # an empty list comes out as float32
            x = x.to(torch.int64)
    if x.is_floating_point() or x.is_complex() or x.dtype == torch.bool:
        raise ValueError(f"StructuredMask: {what} must hold integers, got {x.dtype}")
    if x.dim() not in (1, 2):
        raise ValueError(f"StructuredMask: {what} must be (n,) or (B, n), got shape {tuple(x.shape)}")
    if x.device.type == "cpu" and x.numel() > 0:
        if bool((x < 0).any()):
            raise ValueError(f"StructuredMask: {what} has a negative entry")
        if order and x.size(-1) > 1 and bool((x[..., 1:] < x[..., :-1]).any()):
            raise ValueError(f"StructuredMask: {what} must be in non-decreasing order")
    return x


def resolve(mask, B: int, R: int, T: int, rank: int, packed: bool, device, layout: str = "contiguous"):
    """What an attention entry point does with its mask argument.  A :class:`StructuredMask` is
    checked against the batch and bound to this rank's rows and to the gathered side's column
    order under ``layout`` (``packed``: a path that generates the packed mask from it), or turned
    into its dense tensor once (every other path), columns in rank-major gathered order.  A dense
    tensor has local rows and GLOBAL columns: under a layout whose gathered side is not in global
    order its columns are selected into that order, here (not ``packed``) or per kernel launch
    (:class:`GatheredColumns`).  None passes through."""
    from ..parallel import layout as L  # (xdot.parallel imports this module)

    L.check_layout(layout)
    spec = isinstance(mask, StructuredMask)
    if layout != "contiguous" and spec and mask.row_offset is not None:
        raise ValueError(f"StructuredMask: row_offset={mask.row_offset} says this rank's rows are consecutive, "
                         f"which contradicts layout={layout!r}")
    n = T // R if R else 1
    if n <= 1:
        layout = "contiguous"  # a world of one: the identity
    if not spec:
        if mask is None or layout == "contiguous":
            return mask
        cols = L.gathered_cols(layout, n, R)
        return GatheredColumns(mask, cols, (layout, n, R)) if packed else mask.index_select(-1, cols.to(mask.device))
    mask.check(B)
    if layout == "contiguous":
        return mask.bind(rank * R, T) if packed else mask.dense(B, R, T, rank * R, device)
    if packed:
        return mask.bind(L.row_runs(layout, rank, n, R), T, ((layout, n, R), L.gathered_cols(layout, n, R)))
    return mask.dense_at(B, L.global_rows(layout, rank, n, R), L.gathered_cols(layout, n, R), device)


def run_lengths(idx: torch.Tensor) -> List[Segment]:
    """Run-length encoding of a row of global column indices (-1: always masked) into the
    generator's segment table: maximal runs of consecutive indices, or of -1."""
    v = idx.reshape(-1).to("cpu", torch.int64)
    n = v.numel()
    if n == 0:
        return []
    cont = ((v[1:] - v[:-1] == 1) & (v[:-1] >= 0)) | ((v[1:] < 0) & (v[:-1] < 0))
    starts = torch.cat([torch.zeros(1, dtype=torch.int64), torch.nonzero(~cont).reshape(-1) + 1])
    ends = torch.cat([starts[1:], torch.tensor([n], dtype=torch.int64)])
    g = v[starts]
    return [(int(s), int(e - s), int(x) if x >= 0 else -1) for s, e, x in zip(starts.tolist(), ends.tolist(), g.tolist())]


def segments_of(view, T: int, cols: Optional[torch.Tensor] = None) -> List[Segment]:
    """The segment table of ``view`` (a function of a ``(B, R, T)`` mask giving the columns a
    kernel launch sees, or None for all of them in order): the same function applied to a
    ``(1, 1, T)`` row of column indices, run-length encoded.  ``cols``: the global index of every
    column the view starts from (the gathered side's order under a layout; None: the identity),
    so every view composes with the layout unchanged."""
    idx = (torch.arange(T, dtype=torch.int32) if cols is None else cols.to("cpu", torch.int32).reshape(-1)).view(1, 1, T)
    return run_lengths(idx if view is None else view(idx))


def expand_segments(segs: Sequence[Segment]) -> torch.Tensor:
    """Inverse of :func:`run_lengths`: the int64 index row of a segment table."""
    parts = [torch.full((ln,), -1, dtype=torch.int64) if g < 0 else torch.arange(g, g + ln, dtype=torch.int64)
             for _p, ln, g in segs]
    return torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int64)
