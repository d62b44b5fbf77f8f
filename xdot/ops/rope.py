"""Rotary position embedding (RoPE) of the projected ``k`` / ``q``.

The rotation is a pass of its own between the projections and the attention
(``csrc/rope.hip``): the flash kernels, :class:`xdot.parallel.attention.SeqParallelAttention`
and the ring know nothing about positions.  Under sequence parallelism rank ``r`` holds rows
``[rR, (r+1)R)`` and rotates them at their GLOBAL positions before the all-gather: the same
``rank * R`` convention as ``StructuredMask(row_offset=None)``.  Under ``layout="zigzag"``
(:mod:`xdot.parallel.layout`) a rank's rows are two runs of global positions; the table is then
built per run and concatenated, the apply kernel reads a per-row table either way.

Convention: half-split pairs.  In a head of width ``D`` element ``i`` pairs with ``i + D/2``
(``i < D/2``), the angle at position ``p`` is ``θ(p, i) = p · base^(−2i/D)`` and

    out[i]       = x[i]·cos θ − x[i + D/2]·sin θ
    out[i + D/2] = x[i + D/2]·cos θ + x[i]·sin θ

All batches and heads share the positions.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from .. import _ext
from ._rowview import rotate_half, split_heads, unit_inner

__all__ = ["Rotary", "rope", "rope_apply"]

_HIP_DTYPES = (torch.bfloat16, torch.float16, torch.float32)
_MAX_POS = 2**31 - 1


class Rotary:
    """``Rotary(base=10000.0, offset=None)``: a description, like :class:`xdot.StructuredMask`.

    ``offset`` is the global position of this rank's first row; ``None`` resolves to this rank's
    rows under the entry point's ``layout`` at the call (``rank * R`` onward for the contiguous one,
    the rank's two chunks for ``"zigzag"``, which an explicit ``offset`` therefore contradicts; 0
    with ``distributed=False``).  Pass it as ``rope=`` to
    :class:`xdot.DistributedDotProductAttn` / :func:`xdot.seq_parallel_attention`, or to
    :func:`xdot.rope`.  The ``(cos, sin)`` tables are cached on the object."""

    __slots__ = ("base", "offset", "_tables", "__weakref__")

    def __init__(self, base: float = 10000.0, offset: Optional[int] = None):
        base = float(base)
        if not base > 0.0:
            raise ValueError(f"Rotary: base must be positive, got {base}")
        if offset is not None:
            offset = int(offset)
            if offset < 0:
                raise ValueError(f"Rotary: offset must be >= 0, got {offset}")
        self.base = base
        self.offset = offset
        self._tables = {}

    def __repr__(self):
        return f"Rotary(base={self.base:g}, offset={self.offset})"

    def resolve(self, rank: int, R: int, world_size: Optional[int] = None, layout: str = "contiguous"):
        """This rank's global positions: ``offset``, or where it is None ``rank * R`` -- under a
        ``layout`` whose rank holds several runs of rows (``"zigzag"`` with ``world_size > 1``) the
        tuple of its row runs ``(local_start, length, global_start)``, which :meth:`table`
        and :func:`rope` take in place of an offset."""
        if layout != "contiguous":
            from ..parallel import layout as L  # (xdot.parallel imports this module)

            L.check_layout(layout)
            if self.offset is not None:
                raise ValueError(f"Rotary: offset={self.offset} says this rank's rows are consecutive, which "
                                 f"contradicts layout={layout!r}")
            if world_size is not None and int(world_size) > 1:
                runs = L.row_runs(layout, rank, world_size, R)
                return runs[0][2] if len(runs) == 1 else tuple(runs)
        return int(rank) * int(R) if self.offset is None else self.offset

    def inv_freq(self, D: int) -> list:
        """``base ** (-2 i / D)`` for ``i < D/2`` as Python floats: the doubles both the CPU and
        the GPU table multiply the positions with."""
        return [self.base ** (-2.0 * i / D) for i in range(D // 2)]

    def table(self, R: int, D: int, offset, device, dtype: torch.dtype = torch.float32) -> Tuple[Tensor, Tensor]:
        """``(cos, sin)``, each ``(R, D/2)``, of the angles ``(offset + row) * inv_freq[i]``:
        product and sin / cos in fp64, rounded once to ``dtype`` (fp32 for the kernels; fp64
        tensors rotate with the unrounded table).  Cached on the object, keyed on
        ``(device, R, D, offset)`` and the dtype.  GPU: ``rope_table`` (``csrc/rope.hip``);
        CPU, or ``backend='torch'``: torch fp64.

        ``offset`` may be row runs ``[(local_start, length, global_start)]`` tiling the ``R`` rows
        in local order (:func:`xdot.parallel.layout.row_runs`): the table is built per run, the
        same way, and concatenated; one run is its ``global_start``."""
        R, D = int(R), int(D)
        runs = None
        if isinstance(offset, (list, tuple)):
            runs = tuple((int(a), int(b), int(c)) for a, b, c in offset if int(b) > 0)
            at = 0
            for a, b, _c in runs:
                if a != at:
                    break
                at = a + b
            if at != R:
                raise ValueError(f"Rotary: the row runs must tile the {R} rows in order, got {list(offset)}")
            if len(runs) <= 1:
                offset, runs = (runs[0][2] if runs else 0), None
        if runs is None:
            offset = int(offset)
        if D < 2 or D % 2:
            raise ValueError(f"Rotary: the head dim must be even, got {D}")
        for off, ln in ([(offset, R)] if runs is None else [(c, b) for _a, b, c in runs]):
            if off < 0 or off + ln > _MAX_POS:
                raise ValueError(f"Rotary: positions must stay below 2^31 (offset {off} + {ln} rows)")
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        key = (device, R, D, offset if runs is None else runs, dtype)
        tab = self._tables.get(key)
        if tab is None:
            if len(self._tables) >= 8:
                self._tables.pop(next(iter(self._tables)))
            inv = torch.tensor(self.inv_freq(D), dtype=torch.float64).to(device)

            def build(ln, off):
                if dtype == torch.float32 and _ext.use_hip(inv):
                    return tuple(_ext.ops().rope_table(ln, D, off, inv))
                ang = torch.arange(off, off + ln, dtype=torch.float64, device=device).view(ln, 1) * inv.view(1, -1)
                return torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)

            if runs is None:
                tab = build(R, offset)
            else:
                parts = [build(b, c) for _a, b, c in runs]
                tab = (torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]))
            self._tables[key] = tab
        return tab


def _table_dtype(x: Tensor) -> torch.dtype:
    return torch.float64 if x.dtype == torch.float64 else torch.float32


def rope_apply(x: Tensor, num_heads: int, cos: Tensor, sin: Tensor, inverse: bool = False, alpha: float = 1.0,
               out: Optional[Tensor] = None) -> Tensor:
    """``out = alpha * rotate(x)`` with a table of :meth:`Rotary.table`; no autograd.  ``x`` is
    ``(B, R, H*D)``; ``out`` may be ``x`` (in place), another tensor, or None (a new contiguous
    one).  GPU bf16 / fp16 / fp32 tensors with unit last stride run ``csrc/rope.hip`` on the view
    as it is (any row / batch strides); everything else is the torch reference math."""
    B, R, C, H, D = split_heads(x, num_heads, "rope", even=True)
    if cos.shape != (R, D // 2) or sin.shape != (R, D // 2):
        raise ValueError(f"rope: table {tuple(cos.shape)} does not fit (R, D/2) = ({R}, {D // 2})")
    if _ext.use_hip(x) and x.dtype in _HIP_DTYPES:
        x = unit_inner(x, in_place=out is x, what="rope")
        if out is None:
            out = torch.empty((B, R, C), dtype=x.dtype, device=x.device)
        _ext.ops().rope_apply(x, cos, sin, H, bool(inverse), float(alpha), out)
        return out
    o = rotate_half(x.reshape(B, R, H, D).to(_table_dtype(x)), cos, sin, inverse)
    if alpha != 1.0:
        o = o * alpha
    o = o.reshape(B, R, C).to(x.dtype)
    if out is None:
        return o
    out.copy_(o)
    return out


def rope(x: Tensor, num_heads: int, rotary: Rotary, *, offset=None, inverse: bool = False,
         alpha: float = 1.0, out: Optional[Tensor] = None) -> Tensor:
    """``alpha * rotate(x)`` for ``x`` ``(B, R, H*D)`` whose row ``r`` sits at position
    ``offset + r`` (``offset=None``: ``rotary.offset``, else 0; row runs ``[(local_start, length,
    global_start)]`` place each run of rows at its own positions).  Autograd-aware: the backward is
    the inverse rotation of the incoming gradient times ``alpha``.  ``x`` may be a strided view
    with unit last stride (the ``q`` half of a packed ``[q | v]`` buffer, a rank slot of a gather
    buffer); ``out=x`` rotates in place."""
    if not isinstance(rotary, Rotary):
        raise TypeError(f"rope: rotary must be an xdot.Rotary, got {type(rotary).__name__}")
    _B, R, _C, H, D = split_heads(x, num_heads, "rope", even=True)
    if offset is None:
        offset = rotary.offset if rotary.offset is not None else 0
    tab = rotary.table(R, D, offset, x.device, _table_dtype(x))
    if out is not None and (out.shape != x.shape or out.dtype != x.dtype or out.device != x.device):
        raise ValueError("rope: out must match x in shape, dtype and device")
    from .qkprep import prep  # (imports this module)

    return prep(x, x.shape[-1], H, tab, alpha=alpha, out=out, inverse=inverse)
