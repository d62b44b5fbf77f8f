"""Which global rows of a sequence a rank owns: the row sharding, as pure functions.

``"contiguous"`` (the reference's, the default everywhere): rank ``r`` of ``n`` owns the global
rows ``[rR, (r+1)R)``.  Under a causal mask that is badly unbalanced: rank 0 attends to about
``1/(2n)`` of the columns, rank ``n-1`` to ``(2n-1)/(2n)``, and every collective waits for the
last rank.

``"zigzag"``: the sequence is cut into ``2n`` chunks and rank ``r`` owns chunk ``r`` and chunk
``2n-1-r``, so every rank holds about half live score tiles under a causal mask whatever ``n``
is.  Defined for any ``R >= 1``: with ``h0 = ceil(R/2)`` and ``h1 = R - h0``, chunk ``c < n`` has
``h0`` rows starting at global row ``c*h0``, chunk ``c >= n`` has ``h1`` rows starting at
``n*h0 + (c-n)*h1``; a rank's local rows ``[0, h0)`` are chunk ``r``, its rows ``[h0, R)`` chunk
``2n-1-r``.  With ``n = 1`` this is the identity.

The attention kernels know nothing about positions; what depends on the layout is the row side
of the generated masks (:mod:`xdot.ops.mask`), the rotary tables (:mod:`xdot.ops.rope`) and the
order of the gathered columns (rank-major: column ``j*R + i`` is local row ``i`` of rank ``j``).
"""
from __future__ import annotations

from functools import lru_cache
from typing import List, Sequence, Tuple

import torch

__all__ = ["LAYOUTS", "check_layout", "row_runs", "global_rows", "gathered_cols", "shard_rows", "unshard_rows"]

LAYOUTS = ("contiguous", "zigzag")
Run = Tuple[int, int, int]  # (local_start, length, global_start)


def check_layout(layout: str) -> str:
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {'|'.join(LAYOUTS)}, got {layout!r}")
    return layout


def row_runs(layout: str, rank: int, n: int, R: int) -> List[Run]:
    """The local rows of ``rank`` as runs ``(local_start, length, global_start)`` of consecutive
    global rows, in local order; runs adjacent in global order are merged (contiguous, ``n = 1``
    and the last zigzag rank give one run), empty ones dropped."""
    check_layout(layout)
    rank, n, R = int(rank), int(n), int(R)
    if n < 1 or not 0 <= rank < n or R < 0:
        raise ValueError(f"row_runs: rank {rank} of {n} ranks, {R} rows")
    if layout == "contiguous":
        runs = [(0, R, rank * R)]
    else:
        h0 = (R + 1) // 2
        h1 = R - h0
        runs = [(0, h0, rank * h0), (h0, h1, n * h0 + (n - 1 - rank) * h1)]
    out: List[Run] = []
    for ls, ln, gs in runs:
        if ln <= 0:
            continue
        if out and out[-1][0] + out[-1][1] == ls and out[-1][2] + out[-1][1] == gs:
            out[-1] = (out[-1][0], out[-1][1] + ln, out[-1][2])
        else:
            out.append((ls, ln, gs))
    return out


@lru_cache(maxsize=32)
def global_rows(layout: str, rank: int, n: int, R: int) -> torch.Tensor:
    """The global row index of every local row of ``rank``: int64 ``(R,)`` (cached per argument
    set, as :func:`gathered_cols`: the attention entry points ask every step; do not write to it)."""
    parts = [torch.arange(gs, gs + ln, dtype=torch.int64) for _ls, ln, gs in row_runs(layout, rank, n, R)]
    return torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int64)


@lru_cache(maxsize=8)
def gathered_cols(layout: str, n: int, R: int) -> torch.Tensor:
    """The global index of every column of the rank-major gathered side: int64 ``(n * R,)``."""
    return torch.cat([global_rows(layout, j, n, R) for j in range(int(n))])


def shard_rows(x: torch.Tensor, rank: int, world_size: int, dim: int = 1, layout: str = "contiguous") -> torch.Tensor:
    """The rows of the full sequence ``x`` (``world_size * R`` of them along ``dim``) that ``rank``
    owns under ``layout``, in local order: a view for one run, else a copy."""
    T = x.shape[dim]
    if T % int(world_size):
        raise ValueError(f"shard_rows: {T} rows do not divide over {world_size} ranks")
    runs = row_runs(layout, rank, world_size, T // int(world_size))
    if len(runs) == 1:
        return x.narrow(dim, runs[0][2], runs[0][1])
    return torch.cat([x.narrow(dim, gs, ln) for _ls, ln, gs in runs], dim=dim)


def unshard_rows(parts: Sequence[torch.Tensor], dim: int = 1, layout: str = "contiguous") -> torch.Tensor:
    """Inverse of :func:`shard_rows`: the full sequence from every rank's shard, in rank order."""
    parts = list(parts)
    n = len(parts)
    if n == 0:
        raise ValueError("unshard_rows: no shards")
    R = parts[0].shape[dim]
    if any(p.shape[dim] != R for p in parts):
        raise ValueError("unshard_rows: the shards must have equal row counts")
    gathered = torch.cat(parts, dim=dim)
    if check_layout(layout) == "contiguous" or n == 1:
        return gathered
    inv = torch.argsort(gathered_cols(layout, n, R)).to(gathered.device)
    return gathered.index_select(dim, inv)
