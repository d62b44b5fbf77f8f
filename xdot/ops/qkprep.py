"""The one step between a projection and the attention: the first ``ncols`` features of a
``(B, R, ·)`` tensor -- all of a ``k``, the ``q`` part of a packed ``[q | v]`` -- normalised per head
(with a gain: QK-norm, :mod:`.headnorm`) and / or rotated (with a table: :mod:`.rope`).  A rotation
is the norm pass without a gain: one pair of functions without autograd, and one autograd node over
them that :func:`xdot.rope`, :func:`xdot.head_rms_norm` and the module's per-op paths share."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from .. import _ext
from .headnorm import head_rms_norm_apply, head_rms_norm_backward
from .rope import rope_apply

__all__ = ["prep", "prep_apply", "prep_backward"]


def prep_apply(x: Tensor, heads: int, tab, gain: Optional[Tensor] = None, eps: float = 1e-6, alpha: float = 1.0,
               out: Optional[Tensor] = None, save: bool = False) -> Tuple[Tensor, Optional[Tensor], Optional[Tensor]]:
    """``(out, rstd, saved)``; no autograd.  ``tab``: a ``(cos, sin)`` of :meth:`Rotary.table` or None.
    Without a ``gain`` :func:`rope_apply` (no ``rstd``, no ``saved``), with one :func:`head_rms_norm_apply`."""
    if gain is None:
        return rope_apply(x, heads, *tab, alpha=alpha, out=out), None, None
    return head_rms_norm_apply(x, heads, gain, eps, *(tab or (None, None)), alpha=alpha, out=out, save=save)


def prep_backward(g: Tensor, heads: int, tab, gain: Optional[Tensor] = None, x: Optional[Tensor] = None,
                  rstd: Optional[Tensor] = None, alpha: float = 1.0, out: Optional[Tensor] = None,
                  need_dw: bool = True) -> Tuple[Tensor, Optional[Tensor]]:
    """``(dx, dw)`` of :func:`prep_apply` from the gradient ``g`` w.r.t. its output; no autograd.  Without
    a ``gain`` the inverse rotation (no ``dw``), with one :func:`head_rms_norm_backward`."""
    if gain is None:
        return rope_apply(g, heads, *tab, inverse=True, alpha=alpha, out=out), None
    return head_rms_norm_backward(g, x, rstd, heads, gain, *(tab or (None, None)), alpha=alpha, out=out, need_dw=need_dw)


def _prefix(t: Tensor, ncols: int, run):
    """``run(src, dst)`` on the first ``ncols`` features of ``t`` into a new tensor, the rest copied
    (``run(t, None)`` makes the new tensor where ``ncols`` covers ``t``) -> ``(new, run's result)``."""
    if ncols == t.shape[-1]:
        res = run(t, None)
        return res[0], res
    new = torch.empty(t.shape, dtype=t.dtype, device=t.device)
    res = run(t[..., :ncols], new[..., :ncols])
    new[..., ncols:].copy_(t[..., ncols:])
    return new, res


class _PrepFn(torch.autograd.Function):
    """:func:`prep_apply` on the first ``ncols`` features of ``x``.  ``mode``: 0 a new tensor, 1 in
    place on ``x``, 2 into ``out``.  ``inverse`` (no gain): the inverse rotation, which is the
    rotation's own backward.  Kept for the backward: the table, and with a gain ``rstd`` and the
    pre-norm input -- the input itself, or where it is overwritten (``mode`` 1) the pass's own copy."""

    @staticmethod
    @_ext.pinned
    def forward(ctx, x, gain, out, ncols, H, tab, eps, inverse, alpha, bwd_alpha, mode):
        need = gain is not None and (ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        src = x if ncols == x.shape[-1] else x[..., :ncols]

        def run(s, dst):
            if inverse:
                return prep_backward(s, H, tab, alpha=alpha, out=dst) + (None,)
            return prep_apply(s, H, tab, gain, eps, alpha, out=dst, save=need and mode == 1)

        if mode == 0:
            res, (_, rstd, kept) = _prefix(x, ncols, run)
        else:
            res = x if mode == 1 else out
            _, rstd, kept = run(src, res[..., :ncols])
            ctx.mark_dirty(res)
        ctx.tab, ctx.args = tab, (ncols, H, inverse, bwd_alpha)
        if need:
            ctx.save_for_backward(kept if mode == 1 else src, gain, rstd)
        return res

    @staticmethod
    @_ext.pinned
    def backward(ctx, g):
        ncols, H, inverse, bwd_alpha = ctx.args
        xs, gain, rstd = ctx.saved_tensors or (None, None, None)

        def run(s, dst):
            if inverse:
                return prep_apply(s, H, ctx.tab, alpha=bwd_alpha, out=dst)[:2]
            return prep_backward(s, H, ctx.tab, gain, xs, rstd, bwd_alpha, out=dst, need_dw=ctx.needs_input_grad[1])

        gx, (_, dw) = _prefix(g, ncols, run)
        return gx, dw, None, None, None, None, None, None, None, None, None


def prep(x: Tensor, ncols: int, heads: int, tab, gain: Optional[Tensor] = None, eps: float = 1e-6, alpha: float = 1.0,
         bwd_alpha: Optional[float] = None, out: Optional[Tensor] = None, inverse: bool = False) -> Tensor:
    """``x`` with its first ``ncols`` features through :func:`prep_apply`, as one autograd node w.r.t.
    ``x`` and ``gain``; ``out``: None (a new tensor), ``x`` (in place) or another tensor.
    ``bwd_alpha``: the factor of the backward (default ``alpha``; 1 where ``alpha`` is the row side's
    pre-scale, whose gradient the attention already returns w.r.t. the unscaled rows)."""
    if inverse and gain is not None:
        raise ValueError("prep: inverse is the rotation's alone (no gain)")
    mode = 0 if out is None else (1 if out is x else 2)
    return _PrepFn.apply(x, gain, out if mode == 2 else None, int(ncols), int(heads), tab, float(eps), bool(inverse),
                         float(alpha), float(alpha if bwd_alpha is None else bwd_alpha), mode)
