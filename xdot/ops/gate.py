"""Gated attention: a sigmoid gate on the merged attention output, before the output projection
(Qiu et al. 2025, "Gated Attention for Large Language Models"; Qwen3-Next).

    o' = o ⊙ σ(g)          o: (B, R, H·D);  g: (B, R, H·D) -- one gate value per feature
                            ("elementwise") -- or (B, R, H) -- one per (row, head), broadcast over
                            the head's D features ("headwise"); the kind follows from g's last dim

The sigmoid is evaluated in a form that cannot overflow or cancel, from ``e = exp(-|g|)`` and
``r = 1 / (1 + e)``:

    σ = g ≥ 0 ? r : e·r,     σ' = e·r²           (never ``σ - σ²``, never ``1 - σ``)

and the backward is

    do = do' ⊙ σ(g),   dg = do' ⊙ o ⊙ σ'(g)     (headwise: Σ over the head's D features of do'·o,
                                                  times σ'; an ordered fp32 sum, rounded once)

GPU bf16 / fp16 / fp32 tensors run ``csrc/gate.hip`` (one launch each way, 16-byte loads where the
head width and the strides allow, any width otherwise, views with row strides as they are); CPU
tensors, ``backend='torch'`` and other dtypes run the same formulae in torch, in fp32 (fp64 for fp64
tensors) with one cast.  The product is plain IEEE: a NaN in ``o`` stays NaN, ``g = -inf`` gives
``±0`` and ``g = +inf`` gives ``o`` bit for bit.  A zero pre-activation halves the output.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from .. import _ext
from ._rowview import split_heads, unit_inner

__all__ = ["sigmoid_gate", "gate_apply", "gate_backward"]

_HIP_DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def _dims(o: Tensor, g: Tensor, heads: int, what: str) -> Tuple[int, int, int, int, bool]:
    B, R, C, H, _D = split_heads(o, heads, what)
    if g.dim() != 3 or tuple(g.shape[:2]) != (B, R) or g.shape[2] not in (C, H):
        raise ValueError(f"{what}: g must be ({B}, {R}, {C}) or ({B}, {R}, {H}), got {tuple(g.shape)}")
    if g.dtype != o.dtype or g.device != o.device:
        raise ValueError(f"{what}: g must have o's dtype and device, got {g.dtype} on {g.device}")
    return B, R, C, H, g.shape[2] != C


def _sigmoid_parts(g: Tensor):
    """``(σ, σ')`` of ``g`` in fp32 (fp64 for fp64) by the kernels' formulae."""
    gv = g.detach().to(torch.float64 if g.dtype == torch.float64 else torch.float32)
    e = torch.exp(-gv.abs())
    r = 1.0 / (1.0 + e)
    return torch.where(gv >= 0, r, e * r), e * r * r


def _mode(vec: Optional[bool]) -> int:
    return -1 if vec is None else int(bool(vec))


def gate_apply(o: Tensor, g: Tensor, heads: int, out: Optional[Tensor] = None, vec: Optional[bool] = None) -> Tensor:
    """``o' = o ⊙ σ(g)``; no autograd.  Out of place: ``out`` (None: a new contiguous tensor) may not
    share memory with ``o`` or ``g``.  One launch on the GPU.  ``vec`` (GPU kernels only): None picks
    16-byte lane steps where the head width, pointers and strides allow; False forces one element per
    step; True asks for 16-byte steps and raises where they cannot be taken."""
    B, R, C, H, headwise = _dims(o, g, heads, "gate_apply")
    if out is not None and (out.shape != o.shape or out.dtype != o.dtype or out.device != o.device):
        raise ValueError("gate_apply: out must match o in shape, dtype and device")
    if _ext.use_hip(o) and o.dtype in _HIP_DTYPES:
        if out is None:
            out = torch.empty((B, R, C), dtype=o.dtype, device=o.device)
        _ext.ops().gate_apply(unit_inner(o.detach()), unit_inner(g.detach()), H, out, _mode(vec))
        return out
    sig, _ = _sigmoid_parts(g)
    ov = o.detach().to(sig.dtype)
    y = (ov.reshape(B, R, H, C // H) * sig.unsqueeze(-1)).reshape(B, R, C) if headwise else ov * sig
    y = y.to(o.dtype)
    if out is None:
        return y
    out.copy_(y)
    return out


def gate_backward(dy: Tensor, o: Tensor, g: Tensor, heads: int, out: Optional[Tensor] = None,
                  vec: Optional[bool] = None) -> Tuple[Tensor, Tensor]:
    """``(do, dg)`` of :func:`gate_apply` from the gradient ``dy`` w.r.t. its output, the ungated
    ``o`` and ``g``; no autograd.  ``out`` may be ``dy`` (``do`` written over it), another tensor, or
    None (it may not overlap ``dy`` otherwise); ``dg`` is a new tensor shaped like ``g``.  The
    headwise ``dg`` is an ordered sum: two runs give the same bits, and its order is that of the lane
    step in use (``vec`` as in :func:`gate_apply`).  One launch on the GPU."""
    B, R, C, H, headwise = _dims(o, g, heads, "gate_backward")
    if dy.shape != o.shape or dy.dtype != o.dtype or dy.device != o.device:
        raise ValueError("gate_backward: dy must match o in shape, dtype and device")
    if out is not None and (out.shape != o.shape or out.dtype != o.dtype or out.device != o.device):
        raise ValueError("gate_backward: out must match o in shape, dtype and device")
    if _ext.use_hip(o) and o.dtype in _HIP_DTYPES:
        dy = unit_inner(dy, in_place=out is dy, what="gate_backward")
        if out is None:
            out = torch.empty((B, R, C), dtype=o.dtype, device=o.device)
        dg = _ext.ops().gate_backward(dy.detach(), unit_inner(o.detach()), unit_inner(g.detach()), H, out, _mode(vec))
        return out, dg
    sig, sp = _sigmoid_parts(g)
    dv, ov = dy.detach().to(sig.dtype), o.detach().to(sig.dtype)
    if headwise:
        D = C // H
        do = (dv.reshape(B, R, H, D) * sig.unsqueeze(-1)).reshape(B, R, C)
        dg = (dv * ov).reshape(B, R, H, D).sum(dim=-1) * sp
    else:
        do = dv * sig
        dg = dv * ov * sp
    do, dg = do.to(o.dtype), dg.to(o.dtype)
    if out is None:
        return do, dg
    out.copy_(do)
    return out, dg


class _SigmoidGateFn(torch.autograd.Function):
    @staticmethod
    @_ext.pinned
    def forward(ctx, o, g, heads):
        ctx.heads = heads
        ctx.save_for_backward(o, g)
        return gate_apply(o, g, heads)

    @staticmethod
    @_ext.pinned
    def backward(ctx, dy):
        o, g = ctx.saved_tensors
        do, dg = gate_backward(dy, o, g, ctx.heads)
        return (do if ctx.needs_input_grad[0] else None), (dg if ctx.needs_input_grad[1] else None), None


def sigmoid_gate(o: Tensor, g: Tensor, heads: int) -> Tensor:
    """``o ⊙ σ(g)`` for ``o`` ``(B, R, heads·D)``, differentiable w.r.t. both.  ``g`` is
    ``(B, R, heads·D)`` (one gate value per feature) or ``(B, R, heads)`` (one per head, broadcast over
    its ``D`` features); the kind follows from its last dimension.  Row-strided views work as they
    are.  ``g = 0`` halves ``o``."""
    if isinstance(g, Tensor) and isinstance(o, Tensor) and g.dtype != o.dtype:
        g = g.to(o.dtype)
    _dims(o, g, heads, "sigmoid_gate")
    return _SigmoidGateFn.apply(o, g, int(heads))
