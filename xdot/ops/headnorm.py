"""QK-norm: RMSNorm over each head's ``D`` features of the projected ``k`` / ``q`` with a learnable
``(D,)`` gain, applied after the projections and before the rotation.

    r    = rsqrt(mean_j x[j]² + eps)        per (batch, row, head), over the head's D features
    y[i] = x[i] · r · weight[i]
    out  = alpha · rotate(y)                 (rotation only when a :class:`xdot.Rotary` is given:
                                              convention, offsets and table of :mod:`xdot.ops.rope`)

It is one pass at the spot where ``csrc/rope.hip`` touches ``k`` and ``q`` (``csrc/headnorm.hip``):
with a rotary the norm adds no launch and no read to the forward.  The backward folds the inverse
rotation in,

    gy = alpha · rotate⁻¹(g),  x̂ = x·r,  gw = gy ⊙ weight
    dx[i] = r · (gw[i] − x̂[i] · mean_j(gw[j]·x̂[j])),    dw[i] = Σ_(b,row,head) gy[i]·x̂[i]

and needs the pre-norm ``x`` (never reconstructed from the output: a gain may be zero) and ``r``.
``dw`` is an ordered sum: two runs give the same bits.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from .. import _ext
from ._rowview import rotate_half, split_heads, unit_inner
from .rope import Rotary, _table_dtype

__all__ = ["HeadRMSNorm", "head_rms_norm", "head_rms_norm_apply", "head_rms_norm_backward", "norm_packed"]

_HIP_DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def _dims(x: Tensor, num_heads: int, weight: Tensor, what: str) -> Tuple[int, int, int, int, int]:
    B, R, C, H, D = split_heads(x, num_heads, what)
    if tuple(weight.shape) != (D,):
        raise ValueError(f"{what}: weight must have shape ({D},), got {tuple(weight.shape)}")
    return B, R, C, H, D


def _check_table(cos, sin, R: int, D: int, what: str) -> None:
    if (cos is None) != (sin is None):
        raise ValueError(f"{what}: cos and sin go together")
    if cos is not None:
        if D % 2:
            raise ValueError(f"{what}: the rotation needs an even head dim, got {D}")
        if tuple(cos.shape) != (R, D // 2) or tuple(sin.shape) != (R, D // 2):
            raise ValueError(f"{what}: table {tuple(cos.shape)} does not fit (R, D/2) = ({R}, {D // 2})")


def _kernel_weight(weight: Tensor, x: Tensor) -> Tensor:
    """The gain as the kernels take it: ``x``'s dtype or fp32 (fp32 master weights stay fp32)."""
    w = weight.detach()
    if w.dtype != x.dtype and w.dtype != torch.float32:
        w = w.to(x.dtype)
    return w.contiguous()


def head_rms_norm_apply(x: Tensor, num_heads: int, weight: Tensor, eps: float = 1e-6, cos: Optional[Tensor] = None,
                        sin: Optional[Tensor] = None, alpha: float = 1.0, out: Optional[Tensor] = None,
                        save: bool = False) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    """``(out, rstd, saved)``; no autograd.  ``x`` is ``(B, R, H*D)``; ``out`` may be ``x`` (in
    place), another tensor, or None (a new contiguous one); ``cos`` / ``sin``: a table of
    :meth:`Rotary.table` (both None: no rotation).  ``rstd`` is ``(B, R, H)``, fp32 (fp64 for fp64
    inputs); ``saved`` is, with ``save``, a contiguous bit copy of ``x`` written by the same pass
    (what a backward needs after an in-place call), else None.  GPU bf16 / fp16 / fp32 tensors with
    unit last stride run ``csrc/headnorm.hip`` on the view as it is; everything else is the same
    formulas in torch (fp64 for fp64 inputs, else fp32)."""
    B, R, C, H, D = _dims(x, num_heads, weight, "head_rms_norm")
    _check_table(cos, sin, R, D, "head_rms_norm")
    if not float(eps) > 0.0:
        raise ValueError(f"head_rms_norm: eps must be positive, got {eps}")
    if _ext.use_hip(x) and x.dtype in _HIP_DTYPES:
        x = unit_inner(x, in_place=out is x, what="head_rms_norm")
        if out is None:
            out = torch.empty((B, R, C), dtype=x.dtype, device=x.device)
        rstd, saved = _ext.ops().headnorm_fwd(x, _kernel_weight(weight, x), cos, sin, H, float(eps), float(alpha), out,
                                              bool(save))
        return out, rstd, (saved if save else None)
    cdt = _table_dtype(x)
    saved = x.detach().clone(memory_format=torch.contiguous_format) if save else None
    xv = x.reshape(B, R, H, D).to(cdt)
    rstd = torch.rsqrt(xv.pow(2).mean(dim=-1) + float(eps))
    y = xv * rstd.unsqueeze(-1) * weight.detach().to(cdt)
    if cos is not None:
        y = rotate_half(y, cos, sin, False)
    if alpha != 1.0:
        y = y * alpha
    y = y.reshape(B, R, C).to(x.dtype)
    if out is None:
        return y, rstd, saved
    out.copy_(y)
    return out, rstd, saved


def head_rms_norm_backward(g: Tensor, x: Tensor, rstd: Tensor, num_heads: int, weight: Tensor,
                           cos: Optional[Tensor] = None, sin: Optional[Tensor] = None, alpha: float = 1.0,
                           out: Optional[Tensor] = None, need_dw: bool = True) -> Tuple[Tensor, Optional[Tensor]]:
    """``(dx, dw)`` of :func:`head_rms_norm_apply` from the gradient ``g`` w.r.t. its output, the
    pre-norm ``x`` and ``rstd``; no autograd.  ``alpha`` is the factor of the backward; ``out`` may
    be ``g`` (``dx`` written over it), another tensor, or None.  ``dw`` has ``weight``'s dtype and is
    an ordered sum (bitwise reproducible); None without ``need_dw``."""
    B, R, C, H, D = _dims(g, num_heads, weight, "head_rms_norm_backward")
    _check_table(cos, sin, R, D, "head_rms_norm_backward")
    if tuple(x.shape) != (B, R, C) or tuple(rstd.shape) != (B, R, H):
        raise ValueError("head_rms_norm_backward: x must be shaped like g and rstd (B, R, H)")
    if _ext.use_hip(g) and g.dtype in _HIP_DTYPES:
        g = unit_inner(g, in_place=out is g, what="head_rms_norm_backward")
        x = unit_inner(x)
        if out is None:
            out = torch.empty((B, R, C), dtype=g.dtype, device=g.device)
        w = _kernel_weight(weight, g)
        dw = _ext.ops().headnorm_bwd(g, x, rstd, w, cos, sin, H, float(alpha), out, bool(need_dw))
        if not need_dw:
            return out, None
        return out, (dw if dw.dtype == weight.dtype else dw.to(weight.dtype))
    cdt = _table_dtype(g)
    gy = g.reshape(B, R, H, D).to(cdt)
    if cos is not None:
        gy = rotate_half(gy, cos, sin, True)
    if alpha != 1.0:
        gy = gy * alpha
    r = rstd.to(cdt).unsqueeze(-1)
    xh = x.reshape(B, R, H, D).to(cdt) * r
    gw = gy * weight.detach().to(cdt)
    dx = (r * (gw - xh * (gw * xh).mean(dim=-1, keepdim=True))).reshape(B, R, C).to(g.dtype)
    dw = (gy * xh).sum(dim=(0, 1, 2)).to(weight.dtype) if need_dw else None
    if out is None:
        return dx, dw
    out.copy_(dx)
    return out, dw


def _table(x: Tensor, ncols: int, H: int, rotary: Optional[Rotary], offset, what: str):
    if rotary is None:
        return None
    if not isinstance(rotary, Rotary):
        raise TypeError(f"{what}: rotary must be an xdot.Rotary or None, got {type(rotary).__name__}")
    D = ncols // H
    if D % 2:
        raise ValueError(f"{what}: the rotation needs an even head dim, got {D}")
    if offset is None:
        offset = rotary.offset if rotary.offset is not None else 0
    return rotary.table(x.shape[1], D, offset, x.device, _table_dtype(x))


def head_rms_norm(x: Tensor, num_heads: int, weight: Tensor, eps: float = 1e-6, *, rotary: Optional[Rotary] = None,
                  offset=None, alpha: float = 1.0, out: Optional[Tensor] = None) -> Tensor:
    """``alpha · rotate(x · rsqrt(mean x² + eps) · weight)`` per head of ``x`` ``(B, R, H*D)``, the
    mean over the head's ``D`` features and ``weight`` of shape ``(D,)``; the rotation only with a
    ``rotary`` (row ``r`` at position ``offset + r``, offsets and row runs as :func:`xdot.rope`).
    Autograd-aware w.r.t. ``x`` and ``weight``.  ``x`` may be a strided view with unit last stride
    (the ``q`` half of a packed ``[q | v]`` buffer, a rank slot of a gather buffer); ``out=x``
    works in place (the backward then reads the pass's own copy of the input)."""
    what = "head_rms_norm"
    _B, _R, C, H, _D = _dims(x, num_heads, weight, what)
    if not float(eps) > 0.0:
        raise ValueError(f"{what}: eps must be positive, got {eps}")
    tab = _table(x, C, H, rotary, offset, what)
    if out is not None and (out.shape != x.shape or out.dtype != x.dtype or out.device != x.device):
        raise ValueError(f"{what}: out must match x in shape, dtype and device")
    from .qkprep import prep  # (imports this module)

    return prep(x, C, H, tab, weight, eps, alpha, out=out)


def norm_packed(qv: Tensor, ncols: int, num_heads: int, weight: Tensor, eps: float = 1e-6,
                rotary: Optional[Rotary] = None, offset=None, alpha: float = 1.0,
                bwd_alpha: Optional[float] = None) -> Tensor:
    """A copy of ``qv`` with its first ``ncols`` features normalised (and, with ``rotary``, rotated
    at ``offset``) as one autograd node (the ``q`` half of a packed ``[q | v]``; all of a ``k``):
    :func:`xdot.ops.qkprep.prep` with the table built here.  ``bwd_alpha``: the factor of the
    backward (default ``alpha``; 1 where ``alpha`` is the row side's pre-scale)."""
    from .qkprep import prep  # (imports this module)

    ncols, H = int(ncols), int(num_heads)
    _dims(qv[..., :ncols], H, weight, "norm_packed")
    return prep(qv, ncols, H, _table(qv, ncols, H, rotary, offset, "norm_packed"), weight, eps, alpha, bwd_alpha)


class HeadRMSNorm(nn.Module):
    """``HeadRMSNorm(dim, eps=1e-6)``: the gain of a per-head RMSNorm, one parameter ``weight`` of
    shape ``(dim,)`` initialised to ones -- a description plus a parameter, as
    :class:`xdot.Rotary` is a description plus a table.  Calling it normalises ``x``
    ``(B, R, H*dim)`` over every head's ``dim`` features (:func:`head_rms_norm`)."""

    def __init__(self, dim: int, eps: float = 1e-6):
        super().__init__()
        dim, eps = int(dim), float(eps)
        if dim < 1:
            raise ValueError(f"HeadRMSNorm: dim must be positive, got {dim}")
        if not eps > 0.0:
            raise ValueError(f"HeadRMSNorm: eps must be positive, got {eps}")
        self.dim, self.eps = dim, eps
        self.weight = nn.Parameter(torch.ones(dim))

    def forward(self, x: Tensor, *, rotary: Optional[Rotary] = None, offset=None, alpha: float = 1.0,
                out: Optional[Tensor] = None) -> Tensor:
        if x.dim() != 3 or x.shape[-1] % self.dim:
            raise ValueError(f"HeadRMSNorm({self.dim}) expects (B, R, H*{self.dim}), got {tuple(x.shape)}")
        return head_rms_norm(x, x.shape[-1] // self.dim, self.weight, self.eps, rotary=rotary, offset=offset,
                             alpha=alpha, out=out)

    def extra_repr(self) -> str:
        return f"{self.dim}, eps={self.eps:g}"
