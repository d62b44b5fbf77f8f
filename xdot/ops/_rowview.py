"""What the row-wise ops (:mod:`.rope`, :mod:`.headnorm`, :mod:`.gate`) share on the Python side: their
operand is ``(B, R, H*D)`` with a unit last stride, which the kernels take as the view it is."""
from __future__ import annotations

from typing import Tuple

import torch
from torch import Tensor


def split_heads(x: Tensor, heads: int, what: str, even: bool = False) -> Tuple[int, int, int, int, int]:
    """``(B, R, C, H, D)`` of ``x`` ``(B, R, C = H*D)``; ``even``: the rotation's rule, an even ``D``."""
    if x.dim() != 3:
        raise ValueError(f"{what} expects (B, R, H*D), got {tuple(x.shape)}")
    B, R, C = x.shape
    H = int(heads)
    if even:
        if H < 1 or C % H or (C // H) % 2:
            raise ValueError(f"{what}: {C} features over {H} heads is not an even head dim")
    elif H < 1 or C < 1 or C % H:
        raise ValueError(f"{what}: {C} features do not split over {H} heads")
    return B, R, C, H, C // H


def unit_inner(t: Tensor, *, in_place: bool = False, what: str = "") -> Tensor:
    """``t`` as the kernels take it: itself with a unit last stride, else a contiguous copy -- which an
    operand that is written ``in_place`` cannot be."""
    if t.stride(-1) == 1 or t.shape[-1] <= 1:
        return t
    if in_place:
        raise ValueError(f"{what}: in place needs a unit last stride")
    return t.contiguous()


def rotate_half(y: Tensor, cos: Tensor, sin: Tensor, inverse: bool) -> Tensor:
    """Half-split rotation of ``y`` (B, R, H, D) by a (R, D/2) table, in ``y``'s dtype."""
    h = y.shape[-1] // 2
    c = cos.to(y.dtype).view(1, cos.shape[0], 1, h)
    s = sin.to(y.dtype).view(1, cos.shape[0], 1, h)
    if inverse:
        s = -s
    y1, y2 = y[..., :h], y[..., h:]
    return torch.cat([y1 * c - y2 * s, y2 * c + y1 * s], dim=-1)
