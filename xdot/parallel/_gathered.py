"""How the kernels of one attention call read the gathered side: a packed ``[q | v]`` buffer, ``Hg`` heads each
on the wire and in the saved tensors, ``H`` heads for a kernel family without a grouped form.  The flash path
(:mod:`xdot.parallel.attention`) and the ring (:mod:`xdot.parallel.ring`) build one :class:`GatheredSide` in
``forward`` and keep it on ``ctx``, so a launch site names only what varies."""
from __future__ import annotations

import torch
from torch import Tensor

from ..ops import flash
from ..utils.env import FLAGS
from . import _ref


def _native_gqa(k: Tensor, H: int) -> bool:
    """The kernels index a narrower gathered side themselves: the 16-bit families up to head dim 128.  Exact
    fp32, split-bf16 and the wide heads read repeated heads (:meth:`GatheredSide.view`, its ``fold`` for the gradients)."""
    return k.dtype != torch.float32 and k.shape[-1] // H <= 128


def _q_width(k, H, Hg):
    """Columns of the ``q`` half of a packed ``[q | v]``: ``Hg`` heads of the row side's head dim."""
    return k.shape[-1] if not Hg else Hg * (k.shape[-1] // H)


def _expand_heads(g: Tensor, H: int, Hg: int) -> Tensor:
    """Packed ``[q | v]`` (..., 2 * Hg * D) -> (..., 2 * H * D): every gathered head repeated for
    the row heads of its group (one copy)."""
    D = g.shape[-1] // (2 * Hg)
    lead = tuple(g.shape[:-1])
    return g.reshape(*lead, 2, Hg, 1, D).expand(*lead, 2, Hg, H // Hg, D).reshape(*lead, 2 * H * D)


def _fold_heads(d: Tensor, H: int, Hg: int, dtype) -> Tensor:
    """Packed ``[dq | dv]`` (..., 2 * H * D) per row head -> (..., 2 * Hg * D) in ``dtype``: the sum
    over each group, in fp32 and in head order (deterministic)."""
    D = d.shape[-1] // (2 * H)
    lead = tuple(d.shape[:-1])
    x = d.reshape(*lead, 2, Hg, H // Hg, D)
    acc = x[..., 0, :].float()
    for j in range(1, H // Hg):
        acc = acc + x[..., j, :]
    return acc.reshape(*lead, 2 * Hg * D).to(dtype)


def wire_dtype(dtype):
    """The dtype gathered-side gradient partials travel in: a 16-bit dtype itself (one rounding per partial)
    unless ``XDOT_GRAD_FP32``, else the compute dtype (fp64 for fp64, fp32 otherwise)."""
    own = dtype == torch.float64 or (dtype in (torch.bfloat16, torch.float16) and not FLAGS.grad_fp32)
    return dtype if own else torch.float32


def pop_sinks(ctx, saved: list):
    """The attention-sink logits a forward saved last (``ctx.has_sinks``), taken off ``saved``, or None."""
    return saved.pop() if getattr(ctx, "has_sinks", False) else None


def sinks_grad(ds, sinks):
    """The sinks' gradient in their dtype (None without sinks)."""
    return None if ds is None else ds.to(sinks.dtype)


class GatheredSide:
    """The constants of one call's flash launches and the kernels' view of a ``[q | v]`` buffer.  ``Hg``: heads on the
    wire and in the saved buffers (None: ``H``), ``Cq`` columns in the ``q`` half.  ``expand`` (None: decided here):
    grouped heads in a family without a grouped kernel; the kernels read a copy with every head repeated (``kC``
    columns a half, ``kHg`` None) and their ``[dq | dv]`` partials are folded.  ``x`` is what :meth:`view` gave."""

    __slots__ = ("H", "Hg", "scale", "use_hip", "expand", "prescaled", "fp32_mode", "Cq", "kC", "kHg")

    def __init__(self, k: Tensor, H: int, Hg, scale: float, use_hip: bool, prescaled=False, fp32_mode=0, expand=None):
        self.H, self.Hg, self.scale, self.use_hip, self.prescaled, self.fp32_mode = H, Hg, scale, use_hip, prescaled, fp32_mode
        self.expand = (bool(Hg) and use_hip and not _native_gqa(k, H)) if expand is None else expand
        self.Cq = _q_width(k, H, Hg)
        self.kC, self.kHg = (k.shape[-1], None) if self.expand else (self.Cq, Hg)

    def view(self, g: Tensor) -> Tensor:
        """The buffer the kernels read for the wire buffer ``g``: ``g`` itself, or its heads repeated (one copy)."""
        return _expand_heads(g, self.H, self.Hg) if self.expand else g

    def halves(self, x: Tensor):  # (the launches below slice inline: one call level less per launch)
        return x[..., :self.kC], x[..., self.kC:]

    def fold(self, part: Tensor, dtype) -> Tensor:
        """A kernel view's ``[dq | dv]`` partial at the wire width: the group sums in ``dtype``, or ``part`` itself."""
        return _fold_heads(part, self.H, self.Hg, dtype) if self.expand else part

    def fwd(self, k, x, mk, sbuf=None):
        return flash.fwd(k, x[..., :self.kC], x[..., self.kC:], mk, self.H, self.scale, prescaled=self.prescaled,
                         fp32_mode=self.fp32_mode, sbuf=sbuf, Hg=self.kHg)

    def fwd_partial(self, k, x, mk, opart, lpart, slot, ns):
        flash.fwd_partial(k, x[..., :self.kC], x[..., self.kC:], mk, self.H, self.scale, opart, lpart, slot, ns,
                          self.prescaled, self.fp32_mode, self.kHg)

    def bwd_cols(self, do, k, x, o, lse, mk, delta, fp32_out, **kw):
        """``fp32_out``: fp32 partials (always where they are folded).  ``kw``: lse2, score buffers, passes, out_dkv."""
        return flash.bwd_cols(do, k, x[..., :self.kC], x[..., self.kC:], o, lse, mk, self.H, self.scale, delta, Hg=self.kHg,
                              fp32_out=fp32_out or self.expand, prescaled=self.prescaled, fp32_mode=self.fp32_mode, **kw)

    def bwd_rows(self, do, k, x, lse, delta, mk, sbuf, dsbuf):
        return flash.bwd_rows(do, k, x[..., :self.kC], x[..., self.kC:], lse, delta, mk, self.H, self.scale, Hg=self.kHg,
                              nsplit=FLAGS.rows_split, prescaled=self.prescaled, fp32_mode=self.fp32_mode, sbuf=sbuf, dsbuf=dsbuf)

    def bwd_rows_partial(self, do, k, x, lse, delta, mk, dpart, slot, ns):
        flash.bwd_rows_partial(do, k, x[..., :self.kC], x[..., self.kC:], lse, delta, mk, self.H, self.scale, dpart, slot, ns,
                               self.prescaled, self.fp32_mode, self.kHg)

    def ref_fwd(self, k, g, mask, rows=lambda t: t):  # (torch: the wire buffer; ``rows``: each half's layout adapter)
        return _ref.block_fwd(k, rows(g[..., :self.Cq]), rows(g[..., self.Cq:]), mask, self.H, self.scale, self.Hg)

    def ref_bwd(self, do, k, g, lse, delta, mask, rows=lambda t: t):
        return _ref.block_bwd(do, k, rows(g[..., :self.Cq]), rows(g[..., self.Cq:]), lse, delta, mask, self.H, self.scale,
                              self.Hg)

    def sink_fold(self, o, lse, sinks):
        """``lse' = logaddexp(lse, s_h)``, ``o' = exp(lse - lse') o``: the backward runs unchanged on the folded pair."""
        if sinks is None:
            return o, lse
        return (flash.sink_fold if self.use_hip else _ref.sink_fold)(o, lse, sinks, self.H)
