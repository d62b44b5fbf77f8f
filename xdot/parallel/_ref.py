"""The attention maths in torch, written once: the oracle of the CPU tests and the path that CPU
tensors (and GPU dtypes the kernels do not take) run.  Row side ``k`` (B, R, H*dh), one column
segment of the gathered side ``kc`` (B, T, Hg*dh) / ``vc`` (B, T, Hg*dv), ``mask`` bool (B, R, T)
with True = masked, or None.  ``Hg`` (None: ``H``) gathered heads: row head ``h`` reads gathered
head ``h // (H // Hg)`` (grouped-query attention, the ``repeat_interleave`` convention).  fp64 stays fp64, everything else computes in fp32.  The flash and
the ring path are layout adapters over these functions (:mod:`xdot.parallel.attention`,
:mod:`xdot.parallel.ring`)."""
from __future__ import annotations

import torch


def compute_dtype(x):
    return torch.float64 if x.dtype == torch.float64 else torch.float32


def heads(x, H: int, cdt):
    """(B, L, H*d) -> (B, H, L, d) in the compute dtype."""
    B, L, C = x.shape
    return x.reshape(B, L, H, C // H).transpose(1, 2).to(cdt)


def gathered_heads(x, H: int, Hg, cdt):
    """(B, T, Hg*d) -> (B, H, T, d) in the compute dtype: every gathered head repeated for its group."""
    xh = heads(x, Hg or H, cdt)
    return xh if not Hg or Hg == H else xh.repeat_interleave(H // Hg, dim=1)


def _fold(x, H: int, Hg):
    """(B, H, T, d) per-row-head gathered-side gradients -> (B, Hg, T, d): summed over each group."""
    if not Hg or Hg == H:
        return x
    B, _, T, d = x.shape
    return x.reshape(B, Hg, H // Hg, T, d).sum(2)


def _merge(x):
    """(B, H, L, d) -> (B, L, H*d)"""
    return x.transpose(1, 2).reshape(x.shape[0], x.shape[2], -1)


def _scores(kh, qh, mask, scale):
    s = torch.matmul(kh, qh.transpose(-1, -2)) * scale
    if mask is not None:
        s = s.masked_fill(mask.unsqueeze(1), -float("inf"))
    return s


def delta(do, o, H: int, cdt):
    """δ = rowsum(dO ⊙ O) per head: (B, H, R)."""
    return (heads(do, H, cdt) * heads(o, H, cdt)).sum(-1)


def block_fwd(k, kc, vc, mask, H: int, scale: float, Hg=None):
    """One column segment of the forward -> (o (B, R, H*dv) normalised over the segment, lse
    (B, H, R)), compute dtype; a row the segment masks entirely gets o = 0, lse = -inf."""
    cdt = compute_dtype(k)
    s = _scores(heads(k, H, cdt), gathered_heads(kc, H, Hg, cdt), mask, scale)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.clamp_min(torch.finfo(cdt).min).unsqueeze(-1))
    return _merge(torch.matmul(p, gathered_heads(vc, H, Hg, cdt))), lse


def combine(parts, dtype):
    """Merge segment partials [(o, lse)] -> (o in ``dtype``, lse); NaN for fully masked rows.  One
    part comes back bit for bit on its live rows (its weight is exactly 1)."""
    L = torch.stack([l for _, l in parts])                      # (S, B, H, R)
    lse = torch.logsumexp(L, dim=0)
    w = torch.exp(L - lse.unsqueeze(0))                         # NaN only where every segment is -inf
    H = lse.shape[1]
    o = sum(wi.transpose(1, 2).repeat_interleave(oi.shape[-1] // H, dim=-1) * oi
            for wi, (oi, _) in zip(w, parts))
    return o.to(dtype), lse


def sink_fold(o, lse, sinks, H: int):
    """One sink logit per head (``sinks`` (H,), not scaled) folded into a finished forward ->
    (o' in o's dtype, lse'): ``lse' = logaddexp(lse, s_h)``, ``o' = exp(lse - lse') * o``; a fully
    masked row (``lse = -inf``, NaN in ``o``) gives 0 and ``lse' = s_h``.  ``s_h = -inf`` is the
    identity (a fully masked row stays NaN / -inf)."""
    cdt = lse.dtype
    s = sinks.detach().to(cdt).view(1, H, 1)
    new = torch.logaddexp(lse, s)
    g = torch.where(s > -float("inf"), torch.exp(lse - new), torch.ones_like(new))  # -inf - -inf: weight 1
    oh = heads(o, H, cdt)
    dead = ((lse == -float("inf")) & (s > -float("inf"))).unsqueeze(-1)
    oh = torch.where(dead, torch.zeros_like(oh), oh * g.unsqueeze(-1))  # selected, not multiplied: o is NaN there
    return _merge(oh).to(o.dtype), new


def sink_grad(delta, lse, sinks):
    """``ds`` (H,) ``= -sum_{b,r} exp(s_h - lse') * delta`` from the folded ``lse'`` and the δ of the
    folded output, compute dtype; 0 for ``s_h = -inf``."""
    s = sinks.detach().to(lse.dtype).view(1, -1, 1)
    w = torch.where(s > -float("inf"), torch.exp(s - lse), torch.zeros_like(lse))
    return -torch.where(w == 0, torch.zeros_like(delta), w * delta).sum(dim=(0, 2))


def block_bwd(do, k, kc, vc, lse, delta, mask, H: int, scale: float, Hg=None):
    """Gradients of one column segment given the whole row's ``lse`` and ``delta`` (B, H, R) ->
    (dk (B, R, H*dh), dq (B, T, Hg*dh), dv (B, T, Hg*dv)), compute dtype; dq / dv summed over each
    group of row heads."""
    cdt = compute_dtype(k)
    kh, qh, vh, doh = heads(k, H, cdt), gathered_heads(kc, H, Hg, cdt), gathered_heads(vc, H, Hg, cdt), heads(do, H, cdt)
    p = torch.exp(_scores(kh, qh, mask, scale) - lse.unsqueeze(-1))
    ds = p * (torch.matmul(doh, vh.transpose(-1, -2)) - delta.unsqueeze(-1)) * scale
    return (_merge(torch.matmul(ds, qh)), _merge(_fold(torch.matmul(ds.transpose(-1, -2), kh), H, Hg)),
            _merge(_fold(torch.matmul(p.transpose(-1, -2), doh), H, Hg)))
