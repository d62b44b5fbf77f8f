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


def decode_mask(col_pos, pos0: int, Rn: int, window: int = 0):
    """The decode visibility rule as a dense mask (B, Rn, Tcap), True = masked: slot ``c`` of a cache whose
    slot positions are ``col_pos`` (B, Tcap), -1 = empty, is visible to new row ``i`` at ``p_i = pos0 + i``
    iff ``0 <= col_pos[c] <= p_i`` and (no ``window`` or ``col_pos[c] > p_i - window``):
    ``StructuredMask(causal=True, window=window)`` for those rows, whatever order the cache was filled in."""
    p = pos0 + torch.arange(Rn, device=col_pos.device, dtype=torch.int64).view(1, Rn, 1)
    c = col_pos.to(torch.int64).unsqueeze(1)
    m = (c < 0) | (c > p)
    return m | (c <= p - int(window)) if window else m


def decode(rows, qc, vc, col_pos, pos0: int, H: int, scale: float, window: int = 0, Hg=None):
    """``Rn`` new rows against one cache shard -> (o (B, Rn, H*dv), lse (B, H, Rn)), compute dtype; a row
    that sees nothing gets o = 0, lse = -inf."""
    return block_fwd(rows, qc, vc, decode_mask(col_pos, pos0, rows.shape[1], window), H, scale, Hg)


def paged_gather(qpool, vpool, pool_pos, table, npages, qscale=None, vscale=None):
    """A paged cache as the dense one every sequence would have: ``qpool`` / ``vpool`` (P, S, Hg*d) and
    ``pool_pos`` (P, S) gathered by ``table`` (B, maxp) -> (qc, vc (B, maxp*S, Hg*d), col_pos (B, maxp*S) int64);
    the slots of a hole (-1), of an entry outside the pool and of the entries at or past ``npages[b]`` are empty
    (-1).  No host synchronisation.  An fp8 pool's ``qscale`` / ``vscale`` (P, Hg, S) come along as the dense fp8
    cache's (B, Hg, maxp*S): five results."""
    (B, maxp), (P, S) = table.shape, pool_pos.shape
    t = table.to(torch.int64)
    live = (t >= 0) & (t < P) & (torch.arange(maxp, device=table.device).unsqueeze(0) < npages.to(torch.int64).unsqueeze(1))
    idx = t.clamp(0, P - 1).reshape(-1)

    def pages(x):  # one-byte dtypes are gathered as bytes
        if x.element_size() == 1:
            return x.view(torch.uint8).index_select(0, idx).view(x.dtype)
        return x.index_select(0, idx)

    qc, vc = (pages(x).reshape(B, maxp * S, x.shape[-1]) for x in (qpool, vpool))
    pos = pool_pos.index_select(0, idx).reshape(B, maxp, S).to(torch.int64)
    pos = torch.where(live.unsqueeze(-1), pos, pos.new_full((), -1)).reshape(B, maxp * S)
    if qscale is None:
        return qc, vc, pos
    qs, vs = (x.index_select(0, idx).reshape(B, maxp, -1, S).transpose(1, 2).reshape(B, -1, maxp * S) for x in (qscale, vscale))
    return qc, vc, pos, qs, vs


def decode_paged(rows, qpool, vpool, pool_pos, table, npages, pos0, H: int, scale: float, window: int = 0, Hg=None,
                 qscale=None, vscale=None):
    """:func:`decode` per sequence of a ragged batch over a paged cache (:func:`paged_gather`), sequence ``b``'s
    rows at ``pos0[b], pos0[b] + 1, ...``; a sequence with a negative ``pos0`` sees nothing.  ``qscale`` / ``vscale``
    (P, Hg, S): the pool is fp8 and is dequantised in the compute dtype after the gather."""
    qc, vc, pos, *sc = paged_gather(qpool, vpool, pool_pos, table, npages, qscale, vscale)
    if sc:
        cdt, hg = compute_dtype(rows), sc[0].shape[1]
        qc, vc = ((x.to(cdt).reshape(*x.shape[:2], hg, -1) * s.to(cdt).transpose(1, 2).unsqueeze(-1)).reshape(x.shape)
                  for x, s in ((qc, sc[0]), (vc, sc[1])))
    outs = []
    for b, p0 in enumerate(int(p) for p in pos0.tolist()):
        cp = pos[b:b + 1] if p0 >= 0 else torch.full_like(pos[b:b + 1], -1)
        outs.append(decode(rows[b:b + 1], qc[b:b + 1], vc[b:b + 1], cp, max(p0, 0), H, scale, window, Hg))
    return torch.cat([o for o, _ in outs]), torch.cat([l for _, l in outs])


def cache_quant(x, Hg: int):
    """The fp8 cache format, literally: ``x`` (..., 2*Hg*D) 16-bit rows ``[q | v]`` -> (bytes (..., 2*Hg*D)
    ``float8_e4m3fn``, scales (..., 2*Hg) fp32), one scale per chunk of ``D`` features (one head of ``q`` or
    ``v``): ``s = amax * (1 / 448)`` in fp32 (1 for an all-zero chunk), ``bytes = rne(x / s)``.  ``|x / s|``
    stays within ``448 (1 + 2^-23)``, which rounds to 448: nothing saturates."""
    ch = x.float().reshape(*x.shape[:-1], 2 * Hg, -1)
    amax = ch.abs().amax(-1)
    s = torch.where(amax == 0, torch.ones_like(amax), amax * (torch.ones((), dtype=torch.float32, device=x.device) / 448))
    return (ch / s.unsqueeze(-1)).to(torch.float8_e4m3fn).reshape(x.shape), s


def cache_dequant(b8, scales, Hg: int, dtype):
    """``scale * e4m3`` of :func:`cache_quant`'s pair -> (..., 2*Hg*D) in ``dtype`` (the product in fp64 for an
    fp64 ``dtype``, else fp32, rounded once)."""
    cdt = torch.float64 if dtype == torch.float64 else torch.float32
    ch = b8.to(cdt).reshape(*b8.shape[:-1], 2 * Hg, -1) * scales.to(cdt).unsqueeze(-1)
    return ch.reshape(b8.shape).to(dtype)


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
