"""The module by its definition, in plain torch ops and the inputs' dtype (the tests run it in fp64):
three ``F.linear``, the per-head RMSNorm (QK-norm), the explicit rotation (rope), the dense softmax
with the sink logit as one more column, the sigmoid gate, the output linear.  What the rope, QK-norm,
sink and gate tests compare xdot against, so that two xdot runs are not merely equal to each other;
nothing here calls xdot.

Not collected as a test (no ``test_`` prefix).
"""
import math

import torch
import torch.nn.functional as Fn

NINF = -float("inf")


def rotate(x, H, base=10000.0, offset=0):
    """Half-split rotation of ``x`` (B, T, H*D) at positions ``offset + t``, in ``x``'s dtype
    (angles in fp64)."""
    B, T, C = x.shape
    D = C // H
    h = D // 2
    pos = torch.arange(offset, offset + T, dtype=torch.float64, device=x.device)
    inv = torch.tensor([base ** (-2.0 * i / D) for i in range(h)], dtype=torch.float64, device=x.device)
    ang = pos.view(T, 1) * inv.view(1, h)
    c = torch.cos(ang).to(x.dtype).view(1, T, 1, h)
    s = torch.sin(ang).to(x.dtype).view(1, T, 1, h)
    xv = x.reshape(B, T, H, D)
    x1, x2 = xv[..., :h], xv[..., h:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).reshape(B, T, C)


def head_norm(x, H, w, eps):
    """Per-head RMSNorm of ``x`` (B, T, H*D) with the (D,) gain ``w``, in ``x``'s dtype."""
    B, T, C = x.shape
    xv = x.reshape(B, T, H, C // H)
    return (xv * torch.rsqrt(xv.pow(2).mean(-1, keepdim=True) + eps) * w).reshape(B, T, C)


def attend(scores, sinks, v):
    """``softmax(cat([scores, s], -1))[..., :T] @ v`` for scores (B, H, R, T) (masked: -inf), sinks
    (H,), v (B, H, T, d); ``sinks=None``: the plain softmax."""
    if sinks is None:
        return torch.matmul(torch.softmax(scores, dim=-1), v)
    B, H, R, T = scores.shape
    col = sinks.view(1, H, 1, 1).expand(B, H, R, 1)
    return torch.matmul(torch.softmax(torch.cat([scores, col], dim=-1), dim=-1)[..., :T], v)


def definition(k, q, v, mask, H, scale, sinks=None, Hg=None):
    """Attention (with sinks) by the definition on head-interleaved k (B, R, H D), q / v (B, T, Hg D),
    mask bool (B, R, T) or None -> (B, R, H Dv); differentiable, in the inputs' dtype."""
    Hg = Hg or H
    B, R, C = k.shape
    T = q.shape[1]
    kh = k.view(B, R, H, -1).transpose(1, 2)
    qh = q.view(B, T, Hg, -1).transpose(1, 2).repeat_interleave(H // Hg, dim=1)
    vh = v.view(B, T, Hg, -1).transpose(1, 2).repeat_interleave(H // Hg, dim=1)
    s = torch.matmul(kh, qh.transpose(-1, -2)) * scale
    if mask is not None:
        s = s.masked_fill(mask.view(B, 1, R, T), NINF)
    return attend(s, sinks, vh).transpose(1, 2).reshape(B, R, -1)


def gate(o, g, H):
    """``o . sigmoid(g)`` for o (B, R, H D) and g (B, R, H D) or (B, R, H); differentiable."""
    B, R, C = o.shape
    s = torch.sigmoid(g)
    if g.shape[-1] == C:
        return o * s
    return (o.reshape(B, R, H, C // H) * s.unsqueeze(-1)).reshape(B, R, C)


def dense_attn(params, xk, xq, xv, mask, H, Hg=None, *, rope=False, base=10000.0, eps=1e-6):
    """``params``: name -> tensor as the module's ``named_parameters``; the features are the names
    present: QK-norm with ``keys_norm.weight`` / ``queries_norm.weight`` (``eps``), sinks with
    ``sinks``, the gate -- from the ROW-side input ``xk`` -- with ``gate.weight``; ``rope``: k and q
    rotated at positions 0..T-1 (the whole sequence).  ``mask``: bool (B, T, T), True = masked, or
    None; ``Hg``: the gathered heads of q / v (default ``H``)."""
    Hg = Hg or H
    k = Fn.linear(xk, params["keys.weight"], params.get("keys.bias"))
    q = Fn.linear(xq, params["queries.weight"], params.get("queries.bias"))
    v = Fn.linear(xv, params["values.weight"], params.get("values.bias"))
    if "keys_norm.weight" in params:
        k = head_norm(k, H, params["keys_norm.weight"], eps)
        q = head_norm(q, Hg, params["queries_norm.weight"], eps)
    if rope:
        k, q = rotate(k, H, base), rotate(q, Hg, base)
    o = definition(k, q, v, mask, H, 1.0 / math.sqrt(k.shape[-1] // H), params.get("sinks"), Hg)
    if "gate.weight" in params:
        o = gate(o, Fn.linear(xk, params["gate.weight"], params.get("gate.bias")), H)
    return Fn.linear(o, params["composition.weight"], params.get("composition.bias"))


def dense_run(module, x, mask, rope=None, base=None):
    """Forward and backward (loss = mean of squares) of :func:`dense_attn` in fp64 on copies of
    ``module``'s parameters and of the self-attention input ``x`` -> ``(out, dx, {name: grad})``, all
    fp64.  ``rope`` / ``base``: default the module's own (``module.rope``)."""
    params = {n: p.detach().double().clone().requires_grad_(True) for n, p in module.named_parameters()}
    xd = x.detach().double().clone().requires_grad_(True)
    rot = module.rope
    out = dense_attn(params, xd, xd, xd, mask, module.num_heads, module.num_gathered_heads,
                     rope=rot is not None if rope is None else rope,
                     base=(rot.base if rot is not None else 10000.0) if base is None else base,
                     eps=module.qk_norm_eps)
    out.pow(2).mean().backward()
    return out.detach(), xd.grad, {n: p.grad for n, p in params.items()}
