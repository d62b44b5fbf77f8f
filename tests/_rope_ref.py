"""Dense torch reference of the module with rotary position embedding, written out with plain
torch ops (three ``F.linear``, the explicit rotation, softmax, the output linear): what the
rope tests compare xdot against, so that two xdot runs are not merely equal to each other."""
import math

import torch
import torch.nn.functional as F


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


def dense_attn(params, xk, xq, xv, mask, H, base=10000.0, rope=True):
    """``params``: name -> tensor as the module's ``named_parameters``; ``mask``: bool (B, T, T),
    True = masked, or None.  Positions start at 0 (the whole sequence)."""
    k = F.linear(xk, params["keys.weight"], params.get("keys.bias"))
    q = F.linear(xq, params["queries.weight"], params.get("queries.bias"))
    v = F.linear(xv, params["values.weight"], params.get("values.bias"))
    if rope:
        k, q = rotate(k, H, base), rotate(q, H, base)
    B, T, C = k.shape
    D = C // H
    kh = k.view(B, T, H, D).transpose(1, 2)
    qh = q.view(B, T, H, D).transpose(1, 2)
    vh = v.view(B, T, H, -1).transpose(1, 2)
    s = torch.matmul(kh, qh.transpose(-1, -2)) / math.sqrt(D)
    if mask is not None:
        s = s.masked_fill(mask.view(B, 1, T, T), float("-inf"))
    o = torch.matmul(torch.softmax(s, dim=-1), vh).transpose(1, 2).reshape(B, T, -1)
    return F.linear(o, params["composition.weight"], params.get("composition.bias"))


def dense_run(module, x, mask, rope=True, base=10000.0):
    """Forward and backward (loss = mean of squares) of :func:`dense_attn` in fp64 on copies of
    ``module``'s parameters and of the self-attention input ``x``.  Returns
    ``(out, dx, {name: grad})``, all fp64."""
    params = {n: p.detach().double().clone().requires_grad_(True) for n, p in module.named_parameters()}
    xd = x.detach().double().clone().requires_grad_(True)
    out = dense_attn(params, xd, xd, xd, mask, module.num_heads, base, rope)
    out.pow(2).mean().backward()
    return out.detach(), xd.grad, {n: p.grad for n, p in params.items()}
