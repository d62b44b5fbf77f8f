"""fp64 definition, rounding model and torch emulation of the gated-attention kernels
(``csrc/gate.hip``); the definition and the dense module reference are ``tests/_module_ref.py``'s.

Definition (Qiu et al. 2025): a sigmoid gate on the merged attention output, before the output
projection; ``g`` comes from the row-side input:

    g = x_row W_g^T (+ b_g),   o' = o . sigma(g),   out = composition(o')

``g`` is (B, R, H D) ("elementwise") or (B, R, H) ("headwise": one value per head row, broadcast over
its D features).  The kernels evaluate, with e = exp(-|g|) and r = 1 / (1 + e),

    sigma = g >= 0 ? r : e r,     sigma' = e r^2
    do = do' sigma,   dg = (do' o) sigma'   (headwise: S = sum_j do'_j o_j in a fixed order, dg = S sigma')

tests/test_gate.py (CPU) shows that the emulation of the kernels' order of operations stays inside
the bounds defined here and that six wrong algorithms do not; tests/test_gate_gpu.py holds the kernels
to the same bounds.  As in tests/_sink_ref.py every bound is F (= 2) times a first-order model of the
kernel's roundings (the "unit bound"), the references are fp64 from the values the kernel reads, and
nothing here calls xdot.

The model (u = 2^-24; w = e / (1 + e) = sigma(-|g|); g is read exactly, -|g| is exact):
  e        expf at 1 ulp = 2 u:                               rel(e) <= E_EXP u
  r        1 + e and the reciprocal, one rounding each; d ln r = -w d ln e:
                                                               rel(r) <= (w E_EXP + 2) u
  sigma    g >= 0: r, and w = 1 - sigma.  g < 0: e r, one more product, d ln(e r) = (1 - w) d ln e
           and there sigma = w.  Either way                    rel(sigma) <= ((1 - sigma) E_EXP + 3) u
  o'       one fp32 product and one rounding to the tensor dtype:
               |err o'| <= |o'| (((1 - sigma) E_EXP + 4) u + EPS_OUT) + TINY + |o| 2^-125
           (the last term: below the fp32 normal range e, and with it sigma, is a subnormal or
           flushed: an absolute error of at most 2^-126 in sigma, times |o|)
  do       the same with do' in place of o
  sigma'   e r r: d ln sigma' = (1 - 2 w) d ln e, |1 - 2 w| <= 1; r twice (2 u each) and two products:
                                                               rel(sigma') <= (E_EXP + 6) u
  dg       elementwise, (do' o) sigma': two more products and the rounding to the tensor dtype:
               |err dg| <= |dg| ((E_EXP + 8) u + EPS_OUT) + TINY + |do' o| 2^-125
           headwise, S sigma' with S an ordered sum of products whose longest chain of additions is
           K (:func:`k_dg`): |err S| <= sum_j |do'_j o_j| (1 + K) u, then one product and the rounding:
               |err dg| <= sigma' sum_j |do'_j o_j| (1 + K) u + |dg| ((E_EXP + 7) u + EPS_OUT)
                           + TINY + sum_j |do'_j o_j| 2^-125
g = +inf: e = 0 exactly, sigma = 1 exactly and o' = o bit for bit; g = -inf: sigma = 0 and o' = +-0.

Not collected as a test (no ``test_`` prefix).
"""
import math

import torch
import torch.nn.functional as Fn

from _sink_ref import BF16, DT_IDS, EPS_OUT, F, F32, F64, FP16, NINF, TINY, U32, E_EXP, _abs_err, check, ratio  # noqa: F401
from _module_ref import dense_attn, dense_run, gate  # noqa: F401  (the definition)

SUB = 2.0 ** -125   # absolute error of a value below the fp32 normal range (see the docstring)
INF = float("inf")
PLANTED_G = (0.0, 30.0, -30.0, 100.0, -100.0, INF, -INF)


def rank_run(module, x_local, peers_qv, rank, mask_rows):
    """One rank's step by the definition, in fp64: the rank's rows ``x_local`` (B, R, C) against the
    gathered side of the whole sequence -- this rank's own ``q`` / ``v`` block projected here (and
    differentiated through), the other ranks' blocks taken as the constants ``peers_qv`` (B, T, 2 C')
    (the stored values a real gather would deliver) -- under ``mask_rows`` bool (B, R, T), loss = mean of
    squares of the rank's output.  The gathered side's gradient is the rank's own block of its own
    ``d[q|v]`` (what an emulated reduce-scatter hands back).  No norm, rope or sinks.
    -> ``(out, dx, {name: grad})``."""
    params = {n: p.detach().double().clone().requires_grad_(True) for n, p in module.named_parameters()}
    H, Hg = module.num_heads, module.num_gathered_heads
    xd = x_local.detach().double().clone().requires_grad_(True)
    R = xd.shape[1]
    k = Fn.linear(xd, params["keys.weight"], params.get("keys.bias"))
    q = Fn.linear(xd, params["queries.weight"], params.get("queries.bias"))
    v = Fn.linear(xd, params["values.weight"], params.get("values.bias"))
    nq = q.shape[-1]
    pq = peers_qv.detach().double()
    lo, hi = rank * R, (rank + 1) * R
    qf = torch.cat([pq[:, :lo, :nq], q, pq[:, hi:, :nq]], dim=1)
    vf = torch.cat([pq[:, :lo, nq:], v, pq[:, hi:, nq:]], dim=1)
    B, T = qf.shape[0], qf.shape[1]
    D = k.shape[-1] // H
    kh = k.view(B, R, H, D).transpose(1, 2)
    qh = qf.view(B, T, Hg, D).transpose(1, 2).repeat_interleave(H // Hg, dim=1)
    vh = vf.view(B, T, Hg, -1).transpose(1, 2).repeat_interleave(H // Hg, dim=1)
    s = torch.matmul(kh, qh.transpose(-1, -2)) * (1.0 / math.sqrt(D))
    s = s.masked_fill_(mask_rows.view(B, 1, R, T), NINF)
    o = torch.matmul(torch.softmax(s, dim=-1), vh).transpose(1, 2).reshape(B, R, -1)
    if "gate.weight" in params:
        o = gate(o, Fn.linear(xd, params["gate.weight"], params.get("gate.bias")), H)
    out = Fn.linear(o, params["composition.weight"], params.get("composition.bias"))
    out.pow(2).mean().backward()
    return out.detach(), xd.grad, {n: p.grad for n, p in params.items()}


# ---- fp64 references of the two kernels and their unit bounds ---------------------------------------------
def _parts64(g):
    g = g.detach().double().cpu()
    e = torch.exp(-g.abs())
    r = 1.0 / (1.0 + e)
    return torch.where(g >= 0, r, e * r), e * r * r


def _bc(t, B, R, H, D, headwise):
    """A per-gate-value tensor broadcast to (B, R, H, D)."""
    return t.unsqueeze(-1).expand(B, R, H, D) if headwise else t.reshape(B, R, H, D)


def vec_width(D, dtype):
    """Elements per lane step of the kernels on contiguous, aligned tensors: 16 bytes where D is a
    multiple of that many elements, one element otherwise."""
    V = 16 // torch.empty((), dtype=dtype).element_size()
    return V if D % V == 0 else 1


def k_dg(D, dtype):
    """The longest chain of additions of the headwise sum: V per lane step, ceil(nch / L) steps per
    lane, then the halving tree over the L lanes of the head row."""
    V = vec_width(D, dtype)
    nch = D // V
    L = min(nch, 64)
    return V * (-(-nch // L)) + max(0, math.ceil(math.log2(L)))


def _clean(b):
    """A NaN bound (a NaN operand: NaN is expected there, and checked as such) -> 1."""
    return torch.nan_to_num(b, nan=1.0, posinf=1e300)


def ref_apply(o, g, H, dtype):
    """-> (o' fp64, its unit bound) from the stored values."""
    B, R, C = o.shape
    D = C // H
    hw = g.shape[-1] != C
    o64 = o.detach().double().cpu().reshape(B, R, H, D)
    sig, _ = _parts64(g)
    s = _bc(sig, B, R, H, D, hw)
    y = o64 * s
    b = y.abs() * (((1 - s) * E_EXP + 4) * U32 + EPS_OUT[dtype]) + TINY[dtype] + o64.abs() * SUB
    return y.reshape(B, R, C), _clean(b).reshape(B, R, C)


def ref_backward(dy, o, g, H, dtype, K=None):
    """-> (do, dg in fp64, their unit bounds) from the stored values.  ``K``: the longest chain of the
    headwise sum (default: the kernels', :func:`k_dg`; D covers a sum in any order)."""
    B, R, C = o.shape
    D = C // H
    hw = g.shape[-1] != C
    d64 = dy.detach().double().cpu().reshape(B, R, H, D)
    o64 = o.detach().double().cpu().reshape(B, R, H, D)
    sig, sp = _parts64(g)
    s = _bc(sig, B, R, H, D, hw)
    do = d64 * s
    bdo = do.abs() * (((1 - s) * E_EXP + 4) * U32 + EPS_OUT[dtype]) + TINY[dtype] + d64.abs() * SUB
    t = d64 * o64
    if hw:
        S, A = t.sum(-1), t.abs().sum(-1)
        dg = S * sp
        bdg = sp * A * (1 + (k_dg(D, dtype) if K is None else K)) * U32 + dg.abs() * ((E_EXP + 7) * U32 + EPS_OUT[dtype]) + TINY[dtype] + A * SUB
    else:
        dg = (t * sp.reshape(B, R, H, D)).reshape(B, R, C)
        bdg = dg.abs() * ((E_EXP + 8) * U32 + EPS_OUT[dtype]) + TINY[dtype] + t.abs().reshape(B, R, C) * SUB
    return do.reshape(B, R, C), dg, _clean(bdo).reshape(B, R, C), _clean(bdg)


# ---- emulation: the kernels' order of operations in fp32 torch ---------------------------------------------
def _parts32(g, bug=None):
    g = g.detach().cpu().float()
    e = torch.exp(-g.abs())
    r = 1.0 / (1.0 + e)
    sig = torch.where(g >= 0, r, e * r)
    if bug == "one_minus":      # sigma(g) for g < 0 as 1.f - sigma(-g): cancels for large |g|
        sig = torch.where(g >= 0, r, 1.0 - r)
    sp = e * r * r
    if bug == "sigma_minus_sq":  # sigma - sigma^2: cancels for large g
        sp = sig - sig * sig
    return sig, sp


def _wrong_heads(g, H):
    """``g`` (B, R, H) read with the wrong head stride: head h takes the value of head (2 h) mod H."""
    return g[..., (2 * torch.arange(H)) % H]


def emulate_apply(o, g, H, bug=None):
    """``gate_apply`` in fp32 torch on the CPU -> o' in o's dtype.  ``bug``: 'one_minus', 'head_stride'."""
    B, R, C = o.shape
    D = C // H
    hw = g.shape[-1] != C
    if bug == "head_stride" and hw:
        g = _wrong_heads(g, H)
    sig, _ = _parts32(g, bug)
    y = o.detach().cpu().float().reshape(B, R, H, D) * _bc(sig, B, R, H, D, hw)
    return y.to(o.dtype).reshape(B, R, C)


def _ordered_head_sum(t, dtype, bug=None):
    """(B, R, H, D) fp32 products -> (B, R, H) in the kernels' order: lane li of the head row's
    L = min(nch, 64) lanes adds the V elements of steps li, li + L, ... one by one, then lanes
    [half, w) are added onto lanes [0, w - half), w -> half = ceil(w / 2), down to lane 0."""
    B, R, H, D = t.shape
    V = vec_width(D, dtype)
    nch = D // V
    L = min(nch, 64)
    steps = -(-nch // L)
    pad = steps * L * V - D
    tp = torch.cat([t, torch.zeros(B, R, H, pad)], dim=-1).reshape(B, R, H, steps, L, V)
    if bug == "last_chunk":  # the last lane step of the head row is left out
        tp = tp.clone()
        tp.view(B, R, H, steps * L, V)[..., nch - 1, :] = 0
    acc = torch.zeros(B, R, H, L)
    for s in range(steps):
        for k in range(V):
            acc = acc + tp[..., s, :, k]
            if bug == "sum16":  # the accumulator kept in the tensor dtype
                acc = acc.to(dtype).float()
    w = L
    while w > 1:
        half = (w + 1) // 2
        acc = acc.clone()
        acc[..., :w - half] = acc[..., :w - half] + acc[..., half:w]
        if bug == "sum16":
            acc = acc.to(dtype).float()
        w = half
    return acc[..., 0]


def emulate_backward(dy, o, g, H, bug=None):
    """``gate_backward`` in fp32 torch on the CPU -> (do, dg) in o's dtype.  ``bug``: 'sigma_minus_sq',
    'one_minus', 'ungated' (do = do'), 'sum16', 'last_chunk', 'head_stride'."""
    B, R, C = o.shape
    D = C // H
    hw = g.shape[-1] != C
    if bug == "head_stride" and hw:
        g = _wrong_heads(g, H)
    sig, sp = _parts32(g, bug)
    d = dy.detach().cpu().float().reshape(B, R, H, D)
    of = o.detach().cpu().float().reshape(B, R, H, D)
    do = d if bug == "ungated" else d * _bc(sig, B, R, H, D, hw)
    if hw:
        dg = _ordered_head_sum(d * of, o.dtype, bug) * sp
    else:
        dg = ((d * of) * sp.reshape(B, R, H, D)).reshape(B, R, C)
    return do.to(o.dtype).reshape(B, R, C), dg.to(o.dtype)


# ---- inputs -----------------------------------------------------------------------------------------------
def gate_inputs(B, R, H, D, dtype, headwise, seed=0, plant=True):
    """(o, g, do'): normal draws; with ``plant`` g holds 0, +-30, +-100 and +-inf (where it has at
    least seven values), o holds zeros and
    1e4 (one of them under a planted g), and (R > 2) one row of o is NaN."""
    gen = torch.Generator().manual_seed(seed)
    C = H * D
    o = torch.randn(B, R, C, generator=gen)
    g = 2.0 * torch.randn(B, R, H if headwise else C, generator=gen)
    dy = torch.randn(B, R, C, generator=gen)
    if plant:
        gf, of = g.view(-1), o.view(-1)
        n, m = gf.numel(), of.numel()
        if n >= len(PLANTED_G):  # (fewer gate values than planted ones: the draws stay)
            for i, val in enumerate(PLANTED_G):
                gf[(i * 5 + 1) % n] = val
        of[(3 * 7 + 2) % m] = 0.0
        of[(m // 2 + 1) % m] = 0.0
        of[(5 + 1) % m] = 1e4     # (elementwise: the feature under g = 30)
        of[(m // 3) % m] = 1e4
        if R > 2:
            o[-1, R // 2] = float("nan")
    return o.to(dtype), g.to(dtype), dy.to(dtype)
