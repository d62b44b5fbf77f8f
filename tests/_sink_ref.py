"""fp64 definition, rounding model and torch emulation of the attention-sink kernels
(``csrc/sink.hip``); the definition and the dense module reference are ``tests/_module_ref.py``'s.

Definition: one logit ``s_h`` per row head is appended to every row's masked, scaled scores -- it is
not scaled itself -- takes part in the softmax and contributes no value:

    P = softmax(cat([S, s_h], -1))[..., :T],   O = P V

Fold identities (the kernels; ``(o, lse)`` is the finished plain attention of the same row):

    x = lse - s_h,  lse' = logaddexp(lse, s_h) = max(lse, s_h) + log1p(exp(-|x|))
    g = exp(lse - lse') = sigmoid(x),  o' = g o      (lse = -inf: o' = 0 selected, lse' = s_h)
    ds_h = -sum_{b, r} exp(s_h - lse'[b, h, r]) delta'[b, h, r],  delta' = rowsum(dO . o')

tests/test_sinks.py (CPU) shows that the emulation of the kernels' order of operations stays inside
the bounds defined here and that six wrong algorithms do not; tests/test_sinks_gpu.py holds the
kernels to the same bounds.  As in tests/_elementwise.py and tests/_headnorm_ref.py every bound is
F (= 2) times a first-order model of the kernel's roundings (the "unit bound"), the references are
fp64 from the values the kernel reads, and nothing here calls xdot.

The model (u = 2^-24; e = exp(-|x|); w = e / (1 + e) = sigmoid(-|x|)):
  x            one fp32 subtraction: |dx| <= u |x|
  e            exp of the rounded x, the intrinsic at 1 ulp = 2 u:  rel(e) <= (|x| + E_EXP) u
  g            1 + e, the reciprocal, and for x < 0 the product e r: 3 u of its own.  g = 1 / (1 + e)
               or e / (1 + e) carries rel(e) times (1 - g) either way:
                   rel(g) <= ((1 - g)(|x| + E_EXP) + 3) u
  o'           one fp32 product and one rounding to the tensor dtype:
                   |err o'| <= |o'| (((1 - g)(|x| + E_EXP) + 4) u + EPS_OUT) + TINY
  lse'         log1p at 2 ulp = 4 u of its value, d log1p(e) = w rel(e), one fp32 addition:
                   |err lse'| <= (w (|x| + E_EXP) + E_LOG1P log1p(e) + |lse'|) u + TINY
               (lse = -inf: e = 0 exactly and lse' = s_h bit for bit; TINY keeps 0 <= 0 true)
  ds           term_i = exp(s - lse'_i) delta_i: subtraction, exp, product -> (|s - lse'_i| + E_EXP + 1) u,
               and an ordered sum whose longest chain is K (:func:`k_ds`):
                   |err ds| <= sum_i |term_i| (|s - lse'_i| + E_EXP + 1 + K) u + TINY
The module's ``sinks.grad`` in bf16 has its own unit bound, 4 * 2^-9 * E_h, with E_h = sum_{b, r}
p_sink sum_d |dO_d o'_d| from the fp64 run (two output roundings, P rounded once for P V, and lse).

Not collected as a test (no ``test_`` prefix).
"""
import math

import torch
import torch.nn.functional as Fn

from _module_ref import NINF, attend, definition, dense_attn, dense_run  # noqa: F401  (the definition)

F32, BF16, FP16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
DT_IDS = {F32: "fp32", BF16: "bf16", FP16: "fp16"}
F = 2.0
U32 = 2.0 ** -24
EPS_OUT = {F32: 0.0, BF16: 2.0 ** -9, FP16: 2.0 ** -11, F64: 0.0}
# the absolute rounding error below the normal range (fp32 intermediates flush near 2^-126; fp16
# outputs go subnormal below 2^-14, where one rounding is 2^-25)
TINY = {F32: 2.0 ** -125, BF16: 2.0 ** -125, FP16: 2.0 ** -24, F64: 0.0}
E_EXP = 2.0      # expf: 1 ulp
E_LOG1P = 4.0    # log1pf: 2 ulp
CHUNK = 1024     # (b, r) elements of one head per workgroup of the ds kernel: 4 per thread, 256 threads


def sink_scale(k, q, v, mask, H, scale, sinks, dout, Hg=None):
    """E_h (H,) = sum_{b, r} p_sink sum_d |dO_d o'_d| of one attention call, in fp64 from the stored
    operands: the scale of the ``ds`` bounds of the functions and of the module."""
    k, q, v, sinks, dout = (t.detach().double() for t in (k, q, v, sinks, dout))
    Hg = Hg or H
    B, R, C = k.shape
    T = q.shape[1]
    o = definition(k, q, v, mask, H, scale, sinks, Hg)
    kh = k.view(B, R, H, -1).transpose(1, 2)
    qh = q.view(B, T, Hg, -1).transpose(1, 2).repeat_interleave(H // Hg, dim=1)
    s = torch.matmul(kh, qh.transpose(-1, -2)) * scale
    if mask is not None:
        s = s.masked_fill(mask.view(B, 1, R, T), NINF)
    sk = sinks.view(1, H, 1)
    psink = torch.exp(sk - torch.logaddexp(torch.logsumexp(s, dim=-1), sk))          # (B, H, R)
    absdot = (dout * o).abs().view(B, R, H, -1).sum(-1).transpose(1, 2)              # (B, H, R)
    return (psink * absdot).sum(dim=(0, 2))


def sink_grad_scale(module, x, mask):
    """E_h (H,) of the module's ``sinks.grad`` bound, from the fp64 run of :func:`dense_attn` with the
    loss of :func:`dense_run`: ``sum_{b, r} p_sink sum_d |dO_d o'_d|`` with ``o'`` the attention's
    output (before the composition) and ``dO`` the loss's gradient w.r.t. it."""
    p = {n: t.detach().double() for n, t in module.named_parameters()}
    H, Hg = module.num_heads, module.num_gathered_heads
    xd = x.detach().double()
    k = Fn.linear(xd, p["keys.weight"], p.get("keys.bias"))
    q = Fn.linear(xd, p["queries.weight"], p.get("queries.bias"))
    v = Fn.linear(xd, p["values.weight"], p.get("values.bias"))
    B, T, C = k.shape
    D = C // H
    o = definition(k, q, v, mask, H, 1.0 / math.sqrt(D), p["sinks"], Hg).requires_grad_(True)
    out = Fn.linear(o, p["composition.weight"], p.get("composition.bias"))
    out.pow(2).mean().backward()
    return sink_scale(k, q, v, mask, H, 1.0 / math.sqrt(D), p["sinks"], o.grad, Hg)


# ---- fp64 references of the two kernels ---------------------------------------------------------------------
def ref_fold(out, lse, sinks, H):
    """-> (o', lse', g, x) in fp64 on the CPU from the stored values: out (B, R, H D), lse (B, H, R),
    sinks (H,).  Rows with lse = -inf: o' = 0, lse' = s_h.  s_h = -inf: the inputs themselves."""
    B, R, C = out.shape
    o = out.detach().double().cpu().reshape(B, R, H, C // H)
    l = lse.detach().double().cpu()
    s = sinks.detach().double().cpu().view(1, H, 1).expand_as(l)
    off = s == NINF
    x = l - s
    l2 = torch.where(off, l, torch.logaddexp(l, s))
    g = torch.where(off, torch.ones_like(l), torch.sigmoid(x))
    gate = g.transpose(1, 2).unsqueeze(-1)
    dead = ((l == NINF) & ~off).transpose(1, 2).unsqueeze(-1)
    o2 = torch.where(dead.expand_as(o), torch.zeros_like(o), torch.where(off.transpose(1, 2).unsqueeze(-1), o, o * gate))
    return o2.reshape(B, R, C), l2, g, x


def fold_bounds(o2, l2, g, x, dtype):
    """Unit bounds (per element) of o' (B, R, H D) and lse' (B, H, R) from :func:`ref_fold`'s outputs;
    0 where the sink is -inf (nothing may change there)."""
    B, R, C = o2.shape
    H = l2.shape[1]
    ax = x.abs()
    ax = torch.where(torch.isfinite(ax), ax, torch.zeros_like(ax))  # lse = -inf: e = 0 exactly, no |x| term
    e = torch.exp(-x.abs())
    e = torch.where(torch.isnan(e), torch.zeros_like(e), e)
    w = e / (1 + e)
    rel_o = ((1 - g) * (ax + E_EXP) + 4) * U32 + EPS_OUT[dtype]
    bo = o2.abs().reshape(B, R, H, -1) * rel_o.transpose(1, 2).unsqueeze(-1) + TINY[dtype]
    live = torch.isfinite(l2)
    bl = torch.where(live, (w * (ax + E_EXP) + E_LOG1P * torch.log1p(e) + l2.abs()) * U32 + TINY[F32],
                     torch.zeros_like(l2))
    off = x == float("inf")  # s = -inf with a live row; a dead row with s = -inf has x = NaN
    off = off | torch.isnan(x)
    bo = torch.where(off.transpose(1, 2).unsqueeze(-1).expand_as(bo), torch.zeros_like(bo), bo)
    bl = torch.where(off, torch.zeros_like(bl), bl)
    return bo.reshape(B, R, C), bl


def ref_grad(delta, lse, sinks):
    """-> (ds (H,), unit-bound scale parts) in fp64: the terms and ``|s - lse'|`` per element."""
    d = delta.detach().double().cpu()
    l = lse.detach().double().cpu()
    s = sinks.detach().double().cpu().view(1, -1, 1).expand_as(l)
    off = s == NINF
    gap = torch.where(off, torch.zeros_like(l), (s - l).abs())
    term = torch.where(off, torch.zeros_like(l), torch.exp(s - l) * d)
    return -term.sum(dim=(0, 2)), term, gap


def k_ds(B, R):
    """The longest chain of additions of the ordered sum: 4 elements per thread, 6 butterfly levels
    and 3 wave sums per workgroup, twice (the partials: ceil(nparts / 256) per thread)."""
    nparts = max(1, -(-(B * R) // CHUNK))
    return (4 + 6 + 3) + (-(-nparts // 256) + 6 + 3)


def grad_bound(term, gap, B, R):
    """Unit bound (H,) of ds."""
    return (term.abs() * (gap + E_EXP + 1 + k_ds(B, R))).sum(dim=(0, 2)) * U32 + TINY[F32]


def _abs_err(got, want):
    """|got - want| in fp64; a NaN on one side only is an infinite error, NaN on both (a fully masked
    row of a head without a sink, left as it was) none."""
    g = got.detach().double().cpu()
    err = (g - want).abs()
    err = torch.where((torch.isnan(g) & torch.isnan(want)) | (g == want), torch.zeros_like(err), err)  # (-inf == -inf)
    return torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)


def check(name, got, want, bound, factor=F):
    """Print the largest error in units of the unit bound (the RATIO line) and assert it is <= F;
    where the bound is 0 the values must be equal."""
    err = _abs_err(got, want)
    if got.numel() == 0:
        return 0.0
    zero = bound == 0
    exact = bool((err[zero] == 0).all()) if bool(zero.any()) else True
    ratio = (err[~zero] / bound[~zero]).max().item() if bool((~zero).any()) else 0.0
    print(f"RATIO {name}: {ratio:.3f} of the unit bound (allowed {factor:g}){'' if exact else '  [inexact where exact is due]'}")
    assert exact, name
    assert ratio <= factor, (name, ratio)
    return ratio


def ratio(got, want, bound):
    """The largest error in units of the unit bound (inf for a NaN or a miss where the bound is 0)."""
    err = _abs_err(got, want)
    r = torch.where(bound == 0, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))),
                    err / bound.clamp_min(1e-300))
    return r.max().item()


# ---- emulation: the kernels' order of operations in fp32 torch -----------------------------------------
def emulate_fold(out, lse, sinks, H, bug=None, scale=1.0):
    """``sink_fold`` of csrc/sink.hip in fp32 torch on the CPU -> (o' in out's dtype, lse' fp32).
    ``bug``: 'scaled_sink' (the logit times ``scale``), 'lse_kept' (lse not updated), 'multiplied'
    (fully masked rows multiplied by g = 0 instead of selected)."""
    B, R, C = out.shape
    o = out.detach().cpu().float().reshape(B, R, H, C // H)
    l = lse.detach().cpu().float()
    s = sinks.detach().cpu().float()
    if bug == "scaled_sink":
        s = s * torch.tensor(scale, dtype=F32)
    s = s.view(1, H, 1).expand_as(l)
    x = l - s
    e = torch.exp(-x.abs())
    r = 1.0 / (1.0 + e)
    g = torch.where(x >= 0, r, e * r)
    l2 = torch.maximum(l, s) + torch.log1p(e)
    off = s == NINF
    gate = g.transpose(1, 2).unsqueeze(-1)
    o2 = (o * gate).to(out.dtype)
    if bug != "multiplied":
        dead = (l == NINF).transpose(1, 2).unsqueeze(-1).expand_as(o2)
        o2 = torch.where(dead, torch.zeros_like(o2), o2)
    o2 = torch.where(off.transpose(1, 2).unsqueeze(-1).expand_as(o2), out.detach().cpu().reshape(B, R, H, -1), o2)
    l2 = torch.where(off, l, l2)
    if bug == "lse_kept":
        l2 = l.clone()
    return o2.reshape(B, R, C), l2


def _block_sum(v):
    """256 fp32 values -> their sum in the kernels' order: the xor butterfly within each wave of 64,
    then the four waves in order."""
    w = v.reshape(4, 64).clone()
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, torch.arange(64) ^ o]
    return ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]


def emulate_grad(delta, lse, sinks, bug=None):
    """``sink_grad`` in fp32 torch in the kernels' order -> ds (H,) fp32.  ``bug``: 'sign', 'all_heads'
    (every head gets the sum over heads)."""
    d = delta.detach().cpu().float()
    l = lse.detach().cpu().float()
    s = sinks.detach().cpu().float()
    B, H, R = l.shape
    n = B * R
    nparts = max(1, -(-n // CHUNK))
    ds = torch.zeros(H, dtype=F32)
    for h in range(H):
        if s[h] == NINF:
            continue
        term = torch.exp(s[h] - l[:, h].reshape(-1)) * d[:, h].reshape(-1)
        term = torch.cat([term, torch.zeros(nparts * CHUNK - n, dtype=F32)]).reshape(nparts, 4, 256)
        parts = []
        for c in range(nparts):
            acc = torch.zeros(256, dtype=F32)
            for k in range(4):
                acc = acc + term[c, k]
            parts.append(_block_sum(acc))
        parts = torch.stack(parts)
        pad = torch.cat([parts, torch.zeros(-(-nparts // 256) * 256 - nparts, dtype=F32)]).reshape(-1, 256)
        acc = torch.zeros(256, dtype=F32)
        for j in range(pad.shape[0]):
            acc = acc + pad[j]
        ds[h] = -_block_sum(acc)
    if bug == "sign":
        ds = -ds
    if bug == "all_heads":
        ds = ds.sum().expand(H).clone()
    return ds


def delta64(dout, o, H):
    """rowsum(dO . o) per head in fp64: (B, H, R)."""
    B, R, C = o.shape
    return (dout.detach().double().cpu() * o.detach().double().cpu()).reshape(B, R, H, -1).sum(-1).transpose(1, 2)


def fold_inputs(B, R, H, D, dtype, seed=0, gap=6.0, dead_rows=True, sink_dtype=F32):
    """Inputs of a fold as a forward leaves them: out with entries of order 1, lse of order log T,
    sinks within ``gap`` of it in both signs; with ``dead_rows`` some rows have lse = -inf and NaN
    in out, and (H > 1) the last head's sink is -inf."""
    gen = torch.Generator().manual_seed(seed)
    out = torch.randn(B, R, H * D, generator=gen).to(dtype)
    lse = 5.0 + torch.randn(B, H, R, generator=gen)
    sinks = (5.0 + gap * (2 * torch.rand(H, generator=gen) - 1)).to(sink_dtype)
    if dead_rows and R > 2:
        lse[:, :, R // 2] = NINF
        ov = out.view(B, R, H, D)
        ov[:, R // 2] = float("nan")
        if H > 1:
            sinks[-1] = NINF
    return out, lse, sinks
