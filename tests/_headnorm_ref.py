"""fp64 references, a rounding model and a torch emulation of the per-head RMSNorm kernels
(``csrc/headnorm.hip``); the dense module reference is ``tests/_module_ref.py``'s.

    r = rsqrt(mean_j x[j]^2 + eps),  y = x r w,  out = alpha rotate(y)
    gy = alpha rotate^-1(g),  xh = x r,  gw = gy w,  dx = r (gw - xh mean(gw xh)),  dw = sum gy xh

tests/test_headnorm.py (CPU) shows that the emulation of the kernels' algorithm stays inside the
bounds defined here and that five wrong algorithms do not; tests/test_headnorm_gpu.py holds the
kernels to the same bounds.  As in tests/_elementwise.py every bound is F (= 2) times a first-order
model of the kernel's roundings, the references are computed in fp64 from the values the kernel
reads (tensors as stored, ``eps`` / ``alpha`` rounded to fp32), and nothing here calls xdot.

The model (u = 2^-24, half an ulp of 1 in fp32; V = 16 bytes of elements; G lanes per head row):
  sum of squares   non-negative terms, one rounding per fma (the emulation's unfused product: one
                   more), a chain of 2 V + 1 adds in the lane and log2 G butterfly levels:
                   relative error K_SS u,  K_SS = 2 V + 2 + log2 G
  mean + eps       1 / D rounded, one fma: 2 u
  rsqrt            half the argument's error, and 2 u of its own (v_rsq_f32: 1 ulp)
                   E_R = K_SS / 2 + 3            (in units of u)
  y = (x r) w      2 u; without a table w is first multiplied by alpha: 1 u when alpha != 1
  rotation         cos alpha / sin alpha: the table's 2^-24 plus one product each, against the pair
                   norm sqrt 2 (2 u); the product and the fma 2 u;  E_ROT = 2 sqrt 2 + 2
  output           one rounding to the tensor's dtype: EPS_OUT
so that per element
  forward, no table:  |err| <= F |out_ref| ((E_R + 2 + [alpha != 1]) u + EPS_OUT)
  forward, table:     |err| <= F |alpha| hypot(y1, y2) ((E_R + 2 + E_ROT) u + EPS_OUT)
The backward's gy carries E_GY = [alpha != 1] (no table) or E_ROT (table), the latter relative to
the pair norm |alpha| hypot(g1, g2): under a rotation that norm stands in for |gy| in every scale
below (g1 c + g2 s can cancel to nothing while its error cannot), exactly as it does in the
forward's bound; without a table the scales are the plain |gy|.  With |gy|' that stand-in,
gw' = |gy|' |w| and K_P = K_SS the chain of the dot product:
  dx   |err| <= F (S_i (E_GY + 3 E_R + K_P + 7) u + EPS_OUT |dx_ref|),
       S_i = r (gw'_i + |xh_i| mean_j(gw'_j |xh_j|))
  dw   |err| <= F (sum |gy|' |xh| (E_GY + E_R + 2 + K_DW) u + EPS_OUT[weight dtype] |dw_ref|),
       K_DW = the longest chain of the ordered sum: a lane's head rows, the lane groups of a
       workgroup, ceil(partials / 32) partials per strided chain, 32 chains.

Not collected as a test (no ``test_`` prefix).
"""
import math

import torch

from _module_ref import dense_attn, dense_run, head_norm  # noqa: F401  (the dense module reference)

F32, BF16, FP16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
DT_IDS = {F32: "fp32", BF16: "bf16", FP16: "fp16"}
F = 2.0
U32 = 2.0 ** -24
EPS_OUT = {F32: 0.0, BF16: 2.0 ** -9, FP16: 2.0 ** -11, F64: 0.0}
# the absolute rounding error below the normal range of the output dtype
TINY = {F32: 2.0 ** -125, BF16: 2.0 ** -125, FP16: 2.0 ** -24, F64: 0.0}
E_ROT = 2.0 * math.sqrt(2.0) + 2.0


def f32(v: float) -> float:
    """``v`` rounded to fp32: what a ``float`` field of the launch struct holds."""
    return torch.tensor(float(v), dtype=torch.float32).item()


# ---- launch geometry (xdot_headnorm_plan, csrc/headnorm.hip) -------------------------------------------
def plan(B, R, H, D, esize):
    """-> dict(V, G, rows_per_wg, fwd=(gx, gy), bwd=(gx, gy), nparts): the Python mirror of the
    kernels' plan (tests/test_headnorm_gpu.py compares it with ``torch.ops.xdot.headnorm_plan``)."""
    V = 16 // esize
    nchunk = 1 if D // 2 < V else -(-(D // 2) // V)
    G = 1
    while G < nchunk:
        G *= 2
    assert G <= 64
    rpw = 256 // G
    nbh, nrg = B * H, -(-R // rpw)

    def heads(gx):
        return min(max(-(-512 // gx), 1), nbh, 65535)

    bgx = min(nrg, 1024)
    return dict(V=V, G=G, rows_per_wg=rpw, fwd=(nrg, heads(nrg)), bwd=(bgx, heads(bgx)), nparts=bgx * heads(bgx))


def k_ss(p) -> float:
    return 2 * p["V"] + 2 + math.log2(p["G"])


def e_r(p) -> float:
    return k_ss(p) / 2 + 3


def k_dw(p, B, R, H) -> int:
    nrg = -(-R // p["rows_per_wg"])
    per_lane = -(-nrg // p["bwd"][0]) * -(-(B * H) // p["bwd"][1])
    return per_lane + p["rows_per_wg"] + -(-p["nparts"] // 32) + 32


# ---- fp64 references, feature by feature ------------------------------------------------------------------
def _table64(R, D, offset, base=10000.0):
    pos = torch.arange(offset, offset + R, dtype=F64)
    inv = torch.tensor([base ** (-2.0 * i / D) for i in range(D // 2)], dtype=F64)
    ang = pos.view(R, 1) * inv.view(1, -1)
    return torch.cos(ang), torch.sin(ang)


def ref_forward(x, H, w, eps, offset=None, alpha=1.0, base=10000.0):
    """-> (out, rstd, scale) in fp64 on the CPU, written out index by index over the head's
    features.  ``offset``: the position of row 0 (None: no rotation).  ``scale``: what the forward
    bound is relative to: ``|out|`` without a rotation, ``|alpha| hypot(y1, y2)`` of the pair with."""
    B, R, C = x.shape
    D = C // H
    xv = x.detach().double().cpu().reshape(B, R, H, D)
    wv = w.detach().double().cpu()
    eps, alpha = f32(eps), f32(alpha)
    ss = torch.zeros(B, R, H, dtype=F64)
    for j in range(D):
        ss += xv[..., j] * xv[..., j]
    rstd = 1.0 / torch.sqrt(ss / D + eps)
    y = torch.empty_like(xv)
    for i in range(D):
        y[..., i] = xv[..., i] * rstd * wv[i]
    if offset is None:
        out = alpha * y
        return out.reshape(B, R, C), rstd, out.abs().reshape(B, R, C)
    cos, sin = _table64(R, D, offset, base)
    h = D // 2
    out, scale = torch.empty_like(y), torch.empty_like(y)
    for i in range(h):
        c, s = cos[:, i].view(1, R, 1), sin[:, i].view(1, R, 1)
        out[..., i] = alpha * (y[..., i] * c - y[..., i + h] * s)
        out[..., i + h] = alpha * (y[..., i + h] * c + y[..., i] * s)
        scale[..., i] = scale[..., i + h] = abs(alpha) * torch.hypot(y[..., i], y[..., i + h])
    return out.reshape(B, R, C), rstd, scale.reshape(B, R, C)


def ref_backward(g, x, H, w, eps, offset=None, alpha=1.0, base=10000.0):
    """-> (dx, dw, dx_scale, dw_scale) in fp64: the gradients of ``sum(g * forward(x, w))`` with the
    backward's factor ``alpha``, and the scales S_i and ``sum |gy|' |xh|`` of the bounds above."""
    B, R, C = x.shape
    D = C // H
    h = D // 2
    xv = x.detach().double().cpu().reshape(B, R, H, D)
    gv = g.detach().double().cpu().reshape(B, R, H, D)
    wv = w.detach().double().cpu()
    eps, alpha = f32(eps), f32(alpha)
    ss = torch.zeros(B, R, H, dtype=F64)
    for j in range(D):
        ss += xv[..., j] * xv[..., j]
    r = 1.0 / torch.sqrt(ss / D + eps)
    gy, gya = torch.empty_like(gv), torch.empty_like(gv)
    if offset is None:
        gy = alpha * gv
        gya = gy.abs()
    else:
        cos, sin = _table64(R, D, offset, base)
        for i in range(h):
            c, s = cos[:, i].view(1, R, 1), sin[:, i].view(1, R, 1)
            gy[..., i] = alpha * (gv[..., i] * c + gv[..., i + h] * s)
            gy[..., i + h] = alpha * (gv[..., i + h] * c - gv[..., i] * s)
            gya[..., i] = gya[..., i + h] = abs(alpha) * torch.hypot(gv[..., i], gv[..., i + h])
    xh = xv * r.unsqueeze(-1)
    p, pa = torch.zeros(B, R, H, dtype=F64), torch.zeros(B, R, H, dtype=F64)
    for j in range(D):
        p += gy[..., j] * wv[j] * xh[..., j]
        pa += gya[..., j] * wv[j].abs() * xh[..., j].abs()
    dx, sc = torch.empty_like(xv), torch.empty_like(xv)
    dw, dws = torch.empty(D, dtype=F64), torch.empty(D, dtype=F64)
    for i in range(D):
        dx[..., i] = r * (gy[..., i] * wv[i] - xh[..., i] * (p / D))
        sc[..., i] = r * (gya[..., i] * wv[i].abs() + xh[..., i].abs() * (pa / D))
        dw[i] = (gy[..., i] * xh[..., i]).sum()
        dws[i] = (gya[..., i] * xh[..., i].abs()).sum()
    return dx.reshape(B, R, C), dw, sc.reshape(B, R, C), dws


# ---- bounds ------------------------------------------------------------------------------------------------
def forward_bound(scale, dtype, p, rot: bool, alpha: float):
    e = e_r(p) + 2 + (E_ROT if rot else (1.0 if f32(alpha) != 1.0 else 0.0))
    return F * (scale * (e * U32 + EPS_OUT[dtype]) + TINY[dtype])


def dx_bound(dx_ref, dx_scale, dtype, p, rot: bool, alpha: float):
    e = (E_ROT if rot else (1.0 if f32(alpha) != 1.0 else 0.0)) + 3 * e_r(p) + k_ss(p) + 7
    return F * (dx_scale * e * U32 + dx_ref.abs() * EPS_OUT[dtype] + TINY[dtype])


def dw_bound(dw_ref, dw_scale, wdtype, p, rot: bool, alpha: float, B, R, H):
    e = (E_ROT if rot else (1.0 if f32(alpha) != 1.0 else 0.0)) + e_r(p) + 2 + k_dw(p, B, R, H)
    return F * (dw_scale * e * U32 + dw_ref.abs() * EPS_OUT[wdtype] + TINY[wdtype])


def worst(err, bound) -> float:
    """The largest |error| / unit bound (the bound without F)."""
    return (err / (bound / F).clamp_min(1e-300)).max().item()


# ---- emulation of the kernels' order of operations, in fp32 torch on the CPU -----------------------------
def _group_sum(per_lane):
    """(..., G) -> (...): the butterfly of ``__shfl_xor``: level o adds lane l ^ o."""
    G = per_lane.shape[-1]
    v = per_lane
    o = G // 2
    while o >= 1:
        v = v + v[..., torch.arange(G) ^ o]
        o //= 2
    return v[..., 0]


def _lane_chain(terms, p, D):
    """Sum over a head's D features in the kernel's order: lane ``ch`` adds the first-half elements
    [ch V, ch V + V), then the same of the second half, lane 0 then the odd tail; then the
    butterfly.  ``terms``: (..., D) fp32."""
    V, G, h = p["V"], p["G"], D // 2
    lanes = []
    for ch in range(G):
        acc = torch.zeros(terms.shape[:-1], dtype=F32)
        idx = [i for i in range(ch * V, min(ch * V + V, h))]
        for i in idx:
            acc = acc + terms[..., i]
        for i in idx:
            acc = acc + terms[..., h + i]
        if ch == 0 and D % 2:
            acc = acc + terms[..., D - 1]
        lanes.append(acc)
    return _group_sum(torch.stack(lanes, dim=-1))


def _rot32(y, cos, sin, alpha, inverse):
    h = y.shape[-1] // 2
    c = (cos.float() * alpha).view(1, -1, 1, h)
    s = (sin.float() * (-alpha if inverse else alpha)).view(1, -1, 1, h)
    y1, y2 = y[..., :h], y[..., h:]
    return torch.cat([y1 * c - y2 * s, y2 * c + y1 * s], dim=-1)


def emulate_forward(x, H, w, eps, offset=None, alpha=1.0, bug=None):
    """The forward kernel's algorithm in fp32 (unfused products), rounded once to ``x``'s dtype.
    ``bug``: 'eps_after_sqrt', 'mean_over_hd', 'rotate_first'.  -> (out, rstd fp32)."""
    B, R, C = x.shape
    D = C // H
    p = plan(B, R, H, D, x.element_size())
    xv = x.float().reshape(B, R, H, D)
    wv = w.float()
    eps32, al = torch.tensor(eps, dtype=F32), torch.tensor(alpha, dtype=F32)
    inv_d = torch.tensor(1.0, dtype=F32) / D
    ss = _lane_chain(xv * xv, p, D)
    if bug == "mean_over_hd":
        ss = ss.sum(-1, keepdim=True).expand_as(ss) / H
    if bug == "eps_after_sqrt":
        r = 1.0 / (torch.sqrt(ss * inv_d) + eps32)
    else:
        r = torch.rsqrt(ss * inv_d + eps32)
    tab = None if offset is None else tuple(t.float() for t in _table64(R, D, offset))
    if bug == "rotate_first":
        y = _rot32(xv, *tab, torch.tensor(1.0), False) * r.unsqueeze(-1) * wv * al
    elif tab is None:
        y = (xv * r.unsqueeze(-1)) * (wv * al)
    else:
        y = _rot32((xv * r.unsqueeze(-1)) * wv, *tab, al, False)
    return y.reshape(B, R, C).to(x.dtype), r


def emulate_backward(g, x, rstd, H, w, offset=None, alpha=1.0, bug=None):
    """The backward kernels' algorithm in fp32: dx rounded once to ``g``'s dtype, dw through the
    ordered partial sums (lane, lane groups of a workgroup, 32 strided chains, the chains) and
    rounded once to ``w``'s dtype.  ``bug``: 'no_projection', 'drop_partial'."""
    B, R, C = x.shape
    D = C // H
    p = plan(B, R, H, D, x.element_size())
    xv, gv, wv = x.float().reshape(B, R, H, D), g.float().reshape(B, R, H, D), w.float()
    al = torch.tensor(alpha, dtype=F32)
    inv_d = torch.tensor(1.0, dtype=F32) / D
    if offset is None:
        gy = gv * al
    else:
        gy = _rot32(gv, *(t.float() for t in _table64(R, D, offset)), al, True)
    r = rstd.float().unsqueeze(-1)
    xh = xv * r
    gw = gy * wv
    m = _lane_chain(gw * xh, p, D).unsqueeze(-1) * inv_d
    if bug == "no_projection":
        m = torch.zeros_like(m)
    dx = ((gw - xh * m) * r).reshape(B, R, C).to(g.dtype)
    # dw: workgroup (bx, by) owns the row groups bx, bx + gx, ... and the (b, h) pairs by, by + gy, ...
    rpw, (gx, gyy) = p["rows_per_wg"], p["bwd"]
    t = (gy * xh).permute(1, 0, 2, 3).reshape(R, B * H, D)  # bh = b * H + h
    nrg = -(-R // rpw)
    parts = []
    for by in range(gyy):
        for bx in range(gx):
            lanes = torch.zeros(rpw, D, dtype=F32)  # one accumulator row per lane group
            for rg in range(bx, nrg, gx):
                rows = t[rg * rpw:(rg + 1) * rpw]
                for bh in range(by, B * H, gyy):
                    lanes[:rows.shape[0]] = lanes[:rows.shape[0]] + rows[:, bh]
            part = lanes[0].clone()
            for k in range(1, rpw):
                part = part + lanes[k]
            parts.append(part)
    if bug == "drop_partial":
        parts[len(parts) // 2] = torch.zeros(D, dtype=F32)
    chains = []
    for j in range(32):
        acc = torch.zeros(D, dtype=F32)
        for q in range(j, len(parts), 32):
            acc = acc + parts[q]
        chains.append(acc)
    dw = chains[0].clone()
    for k in range(1, 32):
        dw = dw + chains[k]
    return dx, dw.to(w.dtype)


