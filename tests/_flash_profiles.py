"""Score profiles that move the running max of the 16-bit flash kernels, an fp64 reference, the
operation ``flash.bwd`` is documented to compute, and the assertions both the CPU emulation
(tests/test_flash_profiles.py) and the GPU tests (tests/test_flash_profiles_gpu.py) use.

Random ``randn`` operands give scores ~ N(0, 1): the first column tile sets the running max and no
later tile exceeds it by the kernels' deferred-rescale threshold (8 log2 units), so the rescale of
``l`` and of the output accumulators only ever runs from ``m = -inf`` on zeros.  The profiles here
overwrite coordinate 0 of every head with exact small integers, ``rows[..., h*D] = b_i`` and
``kc[..., h*D] = a_j``: the score is ``a_j * b_i * scale`` plus the ~N(0, 1) noise of the other
coordinates, and every operand is exact in bf16 and fp16.

Not collected as a test (no ``test_`` prefix).
"""
import math
from types import SimpleNamespace

import torch

LOG2E = 1.0 / math.log(2.0)
THRESHOLD = 8.0   # RESCALE_LOG2 (csrc/flash_fwd.hip), Pol::RESCALE (csrc/flash_wide.hip, 16-bit)
GROUP = 32        # rows of one wave: the rescale trigger is shared by them (__any)
# both signs, large and small: every 32-row group holds rows that jump, fall, creep and stay
B_PATTERN = (8, -8, 1, 0, 3, -2, 5, -1)
KINDS = ("ramp", "creep", "late_spike", "late_spike_tail", "plateau", "deep_negative", "masked_peak")


def tile_of(D: int) -> int:
    """Column tile of the 16-bit forward: 64 (csrc/flash_fwd.hip, D <= 128), 32 (csrc/flash_wide.hip)."""
    return 64 if D <= 128 else 32


def eps_of(dtype) -> float:
    """Half an ulp of 1: the relative error of one rounding to ``dtype``."""
    return {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -11}[dtype]


def _int_at_least(x: float) -> int:
    return int(math.ceil(x - 1e-9))


def _levels(T: int, tile: int, cap=None) -> torch.Tensor:
    """j // tile, except that a ragged tail narrower than half a tile keeps the level of the tile
    before it: the rows that end on the top level then spread over >= tile / 2 columns (the
    participation ratio of n columns with N(0, 1)-nat noise is about n / e, and it must stay >= 4)."""
    lev = torch.arange(T) // tile
    top = (T - tile // 2) // tile if T > tile else 0
    lev = lev.clamp(max=max(top, 0))
    if cap is not None:
        lev = lev.clamp(max=cap)
    return lev


def profile_a(kind: str, T: int, D: int, spike_log2: float = 40.0) -> torch.Tensor:
    """The column coordinate ``a_j`` (exact small integers, fp64 tensor of T values).  ``spike_log2``:
    how far the late spike lifts the rows with b = 8.  The default keeps |a_j| small, because the profile
    coordinate of d_rows is sum_j dS_ij a_j with sum_j dS_ij = 0: its rounding error grows with |a_j|
    while its value does not, and the relative Frobenius bound of the backward has to hold for a
    correct kernel.  The forward-only tests of the partial-slot merges ask for 150 (> 100 nats)."""
    tile = tile_of(D)
    c8 = 8.0 / math.sqrt(D) * LOG2E                       # log2 units per unit of a for rows with b = 8
    if kind == "ramp":                                    # b = 8 rows: >= 10 log2 units up per tile
        # step * (j // tile), centred: a constant added to a_j moves every score of a row alike and
        # leaves its softmax alone, but halves the largest |a_j| (see spike_log2 above: at 16 tiles the
        # uncentred ramp takes the CPU emulation of a correct kernel past the Frobenius bound of d_rows)
        lev = _levels(T, tile)
        return (_int_at_least(10.0 / c8) * (lev - lev.max() // 2)).double()
    if kind == "plateau":                                 # two such jumps, then flat
        return (_int_at_least(10.0 / c8) * _levels(T, tile, cap=2)).double()
    if kind == "creep":                                   # 1-3 log2 units per tile
        step = max(1, round(2.5 / c8))
        assert 1.0 <= step * c8 <= 3.0, (D, step * c8)
        return (step * _levels(T, tile)).double()
    if kind in ("late_spike", "late_spike_tail"):         # flat, then one tile far above (b > 0) or below (b < 0)
        amp = _int_at_least(spike_log2 / c8)
        a = torch.zeros(T, dtype=torch.float64)
        if kind == "late_spike":
            t = T // tile - 2
            assert t >= 1, "late_spike needs three full tiles"
            a[t * tile:(t + 1) * tile] = amp
        else:
            assert T % tile, "late_spike_tail needs a ragged tail tile"
            start = (T - 1) // tile * tile
            if T - start < tile // 2:
                start -= tile
            a[start:] = amp
        return a
    if kind == "deep_negative":                           # b = -8 rows: every score at -14 log2 units + noise
        assert T % tile, "deep_negative needs padded tail columns"
        return torch.full((T,), float(max(8, _int_at_least(14.0 / c8))), dtype=torch.float64)
    if kind == "masked_peak":
        # live columns alternate per column tile between hi and hi - s (s: ~10 log2 units for
        # b = 8 rows); hidden columns carry 4 * hi: 130 log2 units above the live max of a b = 8 row,
        # more than fp32's exponent range holds below 1 (a max taken before masking flushes every
        # live probability to zero; 20 units would be absorbed without a trace in bf16)
        hi = 8 * _int_at_least(130.0 / (3.0 * c8) / 8.0)
        s = _int_at_least(10.0 / c8)
        a = torch.where((torch.arange(T) // tile) % 2 == 0, float(hi), float(hi - s)).double()
        a[hidden_columns(T)] = 4.0 * hi
        return a
    raise ValueError(kind)


def hidden_columns(T: int) -> torch.Tensor:
    """masked_peak: the columns hidden from every row: the whole mask tile [64, 128) (flag 1) and
    every 7th column elsewhere (flag 2: hidden columns inside live tiles, the tail tile included)."""
    j = torch.arange(T)
    return ((j >= 64) & (j < 128)) | (j % 7 == 3)


def make_profile(kind, B, R, T, H, D, dtype, seed, Hg=None, spike_log2=40.0):
    """-> (rows (B, R, H*D), kc, vc (B, T, Hg*D)) on the CPU in ``dtype``."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    Hg = Hg or H
    rows = torch.randn(B, R, H * D, generator=g)
    kc = torch.randn(B, T, Hg * D, generator=g)
    vc = torch.randn(B, T, Hg * D, generator=g)
    b = torch.tensor(B_PATTERN, dtype=torch.float32)[torch.arange(R) % len(B_PATTERN)]
    a = profile_a(kind, T, D, spike_log2).float()
    assert a.abs().max() <= 2048 and torch.equal(a, a.to(dtype).float()), "a_j must be exact in the dtype"
    rows[:, :, ::D] = b[None, :, None]
    kc[:, :, ::D] = a[None, :, None]
    return rows.to(dtype), kc.to(dtype), vc.to(dtype)


def make_mask(kind, B, R, T, seed, lead=False):
    """The dense mask of ``masked_peak`` (None for the other kinds): the hidden columns for every row,
    plus 15 % of the live ones at random.  ``lead``: the first 128 columns hidden as well, so the
    running max goes -inf -> finite -> jump."""
    if kind != "masked_peak":
        return None
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    mask = torch.rand(B, R, T, generator=g) < 0.15
    mask |= hidden_columns(T)[None, None, :]
    if lead:
        mask[..., :128] = True
    return mask


def make_dout(B, R, H, D, dtype, seed):
    g = torch.Generator(device="cpu").manual_seed(seed + 2)
    return torch.randn(B, R, H * D, generator=g).to(dtype)


def make_case(kind, shape, dtype, device="cpu", Hg=None, spike_log2=40.0):
    """One test case on ``device``: operands, mask, dO and the constants that go with them.  ``kind``
    may be 'masked_peak_lead' (``make_mask(..., lead=True)``).  The seed is a function of the shape."""
    B, R, T, H, D = shape
    base, lead = (kind[:-5], True) if kind.endswith("_lead") else (kind, False)
    seed = sum(shape) + 7 * KINDS.index(base)
    rows, kc, vc = make_profile(base, B, R, T, H, D, dtype, seed, Hg, spike_log2)
    mask = make_mask(base, B, R, T, seed, lead)
    return SimpleNamespace(kind=base, shape=shape, dtype=dtype, H=H, Hg=Hg, D=D, scale=1.0 / math.sqrt(D), tile=tile_of(D),
                           rows=rows.to(device), kc=kc.to(device), vc=vc.to(device),
                           mask=None if mask is None else mask.to(device),
                           dout=make_dout(B, R, H, D, dtype, seed).to(device))


# ---- fp64 reference --------------------------------------------------------------------------------
def _heads(x, H, rep=1):
    B, N, C = x.shape
    h = x.double().view(B, N, H, C // H).transpose(1, 2)
    return h.repeat_interleave(rep, dim=1) if rep > 1 else h


def _scores2(rows_used, kc, H, Hg, scale, prescaled):
    k, q = _heads(rows_used, H), _heads(kc, Hg, H // Hg)
    s2 = k @ q.transpose(-1, -2)
    return s2 if prescaled else s2 * (scale * LOG2E)


def reference(rows_used, kc, vc, mask, H, scale, prescaled, Hg=None):
    """fp64 -> (out (B, R, H*D), lse (B, H, R) natural log, scores (B, H, R, T) in log2 units, unmasked).

    ``prescaled``: ``rows_used`` is the pre-scaled 16-bit buffer the kernel reads (``flash.prescale``:
    rows * scale * log2 e, rounded once); that rounding is an input here, not kernel error."""
    Hg = Hg or H
    B, R, C = rows_used.shape
    s2 = _scores2(rows_used, kc, H, Hg, scale, prescaled)
    s = s2 / LOG2E
    if mask is not None:
        s = s.masked_fill(mask.unsqueeze(1), -float("inf"))
    lse = torch.logsumexp(s, -1)
    out = torch.exp(s - lse.unsqueeze(-1)) @ _heads(vc, Hg, H // Hg)
    return out.transpose(1, 2).reshape(B, R, C), lse, s2


def backward_spec(dout, rows_used, kc, vc, out_given, lse_given, mask, H, scale, prescaled, Hg=None):
    """What ``flash.bwd`` is documented to compute from the ``out`` and ``lse`` it is handed, in fp64:
    P = exp(s - lse_given), delta = rowsum(dO * out_given), dS = P * (dP - delta); d_rows = scale dS q,
    d_kc = scale dS^T k, d_vc = P^T dO, with k the unscaled rows (``prescaled``: rows_used / (scale log2 e)).

    Also the sums the element bounds are made of: ``b_rows`` = scale |dS| |q|, ``b_kc`` = scale |dS|^T |k|,
    ``b_vc`` = P^T |dO|; and what multiplies an absolute error of every dS (P) element: ``u_rows`` = scale 1^T |q|,
    ``u_kc`` = scale 1^T |k|, ``u_vc`` = 1^T |dO|."""
    Hg = Hg or H
    G = H // Hg
    B, R, C = rows_used.shape
    T = kc.shape[1]
    s = _scores2(rows_used, kc, H, Hg, scale, prescaled) / LOG2E
    if mask is not None:
        s = s.masked_fill(mask.unsqueeze(1), -float("inf"))
    k = _heads(rows_used, H)
    if prescaled:
        k = k / (scale * LOG2E)
    q, v, do = _heads(kc, Hg, G), _heads(vc, Hg, G), _heads(dout, H)
    P = torch.exp(s - lse_given.double().unsqueeze(-1))
    delta = (do * _heads(out_given, H)).sum(-1, keepdim=True)
    dS = P * (do @ v.transpose(-1, -2) - delta)
    aS = dS.abs()

    def rows_layout(x):     # (B, H, R, D) -> (B, R, H*D)
        return x.transpose(1, 2).reshape(B, R, C)

    def cols_layout(x):     # (B, H, T, D) -> (B, T, Hg*D), summed over each group of row heads
        x = x.view(B, Hg, G, T, C // H).sum(2)
        return x.transpose(1, 2).reshape(B, T, Hg * (C // H))

    return SimpleNamespace(
        d_rows=rows_layout(scale * (dS @ q)), d_kc=cols_layout(scale * (dS.transpose(-1, -2) @ k)),
        d_vc=cols_layout(P.transpose(-1, -2) @ do),
        b_rows=rows_layout(scale * (aS @ q.abs())), b_kc=cols_layout(scale * (aS.transpose(-1, -2) @ k.abs())),
        b_vc=cols_layout(P.transpose(-1, -2) @ do.abs()),
        u_rows=rows_layout(scale * q.abs().sum(-2, keepdim=True).expand(-1, -1, R, -1)),
        u_kc=cols_layout(scale * k.abs().sum(-2, keepdim=True).expand(-1, -1, T, -1)),
        u_vc=cols_layout(do.abs().sum(-2, keepdim=True).expand(-1, -1, T, -1)), absdS=aS, P=P)


# ---- does the profile do what its name claims? -------------------------------------------------------
def check_profile(scores2, tile, kind, mask=None):
    """Asserts on the reference's log2 scores (B, H, R, T) (unmasked; ``mask`` (B, R, T) hides) that
    the kind exercises what it is meant to; counts in the message on failure."""
    s = scores2.double()
    live = s if mask is None else s.masked_fill(mask.unsqueeze(1), -float("inf"))
    B, H, R, T = s.shape
    nt = (T + tile - 1) // tile
    pad = torch.full((B, H, R, nt * tile - T), -float("inf"), dtype=s.dtype, device=s.device)
    tmax = torch.cat([live, pad], -1).view(B, H, R, nt, tile).amax(-1)
    run = torch.cummax(tmax, -1).values                     # running max after each tile
    prev = run[..., :-1]
    rise = torch.where(torch.isfinite(prev), run[..., 1:] - prev, torch.zeros_like(prev))  # after the first live tile
    njump = (rise > THRESHOLD).sum(-1)                      # (B, H, R)
    ngroups = (R + GROUP - 1) // GROUP
    jp = torch.zeros(B, H, ngroups * GROUP, dtype=torch.bool, device=s.device)
    no = jp.clone()
    jp[..., :R], no[..., :R] = njump > 0, njump == 0
    mixed = (jp.view(B, H, ngroups, GROUP).any(-1) & no.view(B, H, ngroups, GROUP).any(-1)).sum().item()
    info = f"{kind}: rows with a jump {int((njump > 0).sum())}/{njump.numel()}, most jumps on a row {int(njump.max())}, mixed groups {mixed}"
    if kind in ("ramp", "late_spike", "late_spike_tail", "plateau"):
        assert mixed >= 1, info
    if kind == "ramp":
        assert njump.max().item() >= 3, info
    if kind == "creep":
        total = rise.sum(-1)
        creeping = total > 2 * THRESHOLD
        info += f", creeping rows {int(creeping.sum())}, their largest single rise {rise[creeping].max().item() if creeping.any() else float('nan'):.2f}"
        assert creeping.any() and rise[creeping].max().item() <= THRESHOLD, info
    if kind == "deep_negative":
        deep = (live.amax(-1) <= -10.0).sum().item()
        assert deep >= 1, info + f", rows with max <= -10: {deep}"
    if kind == "masked_peak":
        assert mask is not None
        hid = s.masked_fill(~mask.unsqueeze(1), -float("inf")).amax(-1)
        gap = (hid - live.amax(-1)).max().item()
        assert gap > 20.0, info + f", hidden max - live max {gap:.1f}"
    p = torch.softmax(live / LOG2E, -1)
    pr = 1.0 / p.pow(2).sum(-1)
    frac = (pr >= 4.0).double().mean().item()
    assert frac >= 0.9, info + f", participation ratio >= 4 on {frac:.2%} of rows (min {pr.min().item():.2f})"
    return SimpleNamespace(njump=njump, mixed=mixed, pr_min=pr.min().item(), pr_median=pr.median().item())


# ---- assertions ------------------------------------------------------------------------------------
def close(what, a, b, fro, elem=10.0):
    """tests/test_flash_gpu.py::_close: rel. Frobenius error <= fro, and |a - b| <= elem * fro *
    (|b| + 0.25 rms(b)) everywhere.  -> (Frobenius error / fro, worst element / its bound)."""
    a, b = a.double(), b.double()
    assert torch.isfinite(a).all(), f"{what}: non-finite"
    err = ((a - b).norm() / b.norm().clamp_min(1e-12)).item()
    assert err <= fro, f"{what}: relative Frobenius error {err:.3e} > {fro:.1e}"
    rms = b.pow(2).mean().sqrt()
    bound = elem * fro * (b.abs() + 0.25 * rms)
    worst = ((a - b).abs() / bound).max().item()
    assert worst <= 1.0, f"{what}: an element is {worst:.2f}x past its bound"
    return err / fro, worst


FWD_FRO = {torch.bfloat16: 1e-2, torch.float16: 3e-3}
BWD_FRO = {torch.bfloat16: 1.5e-2, torch.float16: 4e-3}
LSE_TOL = 1e-2
# Element bound of the backward: FACTOR * (the first-order model of the kernels' roundings).  The
# model is the 16-bit rounding of dS (d_rows, d_kc) and of P (d_vc) plus the rounding of a 16-bit
# output; the factor 2 is for the second-order terms (v_exp_f32, fp32 accumulation order, fp32
# lse / delta).  Measured ratios to the UNIT bound (FACTOR = 1) are listed at MEASURED below.
BWD_FACTOR = 2.0
# Below its normal range a format rounds with an ABSOLUTE error, which the relative model above
# does not see: fp16 is subnormal under 2^-14 (spacing 2^-24, so up to 2^-25 per element; a dS of
# 2^-27 becomes 0), and the fp32 the kernels compute P in holds nothing under 2^-126.  Peaked
# profiles have such elements by construction (a column 20 log2 units under its row's max), and an
# output coordinate made only of them (the profile coordinate of a row whose spike columns are
# the only ones with a_j != 0) has a reference as small as that error.  The unit bound therefore
# also carries UNDERFLOW[dtype] * (the 1-norm that multiplies a per-element absolute error):
# at most 2^-25 * scale * sum_j |q_j|, about 1e-5 of a typical gradient element here.
UNDERFLOW = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -25}
# MEASURED (worst ratio of |error| to the unit bound, d_rows / d_kc / d_vc, over every kind and shape
# of tests/test_flash_profiles_gpu.py, prescaled or not):
#   CPU emulation of those cases:   bf16 1.42 / 1.65 / 1.39   fp16 0.67 / 0.79 / 0.74
#   MI355X, narrow (D <= 128):      bf16 1.35 / 1.55 / 1.39   fp16 0.65 / 0.73 / 0.74
#   MI355X, wide (D = 160-384):     bf16 1.42 / 1.50 / 1.36   fp16 0.67 / 0.60 / 0.60
# The kernels sit where the rounding model alone does, so the factor stays 2.


def assert_forward(what, out, lse, ref_out, ref_lse, dtype):
    """Finite wherever the reference is, then the forward tolerances of tests/test_flash_gpu.py."""
    assert torch.isfinite(ref_out).all() and torch.isfinite(ref_lse).all(), f"{what}: the profile has a dead row"
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all(), f"{what}: non-finite output"
    fr, el = close(f"{what} out", out, ref_out, FWD_FRO[dtype])
    le = (lse.double() - ref_lse).abs().max().item()
    assert le < LSE_TOL, f"{what}: lse off by {le:.3e}"
    return {"out_fro": fr, "out_elem": el, "lse": le / LSE_TOL}


def assert_backward(what, d_rows, d_kc, d_vc, spec, dtype):
    """Against :func:`backward_spec`: the Frobenius tolerances of tests/test_flash_gpu.py and
        |d_rows - ref| <= F (eps scale |dS| |q| + eps |ref|)
        |d_kc  - ref| <= F  eps scale |dS|^T |k|
        |d_vc  - ref| <= F  eps P^T |dO|
    (+ eps |ref| for any output that is itself 16-bit), eps = 2^-9 (bf16) / 2^-11 (fp16), F = 2; every
    eps |x| term also carries the format's absolute rounding error under its normal range (UNDERFLOW).
    -> the worst ratio to the unit bound (F = 1) per output."""
    eps, ratios, errs = eps_of(dtype), {}, []
    u = UNDERFLOW[dtype]
    for name, got, ref, model, under in (("d_rows", d_rows, spec.d_rows, spec.b_rows, spec.u_rows),
                                         ("d_kc", d_kc, spec.d_kc, spec.b_kc, spec.u_kc),
                                         ("d_vc", d_vc, spec.d_vc, spec.b_vc, spec.u_vc)):
        if got is None:  # (a test of one kernel alone hands in what that kernel computes)
            continue
        assert torch.isfinite(ref).all()
        assert torch.isfinite(got.float()).all(), f"{what} {name}: non-finite"
        unit = eps * model + u * under + (eps * ref.abs() + u if got.dtype != torch.float32 else 0.0)
        ratios[name] = ((got.double() - ref).abs() / unit).max().item()
        fro = ((got.double() - ref).norm() / ref.norm().clamp_min(1e-300)).item()
        ratios[name + "_fro"] = fro / BWD_FRO[dtype]
        if fro > BWD_FRO[dtype]:
            errs.append(f"{name}: relative Frobenius error {fro:.3e} > {BWD_FRO[dtype]:.1e}")
        if ratios[name] > BWD_FACTOR:
            errs.append(f"{name}: an element is {ratios[name]:.2f}x its unit bound (allowed {BWD_FACTOR})")
    assert not errs, f"{what}: " + "; ".join(errs) + f"  [ratios {ratios}]"
    return ratios
