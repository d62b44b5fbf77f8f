"""The score profiles of tests/_flash_profiles.py against a torch emulation of the 16-bit flash
kernels' algorithm (CPU only): every kind does what its name claims, the reference algorithm alone
stays within the forward and backward bounds the GPU tests assert, and three deliberately wrong
emulations are caught by them.

The emulation follows csrc/flash_fwd.hip / csrc/flash_wide.hip: column tiles, the running max only
moved when some row of a 32-row group exceeds it by the threshold (then every row of the group moves
to its own new max), P = 2^(s - m) rounded to the dtype for the PV product while ``l`` sums the
unrounded P, fp32 accumulators, the output rounded once.  The backward emulation has the kernels'
rounding points: P and dS rounded to the dtype before their products, delta from the rounded output,
d_rows rounded to the dtype."""
import math

import pytest
import torch

import _flash_profiles as fp

NEG_INF = -float("inf")


def prescale_emu(rows, scale):
    """flash.prescale: rows * (scale * log2 e) in fp32, rounded once to the dtype."""
    return (rows.float() * (scale * fp.LOG2E)).to(rows.dtype)


def emulate_fwd(rows_used, kc, vc, mask, H, scale, prescaled, tile, threshold=fp.THRESHOLD, bug=None):
    """-> (out in the dtype, lse fp32).  ``bug``: None, or one of
    'l_not_rescaled' (the rescale leaves ``l`` alone), 'o_slice_not_rescaled' (it skips output
    coordinates 32..63), 'mask_after_max' (the row max is taken before the mask is applied)."""
    dtype = rows_used.dtype
    B, R, C = rows_used.shape
    T, D = kc.shape[1], C // H
    # exact products, fp32 accumulation: fp64 rounded once to fp32 stands in for the MFMA chain
    s2 = fp._scores2(rows_used, kc, H, H, scale, prescaled).float()
    dead = torch.zeros(B, 1, R, T, dtype=torch.bool) if mask is None else mask.unsqueeze(1)
    v = fp._heads(vc, H).float()
    Rp = (R + fp.GROUP - 1) // fp.GROUP * fp.GROUP
    m = torch.full((B, H, R), NEG_INF)
    l = torch.zeros(B, H, R)
    o = torch.zeros(B, H, R, D)
    for t0 in range(0, T, tile):
        cols = slice(t0, min(T, t0 + tile))
        st = s2[..., cols].masked_fill(dead[..., cols], NEG_INF)
        mx = (s2[..., cols] if bug == "mask_after_max" else st).amax(-1)
        m_new = torch.maximum(m, mx)
        want = torch.zeros(B, H, Rp, dtype=torch.bool)
        want[..., :R] = m_new > m + threshold
        trig = want.view(B, H, -1, fp.GROUP).any(-1, keepdim=True).expand(-1, -1, -1, fp.GROUP).reshape(B, H, Rp)[..., :R]
        alpha = torch.exp2(m - torch.where(m_new == NEG_INF, torch.zeros_like(m_new), m_new))
        alpha = torch.where(trig, alpha, torch.ones_like(alpha))
        if bug != "l_not_rescaled":
            l = l * alpha
        a_o = alpha.unsqueeze(-1).expand(-1, -1, -1, D).clone()
        if bug == "o_slice_not_rescaled":
            a_o[..., 32:64] = 1.0
        o = o * a_o
        m = torch.where(trig, m_new, m)
        p = torch.exp2(st - torch.where(m == NEG_INF, torch.zeros_like(m), m).unsqueeze(-1))
        l = l + p.sum(-1)
        o = o + p.to(dtype).float() @ v[:, :, cols]
    out = (o / l.unsqueeze(-1)).to(dtype).transpose(1, 2).reshape(B, R, C)
    return out, (m + torch.log2(l)) * math.log(2.0)


def emulate_bwd(dout, rows_used, kc, vc, out, lse, mask, H, scale, prescaled):
    """-> (d_rows in the dtype, d_kc fp32, d_vc fp32) with the kernels' rounding points."""
    dtype = rows_used.dtype
    B, R, C = rows_used.shape
    T = kc.shape[1]
    s2 = fp._scores2(rows_used, kc, H, H, scale, prescaled).float()
    if mask is not None:
        s2 = s2.masked_fill(mask.unsqueeze(1), NEG_INF)
    k = fp._heads(rows_used, H).float()
    if prescaled:
        k = k / (scale * fp.LOG2E)
    q, v, do = fp._heads(kc, H).float(), fp._heads(vc, H).float(), fp._heads(dout, H).float()
    P = torch.exp2(s2 - (lse.float() * fp.LOG2E).unsqueeze(-1))
    delta = (do * fp._heads(out, H).float()).sum(-1, keepdim=True)
    dS = (P * (do @ v.transpose(-1, -2) - delta)).to(dtype).float()
    P16 = P.to(dtype).float()
    d_rows = (scale * (dS @ q)).transpose(1, 2).reshape(B, R, C).to(dtype)
    d_kc = (scale * (dS.transpose(-1, -2) @ k)).transpose(1, 2).reshape(B, T, C)
    d_vc = (P16.transpose(-1, -2) @ do).transpose(1, 2).reshape(B, T, C)
    return d_rows, d_kc, d_vc


# (B, R, T, H, D): a narrow shape with a ragged tail, the creep shape, a wide-head shape (tile 32)
NARROW, CREEP, WIDE = (1, 128, 300, 2, 64), (1, 64, 600, 1, 96), (1, 96, 200, 1, 160)
CASES = [(kind, NARROW) for kind in fp.KINDS if kind != "creep"] + [("creep", CREEP)] + \
        [(kind, WIDE) for kind in ("ramp", "late_spike", "late_spike_tail", "deep_negative", "masked_peak")]


def _case(kind, shape, dtype, prescaled, lead=False):
    B, R, T, H, D = shape
    scale = 1.0 / math.sqrt(D)
    rows, kc, vc = fp.make_profile(kind, B, R, T, H, D, dtype, seed=sum(shape))
    mask = fp.make_mask(kind, B, R, T, seed=sum(shape), lead=lead)
    rk = prescale_emu(rows, scale) if prescaled else rows
    return rk, kc, vc, mask, H, scale, fp.tile_of(D), fp.make_dout(B, R, H, D, dtype, seed=sum(shape))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("prescaled", [False, True], ids=["plain", "prescaled"])
@pytest.mark.parametrize("kind,shape", CASES)
def test_emulation_within_bounds(kind, shape, dtype, prescaled):
    """check_profile holds, and the reference algorithm passes the forward and backward assertions."""
    for lead in ((False, True) if kind == "masked_peak" else (False,)):
        rk, kc, vc, mask, H, scale, tile, do = _case(kind, shape, dtype, prescaled, lead)
        ref_out, ref_lse, s2 = fp.reference(rk, kc, vc, mask, H, scale, prescaled)
        st = fp.check_profile(s2, tile, kind, mask)
        assert st.pr_min > 1.0
        out, lse = emulate_fwd(rk, kc, vc, mask, H, scale, prescaled, tile)
        f = fp.assert_forward(kind, out, lse, ref_out, ref_lse, dtype)
        spec = fp.backward_spec(do, rk, kc, vc, out, lse, mask, H, scale, prescaled)
        r = fp.assert_backward(kind, *emulate_bwd(do, rk, kc, vc, out, lse, mask, H, scale, prescaled), spec, dtype)
        print(f"{kind} {shape} pr min {st.pr_min:.1f} median {st.pr_median:.1f} fwd {f} bwd {r}")


def test_random_scores_within_bounds():
    """The plain randn case of the existing suite passes the same backward bound."""
    B, R, T, H, D = NARROW
    g = torch.Generator(device="cpu").manual_seed(0)
    rows, kc, vc, do = (torch.randn(B, n, H * D, generator=g).to(torch.bfloat16) for n in (R, T, T, R))
    scale = 1.0 / math.sqrt(D)
    out, lse = emulate_fwd(rows, kc, vc, None, H, scale, False, 64)
    spec = fp.backward_spec(do, rows, kc, vc, out, lse, None, H, scale, False)
    fp.assert_backward("randn", *emulate_bwd(do, rows, kc, vc, out, lse, None, H, scale, False), spec, torch.bfloat16)


def _caught(bug, kind, dtype=torch.bfloat16, prescaled=False):
    rk, kc, vc, mask, H, scale, tile, _ = _case(kind, NARROW, dtype, prescaled)
    ref_out, ref_lse, _ = fp.reference(rk, kc, vc, mask, H, scale, prescaled)
    out, lse = emulate_fwd(rk, kc, vc, mask, H, scale, prescaled, tile, bug=bug)
    try:
        fp.assert_forward(kind, out, lse, ref_out, ref_lse, dtype)
    except AssertionError as e:
        return str(e)
    return None


@pytest.mark.parametrize("bug,kinds", [
    ("l_not_rescaled", ("ramp", "creep", "late_spike", "late_spike_tail", "plateau", "masked_peak")),
    ("o_slice_not_rescaled", ("ramp", "creep", "late_spike", "late_spike_tail", "plateau", "masked_peak")),
    ("mask_after_max", ("masked_peak",)),
])
def test_wrong_emulations_are_caught(bug, kinds):
    """The forward assertions fail for each broken emulation, on every kind that reaches the broken
    code with a finite running max; random scores (the existing suite's data) do not notice the two
    rescale bugs at all."""
    for kind in kinds:
        if kind == "creep":
            B, R, T, H, D = CREEP
            scale = 1.0 / math.sqrt(D)
            rows, kc, vc = fp.make_profile(kind, B, R, T, H, D, torch.bfloat16, seed=1)
            ref_out, ref_lse, _ = fp.reference(rows, kc, vc, None, H, scale, False)
            out, lse = emulate_fwd(rows, kc, vc, None, H, scale, False, 64, bug=bug)
            with pytest.raises(AssertionError):
                fp.assert_forward(kind, out, lse, ref_out, ref_lse, torch.bfloat16)
            continue
        for dtype in (torch.bfloat16, torch.float16):
            msg = _caught(bug, kind, dtype)
            assert msg is not None, f"{bug} on {kind} ({dtype}) passed the forward assertions"
            print(f"caught {bug} on {kind} ({dtype}): {msg}")
    if bug != "mask_after_max":
        B, R, T, H, D = NARROW
        g = torch.Generator(device="cpu").manual_seed(0)
        rows, kc, vc = (torch.randn(B, n, H * D, generator=g).to(torch.bfloat16) for n in (R, T, T))
        ref_out, ref_lse, _ = fp.reference(rows, kc, vc, None, H, 0.125, False)
        out, lse = emulate_fwd(rows, kc, vc, None, H, 0.125, False, 64, bug=bug)
        fp.assert_forward("randn", out, lse, ref_out, ref_lse, torch.bfloat16)   # the gap this file closes
