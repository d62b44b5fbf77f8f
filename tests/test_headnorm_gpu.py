"""QK-norm on the MI355X: the per-head RMSNorm kernels (``csrc/headnorm.hip``) against fp64 under
the rounding model of ``tests/_headnorm_ref.py``, strided views and in-place calls, and the module
with ``qk_norm=True`` on the flash / ring paths against the dense fp64 reference."""
import math

import pytest
import torch

import _headnorm_ref as ref
from _headnorm_ref import BF16, DT_IDS, F32, FP16

pytestmark = pytest.mark.gpu

DTYPES = [BF16, FP16, F32]
SHAPES = [(1, 1, 1, 96), (2, 63, 8, 96), (1, 65, 3, 64), (2, 257, 2, 128), (1, 130, 2, 160), (1, 70, 1, 384),
          (1, 33, 5, 7), (1, 3125, 8, 96)]
EPS = 1e-6


def _inputs(shape, dtype, seed=0, kind="normal"):
    """x, g (B, R, H*D) and a gain (D,) away from 1, on the CPU in ``dtype``."""
    B, R, H, D = shape
    gen = torch.Generator().manual_seed(1000 * seed + B * 100 + R)
    x = torch.randn(B, R, H * D, generator=gen)
    g = torch.randn(B, R, H * D, generator=gen)
    w = torch.rand(D, generator=gen) + 0.5
    if kind == "scaled":      # squares past fp16's range
        x = x * 200.0
    elif kind == "zero_rows":
        x[:, ::3] = 0.0
    elif kind == "huge":      # one element carries the head's norm
        x.view(B, R, H, D)[..., 0, D // 3] = 3.0e4
    return x.to(dtype), g.to(dtype), w.to(dtype)


def _variants(D):
    """(rotary offset or None, alpha): plain, scaled, and with an even D rotated."""
    v = [(None, 1.0), (None, 0.37)]
    if D % 2 == 0:
        v += [(1000, 1.0), (1000, 0.1803)]
    return v


def _check(gpu, shape, dtype, kind="normal", wdtype=None):
    import xdot
    from xdot.ops.headnorm import head_rms_norm_apply, head_rms_norm_backward

    B, R, H, D = shape
    x, g, w = _inputs(shape, dtype, kind=kind)
    if wdtype is not None:
        w = w.to(wdtype)
    p = ref.plan(B, R, H, D, x.element_size())
    assert list(torch.ops.xdot.headnorm_plan(B, R, H, D, dtype)) == [p["G"], p["rows_per_wg"], *p["fwd"], *p["bwd"]]
    xg, gg, wg = x.to(gpu), g.to(gpu), w.to(gpu)
    rot = xdot.Rotary()
    for off, alpha in _variants(D):
        tab = (None, None) if off is None else rot.table(R, D, off, gpu)
        out, rstd, saved = head_rms_norm_apply(xg, H, wg, EPS, *tab, alpha=alpha, save=True)
        assert out.dtype == dtype and out.is_contiguous() and rstd.dtype == F32 and tuple(rstd.shape) == (B, R, H)
        assert torch.equal(saved, xg) and saved.is_contiguous()  # a bit copy
        o64, r64, scale = ref.ref_forward(x, H, w, EPS, off, alpha)
        bound = ref.forward_bound(scale, dtype, p, off is not None, alpha)
        err = (out.double().cpu() - o64).abs()
        rerr = ((rstd.double().cpu() - r64).abs() / r64).max().item() / ref.U32
        print(f"RATIO headnorm fwd {DT_IDS[dtype]} {shape} {kind} off={off} alpha={alpha}: out {ref.worst(err, bound):.2f} "
              f"rstd {rerr / ref.e_r(p):.2f} (of E_R = {ref.e_r(p):.1f} u)")
        assert torch.isfinite(out.float()).all()
        assert (err <= bound).all(), ref.worst(err, bound)
        assert rerr <= ref.F * ref.e_r(p)
        # backward: from the kernel's own rstd and saved copy, the factor alpha
        dx, dw = head_rms_norm_backward(gg, saved, rstd, H, wg, *tab, alpha=alpha)
        assert dx.dtype == dtype and dw.dtype == w.dtype and tuple(dw.shape) == (D,)
        dx64, dw64, sx, sw = ref.ref_backward(g, x, H, w, EPS, off, alpha)
        bx = ref.dx_bound(dx64, sx, dtype, p, off is not None, alpha)
        bw = ref.dw_bound(dw64, sw, w.dtype, p, off is not None, alpha, B, R, H)
        ex, ew = (dx.double().cpu() - dx64).abs(), (dw.double().cpu() - dw64).abs()
        print(f"RATIO headnorm bwd {DT_IDS[dtype]} {shape} {kind} off={off} alpha={alpha}: dx {ref.worst(ex, bx):.2f} "
              f"dw {ref.worst(ew, bw):.2f} (K_DW = {ref.k_dw(p, B, R, H)})")
        assert torch.isfinite(dx.float()).all() and torch.isfinite(dw.float()).all()
        assert (ex <= bx).all(), ref.worst(ex, bx)
        assert (ew <= bw).all(), ref.worst(ew, bw)
        # the ordered sum: the same bits again
        dx2, dw2 = head_rms_norm_backward(gg, saved, rstd, H, wg, *tab, alpha=alpha)
        assert torch.equal(dw, dw2) and torch.equal(dx, dx2)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS.get)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels(gpu, dtype, shape):
    """Forward, ``rstd``, the saved copy, ``dx`` and ``dw`` against fp64 under the model's bounds
    (each F = 2 times its unit bound; the RATIO lines print error / unit bound), with and without
    the fused rotation and ``alpha``."""
    _check(gpu, shape, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS.get)
@pytest.mark.parametrize("kind", ["scaled", "zero_rows", "huge"])
def test_inputs(gpu, dtype, kind):
    """``x`` times 200 (fp16 squares would overflow: the sum is fp32), rows of zeros (out is zero,
    everything finite, ``dx = g w / sqrt(eps)`` there) and a head with one huge element."""
    _check(gpu, (2, 63, 8, 96), dtype, kind=kind)
    if kind == "zero_rows":
        from xdot.ops.headnorm import head_rms_norm_apply

        x, _g, w = _inputs((2, 63, 8, 96), dtype, kind=kind)
        out, rstd, _ = head_rms_norm_apply(x.to(gpu), 8, w.to(gpu), EPS)
        assert bool((out[:, ::3] == 0).all()) and bool((rstd[:, ::3] == rstd[0, 0, 0]).all())


@pytest.mark.parametrize("dtype", [BF16, F32], ids=DT_IDS.get)
def test_weight_dtype(gpu, dtype):
    """An fp32 gain beside 16-bit tensors (fp32 master weights): the same bounds; and with the same
    gain values ``dw`` differs from the 16-bit gain's only by the final rounding."""
    from xdot.ops.headnorm import head_rms_norm_apply, head_rms_norm_backward

    shape = (2, 63, 8, 96)
    _check(gpu, shape, dtype, wdtype=F32)
    x, g, w = _inputs(shape, dtype)
    xg, gg = x.to(gpu), g.to(gpu)
    res = []
    for wt in (w.to(gpu), w.float().to(gpu)):
        out, rstd, saved = head_rms_norm_apply(xg, 8, wt, EPS, save=True)
        dx, dw = head_rms_norm_backward(gg, saved, rstd, 8, wt)
        res.append((out, dx, dw))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert res[1][2].dtype == F32 and torch.equal(res[0][2], res[1][2].to(dtype))


@pytest.mark.parametrize("dtype", [BF16, F32], ids=DT_IDS.get)
def test_views(gpu, dtype):
    """Strided views give bitwise the contiguous call's values, forward and backward, and touch
    nothing else; the saved copy is bitwise the input also after an in-place call."""
    import xdot
    from xdot.ops.headnorm import head_rms_norm_apply, head_rms_norm_backward

    B, R, H, D = 2, 37, 4, 48
    C = H * D
    rot = xdot.Rotary()
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(B, R, C, generator=gen).to(gpu, dtype)
    v = torch.randn(B, R, C, generator=gen).to(gpu, dtype)
    g = torch.randn(B, R, C, generator=gen).to(gpu, dtype)
    w = (torch.rand(D, generator=gen) + 0.5).to(gpu, dtype)
    for off in (None, 70):
        tab = (None, None) if off is None else rot.table(R, D, off, gpu)
        want, rstd, _ = head_rms_norm_apply(x, H, w, EPS, *tab, alpha=0.25)
        wdx, wdw = head_rms_norm_backward(g, x, rstd, H, w, *tab, alpha=0.25)

        def same(view, gview):
            """forward in place on ``view``, backward in place on ``gview``"""
            o, r, s = head_rms_norm_apply(view, H, w, EPS, *tab, alpha=0.25, out=view, save=True)
            assert o is view and torch.equal(view, want) and torch.equal(r, rstd) and torch.equal(s, x)
            d, dw = head_rms_norm_backward(gview, s, r, H, w, *tab, alpha=0.25, out=gview)
            assert d is gview and torch.equal(gview, wdx) and torch.equal(dw, wdw)

        # in place on a contiguous tensor
        same(x.clone(), g.clone())
        # the q half of a packed [q | v] buffer
        buf, gbuf = torch.cat([x, v], dim=-1), torch.cat([g, v], dim=-1)
        same(buf[..., :C], gbuf[..., :C])
        assert torch.equal(buf[..., C:], v) and torch.equal(gbuf[..., C:], v)
        # rank slot 1 of a (3, B, R, 2C) gather buffer
        gb = torch.cat([x, v], dim=-1).unsqueeze(0).repeat(3, 1, 1, 1)
        gg = torch.cat([g, v], dim=-1).unsqueeze(0).repeat(3, 1, 1, 1)
        keep = gb.clone()
        same(gb[1][..., :C], gg[1][..., :C])
        assert torch.equal(gb[1][..., C:], v) and torch.equal(gb[0], keep[0]) and torch.equal(gb[2], keep[2])
        # a base pointer one element off the 16-byte grid (the scalar path)
        odd, godd = torch.zeros(B, R, C + 8, device=gpu, dtype=dtype), torch.zeros(B, R, C + 8, device=gpu, dtype=dtype)
        odd[..., 1:1 + C] = x
        godd[..., 1:1 + C] = g
        o, r, _ = head_rms_norm_apply(odd[..., 1:1 + C], H, w, EPS, *tab, alpha=0.25)
        assert torch.equal(o, want) and torch.equal(r, rstd)
        same(odd[..., 1:1 + C], godd[..., 1:1 + C])
        assert bool((odd[..., 0] == 0).all()) and bool((odd[..., 1 + C:] == 0).all())
        assert bool((godd[..., 0] == 0).all()) and bool((godd[..., 1 + C:] == 0).all())
        # into a strided out with a padded batch stride
        dst = torch.full((B, R + 3, C), 7.0, device=gpu, dtype=dtype)
        head_rms_norm_apply(x, H, w, EPS, *tab, alpha=0.25, out=dst[:, :R])
        assert torch.equal(dst[:, :R], want) and bool((dst[:, R:] == 7).all())
    # overlapping but different views are refused
    buf = torch.cat([x, v], dim=-1)
    with pytest.raises(RuntimeError):
        head_rms_norm_apply(buf[..., :C], H, w, EPS, out=buf[..., 8:C + 8])


def test_fused_rotation_is_rope_of_the_norm(gpu):
    """fp32 tensors: norm and rotation in one pass against ``rope_apply`` of the norm's output.  The
    two-pass form rounds ``y`` to the tensor's dtype in between, which in fp32 is what the one pass
    holds in registers: at most that one rounding (2^-23 of the pair norm) apart."""
    import xdot
    from xdot.ops.headnorm import head_rms_norm_apply
    from xdot.ops.rope import rope_apply

    B, R, H, D = 2, 63, 8, 96
    rot = xdot.Rotary()
    x, _g, w = _inputs((B, R, H, D), F32)
    x, w = x.to(gpu), w.to(gpu)
    tab = rot.table(R, D, 1000, gpu)
    for wt in (torch.ones_like(w), w):
        for alpha in (1.0, 0.1803):
            one, _, _ = head_rms_norm_apply(x, H, wt, EPS, *tab, alpha=alpha)
            y, _, _ = head_rms_norm_apply(x, H, wt, EPS)
            two = rope_apply(y, H, *tab, alpha=alpha)
            yv = y.view(B, R, H, D)
            hyp = torch.hypot(yv[..., :D // 2], yv[..., D // 2:])
            hyp = torch.cat([hyp, hyp], -1).reshape(B, R, H * D)
            diff = (one - two).abs()
            print(f"fused rotation alpha={alpha}: bitwise {torch.equal(one, two)}, "
                  f"max diff / (alpha hypot) {(diff / (alpha * hyp)).max().item():.2e}")
            assert (diff <= 2.0 ** -23 * alpha * hyp).all()


def test_autograd_matches_raw(gpu):
    """``xdot.head_rms_norm`` (new tensor, in place, packed) is the raw forward / backward pair."""
    import xdot
    from xdot.ops.headnorm import head_rms_norm_apply, head_rms_norm_backward, norm_packed

    B, R, H, D = 2, 33, 2, 96
    rot = xdot.Rotary()
    x, g, w = _inputs((B, R, H, D), BF16)
    x, g, w = x.to(gpu), g.to(gpu), w.to(gpu)
    tab = rot.table(R, D, 9, gpu)
    want, rstd, _ = head_rms_norm_apply(x, H, w, EPS, *tab, alpha=0.5)
    wdx, wdw = head_rms_norm_backward(g, x, rstd, H, w, *tab, alpha=0.5)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    xdot.head_rms_norm(xr, H, wr, EPS, rotary=rot, offset=9, alpha=0.5).backward(g)
    assert torch.equal(xr.grad, wdx) and torch.equal(wr.grad, wdw)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = xr * 1.0
    out = xdot.head_rms_norm(y, H, wr, EPS, rotary=rot, offset=9, alpha=0.5, out=y)
    assert torch.equal(out, want)
    out.backward(g)
    assert torch.equal(xr.grad, wdx) and torch.equal(wr.grad, wdw)
    v = torch.randn(B, R, 64, device=gpu).to(BF16)
    qv = torch.cat([x, v], -1).requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    out = norm_packed(qv, H * D, H, wr, EPS, rot, 9, alpha=0.5, bwd_alpha=1.0)
    assert torch.equal(out[..., :H * D], want) and torch.equal(out[..., H * D:], v)
    out.backward(torch.cat([g, v], -1))
    dx1, dw1 = head_rms_norm_backward(g, x, rstd, H, w, *tab, alpha=1.0)
    assert torch.equal(qv.grad[..., :H * D], dx1) and torch.equal(qv.grad[..., H * D:], v) and torch.equal(wr.grad, dw1)


# ---------------------------------------------------------------------------------- module
def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()


def _step(m, x, mask):
    x = x.detach().clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    out = m(x, x, x, mask)
    out.float().pow(2).mean().backward()
    torch.cuda.synchronize()
    return out.detach(), x.grad, {n: p.grad for n, p in m.named_parameters()}


def _errors(got, want):
    """As ``tests/test_rope_gpu.py``: relative Frobenius error per tensor, ``queries.bias`` against
    the keys bias gradient's norm."""
    (o, dx, gp), (ro, rdx, rgp) = got, want
    e = {"out": _rel(o, ro), "dx": _rel(dx, rdx)}
    for n, gr in gp.items():
        if n == "queries.bias":
            e[n] = ((gr.double() - rgp[n]).norm() / rgp["keys.bias"].norm()).item()
        else:
            e[n] = _rel(gr, rgp[n])
    return e


def _set_gains(m, seed=5):
    """Gains away from their initial ones, so that a missing or misplaced gain shows: uniform in
    [0.3, 0.8].  The norm fixes the logits' scale at the product of the two gains; these (rms 0.57)
    give the logits the scale they have in the same module without the norm, whose default
    projections of N(0, 1) inputs have rms 1 / sqrt 3 = 0.58.  The bf16 tests below take that
    module's error on the same inputs as their yardstick, which says something only in the same
    softmax regime: the module WITHOUT the norm whose ``keys`` / ``queries`` weights are scaled by
    sqrt 3 (unit-rms k and q, as gains of 1 give) has itself 1.6x the yardstick's ``dx`` error
    (5.2e-3 against 3.2e-3; with the norm and gains of 1: 5.1e-3).  ``profiles/qk_norm.md`` has
    the table."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n in ("keys_norm", "queries_norm"):
            wt = getattr(m, n).weight
            wt.copy_((torch.rand(wt.shape, generator=gen) * 0.5 + 0.3).to(wt))


def _module(gpu, dtype, key_dim, H, impl, bias, norm, rope=True, Hg=None, gains="drawn", **kw):
    """``gains``: 'drawn' (:func:`_set_gains`) or 'init' (the ones a user's new module has)."""
    import xdot

    torch.manual_seed(0)
    m = xdot.DistributedDotProductAttn(key_dim, num_heads=H, impl=impl, add_bias=bias, qk_norm=norm,
                                       rope=xdot.Rotary() if rope else None, num_gathered_heads=Hg, **kw).to(gpu, dtype)
    if norm and gains == "drawn":
        _set_gains(m)
    return m


def test_module_exact_fp32(gpu):
    """Exact fp32 family, D = 96, R = T = 160, causal, rope: forward and all gradients, the two
    gains' included, within the 2e-6 relative Frobenius error ``tests/test_rope_gpu.py`` holds the
    same configuration to."""
    import xdot

    m = _module(gpu, F32, 192, 2, "flash", False, True)
    x = torch.randn(1, 160, 192, generator=torch.Generator().manual_seed(1)).to(gpu)
    spec = xdot.StructuredMask(causal=True)
    e = _errors(_step(m, x, spec), ref.dense_run(m, x, spec.dense(1, 160, 160, 0, gpu)))
    print("qk_norm exact fp32 module errors:", {k: f"{v:.2e}" for k, v in e.items()})
    assert "keys_norm.weight" in e and "queries_norm.weight" in e
    for k, v in e.items():
        assert v <= 2e-6, (k, v)


BF16_CASES = {
    "fused": dict(key_dim=768, H=8, impl="flash", fused=True, bias=False),
    "per_op": dict(key_dim=768, H=8, impl="flash", fused=False, bias=False),
    "bias": dict(key_dim=768, H=8, impl="flash", fused=True, bias=True),
    "padded": dict(key_dim=80, H=2, impl="flash", fused=True, bias=False),
    "wide": dict(key_dim=320, H=2, impl="flash", fused=True, bias=False),
    "ring": dict(key_dim=768, H=8, impl="ring", fused=True, bias=False),
    "gqa": dict(key_dim=768, H=8, impl="flash", fused=True, bias=False, Hg=2),
}


def _bf16_runs(gpu, c, T=320):
    """Errors against the dense fp64 reference of each, same inputs: with QK-norm and rope, with
    rope alone (the module before QK-norm existed), and with neither."""
    import xdot

    spec = xdot.StructuredMask(causal=True)
    res = []
    for norm, rope in ((True, True), (False, True), (False, False)):
        m = _module(gpu, BF16, c["key_dim"], c["H"], c["impl"], c["bias"], norm, rope, c.get("Hg"))
        x = torch.randn(1, T, c["key_dim"], generator=torch.Generator().manual_seed(1)).to(gpu, BF16)
        want = ref.dense_run(m, x, spec.dense(1, T, T, 0, gpu), rope=rope)
        res.append(_errors(_step(m, x, spec), want))
    return res


@pytest.mark.parametrize("case", list(BF16_CASES))
def test_module_bf16(gpu, case, monkeypatch):
    """The bound of ``tests/test_rope_gpu.py`` for the same configurations: every tensor's error
    against its fp64 reference at most 1.5x that of the module with neither rope nor norm on the same
    inputs (``queries.bias``: the absolute 3e-2 of the keys bias gradient's norm).  The two gain
    gradients have no counterpart there: they are held to the largest error any projection weight's
    gradient is allowed in the same run."""
    from xdot.utils.env import FLAGS

    c = BF16_CASES[case]
    monkeypatch.setattr(FLAGS, "fused_module", c["fused"])
    normed, roped, plain = _bf16_runs(gpu, c)
    for k in normed:
        print(f"qk_norm bf16 [{case}] {k}: norm+rope {normed[k]:.3e}  rope {roped.get(k, float('nan')):.3e}  "
              f"none {plain.get(k, float('nan')):.3e}")
    wmax = max(v for k, v in plain.items() if k.endswith(".weight"))
    for k in normed:
        if k == "queries.bias":
            assert normed[k] <= 3e-2, (k, normed[k])
        elif k in plain:
            assert normed[k] <= 1.5 * plain[k], (k, normed[k], plain[k])
        else:
            assert normed[k] <= 1.5 * wmax, (k, normed[k], wmax)


@pytest.mark.parametrize("case", list(BF16_CASES))
def test_module_bf16_initial_gains(gpu, case, monkeypatch):
    """The module as a user builds it: gains of 1, so unit-rms ``k`` and ``q`` and logits sqrt 3 x
    sqrt 3 times those of the module without the norm.  Its yardstick is that module in the same
    regime: ``qk_norm=False`` on the same inputs with the ``keys`` / ``queries`` weights (and biases)
    scaled by sqrt 3, whose ``k`` and ``q`` have unit rms too, against ITS fp64 reference.  Every
    tensor's error at most 1.5x that; ``queries.bias`` and the two gains' gradients as
    :func:`test_module_bf16`."""
    import xdot
    from xdot.utils.env import FLAGS

    c = BF16_CASES[case]
    monkeypatch.setattr(FLAGS, "fused_module", c["fused"])
    spec = xdot.StructuredMask(causal=True)
    T = 320
    x = torch.randn(1, T, c["key_dim"], generator=torch.Generator().manual_seed(1)).to(gpu, BF16)
    res = []
    for norm in (True, False):
        m = _module(gpu, BF16, c["key_dim"], c["H"], c["impl"], c["bias"], norm, True, c.get("Hg"), gains="init")
        if norm:
            assert bool((m.keys_norm.weight == 1).all()) and bool((m.queries_norm.weight == 1).all())
        else:
            with torch.no_grad():
                for lin in (m.keys, m.queries):
                    lin.weight.mul_(3 ** 0.5)
                    if lin.bias is not None:
                        lin.bias.mul_(3 ** 0.5)
        want = ref.dense_run(m, x, spec.dense(1, T, T, 0, gpu), rope=True)
        res.append(_errors(_step(m, x, spec), want))
    normed, scaled = res
    for k in normed:
        print(f"qk_norm bf16 gains=1 [{case}] {k}: norm+rope {normed[k]:.3e}  rope, W x sqrt3 {scaled.get(k, float('nan')):.3e}")
    wmax = max(v for k, v in scaled.items() if k.endswith(".weight"))
    for k in normed:
        if k == "queries.bias":
            assert normed[k] <= 3e-2, (k, normed[k])
        elif k in scaled:
            assert normed[k] <= 1.5 * scaled[k], (k, normed[k], scaled[k])
        else:
            assert normed[k] <= 1.5 * wmax, (k, normed[k], wmax)


def test_emulated_middle_rank(gpu, monkeypatch):
    """Rank 1 of N = 4 (R = 96, bf16, two gather chunks) with a communicator replaying the real
    peers' normalised, rotated blocks, against rows [96, 192) of the whole sequence's dense fp64
    reference: within 1.5x the same rank's error without norm and rope, as
    ``tests/test_rope_gpu.py``."""
    import xdot
    from xdot.ops import flash
    from xdot.utils.comm import EmulatedComm
    from xdot.utils.env import FLAGS

    N, RANK, R, dim, H = 4, 1, 96, 192, 2
    monkeypatch.setattr(FLAGS, "gather_chunks", 2)
    monkeypatch.setattr(FLAGS, "fused_module", True)
    flash.MASK_CACHE.clear()
    spec = xdot.StructuredMask(causal=True)
    x = torch.randn(1, N * R, dim, generator=torch.Generator().manual_seed(1)).to(gpu, BF16)
    rows = slice(RANK * R, (RANK + 1) * R)

    class Replay(EmulatedComm):
        def __init__(self, peers):
            super().__init__(N, rank=RANK)
            self.peers, self.row = peers, 0

        def all_gather_into(self, out, inp, async_op=False):
            rc = inp.shape[1]
            r0 = self.row % R
            self.row += rc
            h = super().all_gather_into(out, inp, async_op=async_op)
            if h is not None:
                h.wait()
            ov = out.view(N, 1, rc, -1)
            for j in range(N):
                if j != RANK:
                    ov[j].copy_(self.peers[:, j * R + r0:j * R + r0 + rc])
            return h

    errs = []
    for norm in (True, False):
        whole = _module(gpu, BF16, dim, H, "flash", False, norm, norm)
        with torch.no_grad():  # the gathered side of the whole sequence, from the module's own pieces
            qv = whole._project_qv(x, x)
            if norm:
                q = qv[..., :dim]
                xdot.head_rms_norm(q, H, whole.queries_norm.weight, whole.qk_norm_eps, rotary=whole.rope, offset=0, out=q)
        m = _module(gpu, BF16, dim, H, "flash", False, norm, norm, chunk_plan=2, comm=Replay(qv))
        want = ref.dense_run(whole, x, spec.dense(1, N * R, N * R, 0, gpu), rope=norm)
        with torch.no_grad():
            out = m(x[:, rows], x[:, rows], x[:, rows], spec)
        errs.append(_rel(out, want[0][:, rows]))
    print(f"qk_norm bf16 emulated rank 1/4 out: norm+rope {errs[0]:.3e}  none {errs[1]:.3e}")
    assert errs[1] <= 2e-2
    assert errs[0] <= 1.5 * errs[1]


def test_graph_capture(gpu, monkeypatch):
    """A ``GraphedStep`` capture of a training step with ``qk_norm`` and ``rope``: 2 eager warm-up
    steps and 2 replays equal 4 eager steps bitwise, and the gains move: the norm passes are
    capturable and deterministic.  (It does not say that the DEFAULT eager configuration equals a
    replay bit for bit: as for the module without the norm, it does not.)  Both runs take the
    configuration a capture runs in -- a capturable optimizer and the weight gradients on the main
    stream (``XDOT_WGRAD_SIDE=0``: under capture the one-node module has no side stream and forms
    both projections' weight gradients in one launch, another order of summation than the eager
    default's) -- so that eager and replayed steps differ in nothing but the graph."""
    import xdot
    from xdot.utils.env import FLAGS
    from xdot.utils.graphs import GraphedStep

    monkeypatch.setattr(FLAGS, "wgrad_side", False)

    def train(graphed, steps=4, warmup=2):
        torch.manual_seed(0)
        m = xdot.DistributedDotProductAttn(256, num_heads=4, impl="flash", rope=xdot.Rotary(), qk_norm=True).to(gpu, BF16)
        # (lr: an AdamW step of 1e-3 would round back to the bf16 gains' initial 1.0, half an ulp below which is 2e-3)
        opt = xdot.FusedAdamW(m.parameters(), lr=1e-2, capturable=True)
        crit = xdot.MSELoss()
        gen = torch.Generator(device=gpu).manual_seed(1)
        x = torch.rand(1, 256, 256, device=gpu, dtype=BF16, generator=gen)
        y = torch.rand(1, 256, 256, device=gpu, dtype=BF16, generator=gen)
        spec = xdot.StructuredMask(causal=True)

        def body():
            loss = crit(m(x, x, x, spec), y)
            loss.backward()
            opt.step()
            return loss

        losses = []
        if graphed:
            st = GraphedStep(body, zero_grad=opt.zero_grad, warmup=warmup)
            for _ in range(steps - warmup):
                losses.append(st().float().item())
        else:
            for i in range(steps):
                opt.zero_grad(set_to_none=True)
                l = body().float().item()
                if i >= warmup:
                    losses.append(l)
        torch.cuda.synchronize()
        return losses, {n: p.detach().clone() for n, p in m.named_parameters()}

    le, pe = train(False)
    lg, pg = train(True)
    assert len(le) == len(lg) == 2 and math.isfinite(lg[-1])
    for n in pe:
        d = (pe[n].float() - pg[n].float()).abs().max().item()
        print(f"graph capture {n}: max |eager - graphed| {d:.3e}")
    assert le == lg, (le, lg)
    for n in pe:
        assert torch.equal(pe[n], pg[n]), n
    for n in ("keys_norm.weight", "queries_norm.weight"):
        assert not torch.equal(pg[n], torch.ones_like(pg[n]))


class _Counting:
    """``torch.ops.xdot`` with every op call counted by name."""

    def __init__(self, ops):
        self._ops, self.calls = ops, {}

    def __getattr__(self, name):
        op = getattr(self._ops, name)

        def call(*a, **k):
            self.calls[name] = self.calls.get(name, 0) + 1
            return op(*a, **k)

        return call


@pytest.mark.parametrize("rope", [True, False])
def test_launch_accounting(gpu, rope, monkeypatch):
    """One step of the one-node module, counted as calls of the ``torch.ops.xdot`` ops (not kernel
    launches: ``headnorm_fwd`` launches once per call, ``headnorm_bwd`` twice, the pass and the
    ordered ``dw`` sum): two norm passes forward and two backward, no ``rope_apply``
    at all (the rotation rides in them); without ``qk_norm`` the node calls what it called before."""
    from xdot import _ext
    from xdot.utils.env import FLAGS

    monkeypatch.setattr(FLAGS, "fused_module", True)
    x = torch.randn(1, 200, 192, device=gpu).to(BF16).requires_grad_(True)
    counts = {}
    for norm in (True, False):
        m = _module(gpu, BF16, 192, 2, "flash", False, norm, rope)
        m(x, x, x, None).float().sum().backward()  # (tables and packed weights built outside the count)
        c = _Counting(_ext.ops())
        with monkeypatch.context() as mp:
            mp.setattr(_ext, "ops", lambda c=c: c)
            out = m(x, x, x, None)
            fwd = dict(c.calls)
            out.float().sum().backward()
            torch.cuda.synchronize()
        counts[norm] = (fwd, dict(c.calls))
    fwd, both = counts[True]
    assert fwd.get("headnorm_fwd") == 2 and "rope_apply" not in both and both.get("headnorm_bwd") == 2, both
    fwd0, both0 = counts[False]
    assert "headnorm_fwd" not in both0 and "headnorm_bwd" not in both0
    assert fwd0.get("rope_apply", 0) == (2 if rope else 0) and both0.get("rope_apply", 0) == (4 if rope else 0)
    # nothing else changed: the same ops, the same number of times
    strip = lambda d: {k: v for k, v in d.items() if k not in ("headnorm_fwd", "headnorm_bwd", "rope_apply")}
    assert strip(both) == strip(both0), (both, both0)
