"""Grouped-query attention on the GPU (``Hg`` gathered heads < ``H`` row heads): the 16-bit flash
kernels against an fp32 torch reference with the gathered heads repeated, bitwise against the same
call on operands expanded to ``H`` heads, the column kernel's row splits and output modes, the
module (fused node, per-op graph, ring, the families that expand after the gather), an emulated
middle rank, the expanding families' flash and ring paths on three ranks, and a HIP-graph captured step."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, R, N, Rc, H, Hg, D)
CASES = [
    (1, 130, 1, 200, 4, 2, 96),   # 3 row tiles per head (the head switch lands on an odd ring stage), T % 128 != 0,
                                  # the pipelined column kernel when pre-scaled
    (2, 200, 3, 70, 4, 1, 128),   # multi-query; the plain column kernel; B = 2
    (1, 77, 2, 100, 6, 2, 32),    # G = 3; R < 128
    (1, 300, 1, 256, 8, 2, 64),   # G = 4
]


def _close(what, a, b, fro, elem=10.0):
    """tests/test_flash_gpu.py's criterion: rel. Frobenius error <= fro, and |a - b| <= elem * fro *
    (|b| + 0.25 rms(b)) everywhere."""
    a, b = a.float(), b.float()
    assert torch.isfinite(a).all(), f"{what}: non-finite"
    err = ((a - b).norm() / b.norm().clamp_min(1e-12)).item()
    assert err <= fro, f"{what}: relative Frobenius error {err:.3e} > {fro:.1e}"
    rms = b.pow(2).mean().sqrt()
    bound = elem * fro * (b.abs() + 0.25 * rms)
    worst = ((a - b).abs() / bound).max().item()
    assert worst <= 1.0, f"{what}: an element is {worst:.2f}x past its bound"


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _inputs(case, dt, gpu, mask_kind):
    """-> rows (B, R, H*D), kc / vc (B, T, Hg*D) in gathered (rank-major rows) order, do, mask"""
    B, R, N, Rc, H, Hg, D = case
    T = N * Rc
    g = torch.Generator(device="cpu").manual_seed(sum(case))
    rows = torch.randn(B, R, H * D, generator=g).to(gpu, dt)
    kc = torch.randn(B, T, Hg * D, generator=g).to(gpu, dt)
    vc = torch.randn(B, T, Hg * D, generator=g).to(gpu, dt)
    do = torch.randn(B, R, H * D, generator=g).to(gpu, dt)
    mask = None
    if mask_kind == "random":
        mask = torch.rand(B, R, T, generator=g) < 0.4
    elif mask_kind == "blocks":
        mask = torch.zeros(B, R, T, dtype=torch.bool)
        mask[:, :, : min(T, 128)] = True           # fully masked tiles
        r1 = min(R, 90)
        mask[:, 40:r1, 128:] = torch.rand(B, r1 - 40, max(0, T - 128), generator=g) < 0.5
    if mask is not None:
        mask[..., T - 1] = False                   # keep every row alive
        mask = mask.to(gpu)
    return rows, kc, vc, do, mask


def _expand(x, Hg, G):
    """(B, T, Hg*D) -> (B, T, Hg*G*D) contiguous: every gathered head repeated for its group"""
    B, T, C = x.shape
    return x.view(B, T, Hg, 1, C // Hg).expand(B, T, Hg, G, C // Hg).reshape(B, T, Hg * G * (C // Hg)).contiguous()


def _ref(rows, kc, vc, do, mask, H, Hg, scale):
    """fp32 torch reference with repeated heads -> out, lse, d rows, d kc, d vc (the group sums)"""
    B, R, C = rows.shape
    T, D = kc.shape[1], C // H
    k = rows.float().view(B, R, H, D).transpose(1, 2).clone().requires_grad_(True)
    q = kc.float().clone().requires_grad_(True)
    v = vc.float().clone().requires_grad_(True)
    qh = q.view(B, T, Hg, D).transpose(1, 2).repeat_interleave(H // Hg, dim=1)
    vh = v.view(B, T, Hg, D).transpose(1, 2).repeat_interleave(H // Hg, dim=1)
    s = (k @ qh.transpose(-1, -2)) * scale
    if mask is not None:
        s = s.masked_fill(mask.unsqueeze(1), -float("inf"))
    o = (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, R, C)
    o.backward(do.float())
    return o.detach(), torch.logsumexp(s, -1).detach(), k.grad.transpose(1, 2).reshape(B, R, C), q.grad, v.grad


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("mask_kind", ["none", "random", "blocks"])
@pytest.mark.parametrize("prescaled", [False, True])
def test_kernels_match_reference(gpu, dt, case, mask_kind, prescaled):
    from xdot.ops import flash

    B, R, N, Rc, H, Hg, D = case
    T = N * Rc
    rows, kc, vc, do, mask = _inputs(case, dt, gpu, mask_kind)
    scale = 1.0 / math.sqrt(D)
    mk = flash.prepare_mask(mask, B, R, T)
    rk = flash.prescale(rows, scale) if prescaled else rows
    out, lse = flash.fwd(rk, kc, vc, mk, H, scale, prescaled=prescaled, Hg=Hg)
    ref_o, ref_lse, dk_ref, dq_ref, dv_ref = _ref(rows, kc, vc, do, mask, H, Hg, scale)
    fro = 1e-2 if dt == torch.bfloat16 else 3e-3
    _close("fwd out", out, ref_o, fro)
    assert (lse - ref_lse).abs().max().item() < 1e-2, "lse"
    drows, dkc, dvc = flash.bwd(do, rk, kc, vc, out, lse, mk, H, scale, prescaled=prescaled, Hg=Hg)
    assert dkc.shape == kc.shape and dvc.shape == vc.shape and dkc.dtype == torch.float32
    gfro = 1.5e-2 if dt == torch.bfloat16 else 4e-3
    _close("d rows", drows, dk_ref, gfro)
    _close("d cols (q)", dkc, dq_ref, gfro)
    _close("d cols (v)", dvc, dv_ref, gfro)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("prescaled", [False, True])
def test_row_side_bitwise_equals_expanded(gpu, case, prescaled):
    """Per (b, h) the row-block kernels do the same arithmetic whether gathered head h // G is read
    in place or from a repeated copy, and the split plan depends on H only: out, lse, d rows, the
    partial-slot forward + combine and the partial row-side backward + sum are bitwise equal."""
    from xdot.ops import flash

    B, R, N, Rc, H, Hg, D = case
    T, G, dt = N * Rc, H // Hg, torch.bfloat16
    rows, kc, vc, do, mask = _inputs(case, dt, gpu, "random")
    ke, ve = _expand(kc, Hg, G), _expand(vc, Hg, G)
    scale = 1.0 / math.sqrt(D)
    mk = flash.prepare_mask(mask, B, R, T)
    rk = flash.prescale(rows, scale) if prescaled else rows
    for nsplit in (0, 3):
        out, lse = flash.fwd(rk, kc, vc, mk, H, scale, nsplit=nsplit, prescaled=prescaled, Hg=Hg)
        oute, lsee = flash.fwd(rk, ke, ve, mk, H, scale, nsplit=nsplit, prescaled=prescaled)
        assert torch.equal(out, oute) and torch.equal(lse, lsee), f"forward, nsplit {nsplit}"
    delta = flash.bwd_delta(do, out, H)
    for nsplit in (0, 3):
        d = flash.bwd_rows(do, rk, kc, vc, lse, delta, mk, H, scale, nsplit=nsplit, prescaled=prescaled, Hg=Hg)
        de = flash.bwd_rows(do, rk, ke, ve, lse, delta, mk, H, scale, nsplit=nsplit, prescaled=prescaled)
        assert torch.equal(d, de), f"d rows, nsplit {nsplit}"
    ns = 3

    def partial(k_, v_, hg):
        opart = torch.empty(ns, B, R, H * D, dtype=torch.float32, device=gpu)
        lpart = torch.empty(ns, B, H, R, dtype=torch.float32, device=gpu)
        flash.fwd_partial(rk, k_, v_, mk, H, scale, opart, lpart, 0, ns, prescaled, 0, hg)
        o, l = flash.fwd_combine(opart, lpart, H, rows)
        dpart = torch.empty(ns, B, R, H * D, dtype=torch.float32, device=gpu)
        flash.bwd_rows_partial(do, rk, k_, v_, lse, delta, mk, H, scale, dpart, 0, ns, prescaled, 0, hg)
        return o, l, flash.bwd_rows_sum(dpart, H, rows)

    for a, b in zip(partial(kc, vc, Hg), partial(ke, ve, None)):
        assert torch.equal(a, b)


def test_default_argument_is_bitwise_todays(gpu):
    """Every op called with ``Hg=H`` gives bit for bit what it gives without the argument."""
    from xdot.ops import flash

    case = (1, 200, 1, 200, 4, 4, 64)
    B, R, N, Rc, H, Hg, D = case
    rows, kc, vc, do, mask = _inputs(case, torch.bfloat16, gpu, "random")
    scale, mk = 0.125, flash.prepare_mask(mask, B, R, R)
    rk = flash.prescale(rows, scale)
    res = []
    for hg in (None, H):
        kw = {} if hg is None else {"Hg": hg}
        out, lse = flash.fwd(rk, kc, vc, mk, H, scale, prescaled=True, **kw)
        drows, dq, dv = flash.bwd(do, rk, kc, vc, out, lse, mk, H, scale, prescaled=True, **kw)
        dkv16, delta = flash.bwd_cols(do, rk, kc, vc, out, lse, mk, H, scale, fp32_out=False, prescaled=True, **kw)
        plain, _ = flash.bwd_cols(do, rows, kc, vc, out, lse, mk, H, scale, **kw)  # (the plain column kernel)
        opart = torch.empty(2, B, R, H * D, dtype=torch.float32, device=gpu)
        lpart = torch.empty(2, B, H, R, dtype=torch.float32, device=gpu)
        flash.fwd_partial(rk, kc, vc, mk, H, scale, opart, lpart, 0, 2, True, 0, *kw.values())
        dpart = torch.empty(2, B, R, H * D, dtype=torch.float32, device=gpu)
        flash.bwd_rows_partial(do, rk, kc, vc, lse, delta, mk, H, scale, dpart, 0, 2, True, 0, *kw.values())
        res.append((out, lse, drows, dq, dv, dkv16, plain, opart, lpart, dpart))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("case", [CASES[0], CASES[3]])
def test_column_side_splits_modes_and_determinism(gpu, monkeypatch, case):
    """The gathered-side kernel: two runs are bitwise equal; row splits of the concatenated sweep of
    G * NRT tiles (XDOT_CSPLIT 2 and 4; pieces start on even tiles, the ring stage being the tile's
    parity) stay within the reference bounds.  First case, 2 x 3 tiles: 2 pieces cut inside head 0
    (tiles [0, 2) and [2, 6)), 4 do not fit 3 tile pairs and run unsplit.  Last case, 4 x 5 tiles: 2
    pieces cut on the boundary of heads 1 and 2 (tile 10), 4 pieces inside heads as well (4, 10, 14).
    Also the input-dtype output and the packed (B, T, 2 * Hg * D) layout."""
    from xdot.ops import flash

    B, R, N, Rc, H, Hg, D = case
    T, dt = N * Rc, torch.bfloat16
    rows, kc, vc, do, mask = _inputs(case, dt, gpu, "blocks")
    scale = 1.0 / math.sqrt(D)
    mk = flash.prepare_mask(mask, B, R, T)
    rk = flash.prescale(rows, scale)
    fwd = {ps: flash.fwd(rk if ps else rows, kc, vc, mk, H, scale, prescaled=ps, Hg=Hg) for ps in (True, False)}
    _, _, _, dq_ref, dv_ref = _ref(rows, kc, vc, do, mask, H, Hg, scale)

    def cols(fp32_out, ps=True):
        return flash.bwd_cols(do, rk if ps else rows, kc, vc, *fwd[ps], mk, H, scale, fp32_out=fp32_out, prescaled=ps,
                              Hg=Hg)[0]

    monkeypatch.setenv("XDOT_CSPLIT", "1")
    base32 = cols(True)
    assert base32.shape == (B, T, 2 * Hg * D) and base32.is_contiguous()
    for ps in (True, False):
        assert torch.equal(cols(True, ps), cols(True, ps)) and torch.equal(cols(False, ps), cols(False, ps))
    gfro = 1.5e-2
    for s in ("1", "2", "4"):
        monkeypatch.setenv("XDOT_CSPLIT", s)
        for ps in (True, False):  # (the plain kernel takes no row splits: its run covers fp32_out / 16-bit)
            g32, g16 = cols(True, ps), cols(False, ps)
            assert g16.dtype == dt and g32.dtype == torch.float32 and g16.shape == g32.shape == base32.shape
            for what, g_ in (("fp32", g32), ("16-bit", g16)):
                _close(f"splits {s} ps {ps} {what} d cols (q)", g_[..., :Hg * D], dq_ref, gfro)
                _close(f"splits {s} ps {ps} {what} d cols (v)", g_[..., Hg * D:], dv_ref, gfro)
        r32 = _rel(cols(True), base32)
        assert r32 <= 1e-5, f"splits {s}: fp32 out vs unsplit {r32:.2e}"  # another order of the same products


def test_bindings_refuse_bad_groups(gpu):
    from xdot.ops import flash

    rows = torch.randn(1, 64, 4 * 64, device=gpu, dtype=torch.bfloat16)
    kc = torch.randn(1, 64, 2 * 64, device=gpu, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="multiple of the gathered heads"):
        flash.fwd(rows, kc, kc, None, 4, 0.125, Hg=3)
    with pytest.raises(RuntimeError, match="columns"):
        flash.fwd(rows, kc, kc, None, 4, 0.125)            # Hg * D columns, but no Hg given
    with pytest.raises(RuntimeError, match="columns"):
        flash.fwd(rows, kc, kc, None, 4, 0.125, Hg=1)
    out, lse = flash.fwd(rows, kc, kc, None, 4, 0.125, Hg=2)
    wrong = torch.empty(1, 64, 2 * 4 * 64, device=gpu, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="dkv_out"):
        flash.bwd_cols(rows, rows, kc, kc, out, lse, None, 4, 0.125, out_dkv=wrong, Hg=2)
    with pytest.raises(RuntimeError, match="16-bit"):
        flash.fwd(rows.float(), kc.float(), kc.float(), None, 4, 0.125, Hg=2)


# ---- module ------------------------------------------------------------------------------------------
def _step(m, x, mask):
    x = x.detach().clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    out = m(x, x, x, mask)
    out.float().pow(2).mean().backward()
    torch.cuda.synchronize()
    return out.detach(), x.grad, {n: p.grad for n, p in m.named_parameters()}


def _fp64_twin(m, gpu, **kw):
    """The single-device fp64 module (torch ops only) with ``m``'s parameters."""
    import xdot

    ref = xdot.DistributedDotProductAttn(m.keys.in_features, num_heads=m.num_heads, num_gathered_heads=m.num_gathered_heads,
                                         add_bias=m.keys.bias is not None, distributed=False, impl="materialized",
                                         backend="torch", **kw).to(gpu, torch.float64)
    ref.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    return ref


def _errors(got, ref):
    """As tests/test_rope_gpu.py: relative Frobenius error per tensor; ``queries.bias`` against the
    keys bias gradient's norm."""
    (o, dx, gp), (ro, rdx, rgp) = got, ref
    e = {"out": _rel(o, ro), "dx": _rel(dx, rdx)}
    for n, gr in gp.items():
        if n == "queries.bias":
            e[n] = ((gr.double() - rgp[n]).norm() / rgp["keys.bias"].norm()).item()
        else:
            e[n] = _rel(gr, rgp[n])
    return e


@pytest.mark.parametrize("impl,fused", [("flash", True), ("flash", False), ("ring", True)])
def test_module_bf16(gpu, impl, fused, monkeypatch):
    """H = 8, Hg = 2, head dim 64, R = T = 200, causal StructuredMask, bf16, with rope, against the
    fp64 single-device module.  Bounds as tests/test_rope_gpu.py::test_module_bf16: every tensor's
    error with rope at most 1.5x the same module's error without rope (its yardstick), and
    ``queries.bias`` within 3e-2 of the keys bias gradient's norm; the run without rope must itself
    be within tests/test_module_gpu.py's bf16 bounds (output 2e-2, gradients 3e-2), so the yardstick
    cannot drift."""
    import xdot
    from xdot.utils.comm import LocalComm, use_comm
    from xdot.utils.env import FLAGS

    monkeypatch.setattr(FLAGS, "fused_module", fused)
    spec = xdot.StructuredMask(causal=True)
    res = []
    with use_comm(LocalComm()):
        for rope in (xdot.Rotary(), None):
            torch.manual_seed(0)
            m = xdot.DistributedDotProductAttn(512, num_heads=8, num_gathered_heads=2, impl=impl, add_bias=True,
                                               rope=rope).to(gpu, torch.bfloat16)
            x = torch.randn(1, 200, 512, generator=torch.Generator().manual_seed(1)).to(gpu, torch.bfloat16)
            ref = _fp64_twin(m, gpu, rope=rope)
            res.append(_errors(_step(m, x, spec), _step(ref, x.double(), spec.dense(1, 200, 200, 0, gpu))))
    with_rope, without = res
    for k in with_rope:
        print(f"gqa bf16 [{impl} fused={fused}] {k}: rope {with_rope[k]:.3e}  none {without[k]:.3e}")
    for k in with_rope:
        assert without[k] <= (2e-2 if k == "out" else 3e-2), (k, without[k])
        if k == "queries.bias":
            assert with_rope[k] <= 3e-2, (k, with_rope[k])
        else:
            assert with_rope[k] <= 1.5 * without[k], (k, with_rope[k], without[k])


@pytest.mark.parametrize("family", ["exact_fp32", "wide_bf16"])
def test_module_families_that_expand(gpu, family):
    """Exact fp32 (D = 64) and the wide bf16 heads (D = 160) have no grouped kernel: the gathered heads
    are repeated after the gather and the gradients folded before the reduce-scatter.  H = 4, Hg = 2,
    R = T = 200 against the fp64 module, with the module-level bounds of tests/test_flash_f32_gpu.py
    (out 1e-5, gradients 1e-4) and tests/test_flash_wide_gpu.py (2e-2, gradients 10x); the buffer
    kept for the backward stays 2 * Hg * D wide."""
    import xdot
    from xdot.parallel import attention as pa
    from xdot.utils.comm import LocalComm, use_comm

    D, dtype, tol, gtol = (64, torch.float32, 1e-5, 1e-4) if family == "exact_fp32" else (160, torch.bfloat16, 2e-2, 2e-1)
    H, Hg, T = 4, 2, 200
    saved = []
    orig = pa.SeqParallelAttention.forward

    def spy(ctx, *a, **k):
        o = orig(ctx, *a, **k)
        saved.append([tuple(t.shape) for t in ctx.saved_tensors] if hasattr(ctx, "saved_tensors") else None)
        spy.ctx = ctx
        return o

    torch.manual_seed(0)
    with use_comm(LocalComm()):
        m = xdot.DistributedDotProductAttn(H * D, num_heads=H, num_gathered_heads=Hg, impl="flash", add_bias=True).to(gpu, dtype)
        x = torch.randn(1, T, H * D, generator=torch.Generator().manual_seed(1)).to(gpu, dtype)
        mask = torch.rand(1, T, T, generator=torch.Generator().manual_seed(2)) < 0.3
        mask[..., 0] = False
        mask = mask.to(gpu)
        ref = _fp64_twin(m, gpu)
        pa.SeqParallelAttention.forward = staticmethod(spy)
        try:
            got = _step(m, x, mask)
        finally:
            pa.SeqParallelAttention.forward = staticmethod(orig)
        e = _errors(got, _step(ref, x.double(), mask))
    print(f"gqa {family}:", {k: f"{v:.2e}" for k, v in e.items()})
    assert spy.ctx.gs.expand and spy.ctx.gs.Hg == Hg
    # saved: k, o, lse, then the gathered buffer(s) (and score buffers, 1-D): the [q|v] buffer is Hg wide
    bufs = [s for s in saved[0][3:] if len(s) == 3]
    assert bufs and all(s == (1, T, 2 * Hg * D) for s in bufs), saved
    assert e["out"] <= tol, e
    for k, v in e.items():
        if k != "out":
            assert v <= gtol, (k, v)


# ---- emulated middle rank --------------------------------------------------------------------------
def _middle_rank_case(rank, ws, chunks, B=1):
    """As tests/test_segmented.py::_gpu_case (segmented forward, own block first, bounds 1e-2 / 2e-2),
    with 2 gathered heads for 4 row heads.  ``B`` = 2 with 2 chunks: the chunks are separate buffers,
    so the backward runs one column kernel and one partial row-side launch per chunk."""
    import os

    from xdot.parallel import gather_sequence
    from xdot.parallel.attention import _hip_ok, seq_parallel_attention_packed, start_gather
    from xdot.utils.env import FLAGS

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.environ["XDOT_LOCAL_FIRST"] = "1"
    FLAGS.reload()
    C, H, Hg, L = 256, 4, 2, 200
    Cg, T, G = C * Hg // H, L * ws, H // Hg
    g = torch.Generator().manual_seed(9)
    k_full = torch.randn(B, T, C, generator=g).to(dev, torch.bfloat16)
    qv_full = torch.randn(B, T, 2 * Cg, generator=g).to(dev, torch.bfloat16)
    mask = torch.rand(B, T, T, generator=g) < 0.3
    mask[:, :L, :L] = True                        # rank 0's rows: own block fully masked
    mask[:, :L, L] = False
    mask = mask.to(dev)
    sl = slice(rank * L, (rank + 1) * L)
    k = k_full[:, sl].clone().requires_grad_(True)
    qv = qv_full[:, sl].clone().requires_grad_(True)
    assert _hip_ok(k, qv, H, Hg) and not _hip_ok(k, qv, H)
    pend = start_gather(qv, chunks=chunks)
    o = seq_parallel_attention_packed(k, qv, mask[:, sl], H, 0.125, pending=pend, gathered_heads=Hg)
    o.float().square().sum().backward()
    assert qv.grad.shape == qv.shape

    kf = k_full.float().requires_grad_(True)
    qvf = qv_full.float().requires_grad_(True)
    kh = kf.view(B, T, H, C // H).transpose(1, 2)
    qh = qvf[..., :Cg].reshape(B, T, Hg, C // H).transpose(1, 2).repeat_interleave(G, dim=1)
    vh = qvf[..., Cg:].reshape(B, T, Hg, C // H).transpose(1, 2).repeat_interleave(G, dim=1)
    s = (kh @ qh.transpose(-1, -2) * 0.125).masked_fill(mask.unsqueeze(1), -float("inf"))
    ref = (s.softmax(-1) @ vh).transpose(1, 2).reshape(B, T, C)
    ref.square().sum().backward()
    assert _rel(gather_sequence(o.detach(), -2), ref) <= 1e-2
    assert _rel(gather_sequence(k.grad, -2), kf.grad) <= 2e-2
    assert _rel(gather_sequence(qv.grad, -2), qvf.grad) <= 2e-2


@pytest.mark.parametrize("chunks,B", [(1, 1), (2, 1), (2, 2)])
def test_emulated_middle_rank(gpu, chunks, B):
    """3 gloo ranks sharing the GPU: rank 1 is a middle rank (peers on both sides of its own block)."""
    from _dist import run_gloo

    run_gloo(_middle_rank_case, 3, chunks, B, timeout=400)


# ---- the families that expand, on several ranks ------------------------------------------------------
# family -> (D, dtype, relative Frobenius bound against fp64 for out and every gradient: the op-level bound of
# tests/test_flash_wide_gpu.py::test_flash_wide_bf16 and of tests/test_flash_f32_gpu.py::test_flash_f32_fwd_bwd)
EXPANDING = {"wide_bf16": (160, torch.bfloat16, 2e-2), "exact_fp32": (64, torch.float32, 2e-6)}


def _expanding_case(rank, ws, path, chunks, B):
    """One rank of ``ws``, 200 rows each, H = 4, Hg = 2, the random 0.3 mask of :func:`_middle_rank_case` (rank
    0's own block fully masked), both families of ``EXPANDING``.  (a) ``o`` and ``k.grad`` are bitwise those of
    the same call without ``gathered_heads`` on a ``qv`` whose heads are repeated here: the kernels then get
    the same values under the same launch plan.  (b) ``o``, ``k.grad`` and ``qv.grad`` (the group sums),
    gathered over the ranks, against fp64 torch on the whole sequence with repeated heads."""
    import os

    from xdot.parallel import gather_sequence
    from xdot.parallel.attention import seq_parallel_attention_packed, start_gather
    from xdot.parallel.ring import ring_attention_packed
    from xdot.utils.env import FLAGS

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.environ["XDOT_LOCAL_FIRST"] = "1"
    FLAGS.reload()
    H, Hg, L = 4, 2, 200
    T, G = L * ws, H // Hg
    sl = slice(rank * L, (rank + 1) * L)
    for family, (D, dt, tol) in EXPANDING.items():
        C, Cg, scale = H * D, Hg * D, 1.0 / math.sqrt(D)
        g = torch.Generator().manual_seed(9)
        k_full = torch.randn(B, T, C, generator=g).to(dev, dt)
        qv_full = torch.randn(B, T, 2 * Cg, generator=g).to(dev, dt)
        do_full = torch.randn(B, T, C, generator=g).to(dev, dt)
        mask = torch.rand(B, T, T, generator=g) < 0.3
        mask[:, :L, :L] = True                        # rank 0's rows: own block fully masked
        mask[:, :L, L] = False
        mask = mask.to(dev)
        qv_rep = torch.cat([_expand(qv_full[..., :Cg], Hg, G), _expand(qv_full[..., Cg:], Hg, G)], dim=-1)

        def run(src, hg):
            k = k_full[:, sl].clone().requires_grad_(True)
            qv = src[:, sl].clone().requires_grad_(True)
            if path == "flash":
                o = seq_parallel_attention_packed(k, qv, mask[:, sl], H, scale, pending=start_gather(qv, chunks=chunks),
                                                  gathered_heads=hg)
            else:
                o = ring_attention_packed(k, qv, mask[:, sl], H, scale, gathered_heads=hg)
            o.backward(do_full[:, sl])
            torch.cuda.synchronize()
            assert qv.grad.shape == qv.shape, f"{family}: d[q|v] {tuple(qv.grad.shape)}, qv {tuple(qv.shape)}"
            return o.detach(), k.grad, qv.grad

        o, dk, dqv = run(qv_full, Hg)
        o_rep, dk_rep, _ = run(qv_rep, None)
        assert torch.equal(o, o_rep), f"{family}: o differs from the call on repeated heads"
        assert torch.equal(dk, dk_rep), f"{family}: dk differs from the call on repeated heads"

        kf = k_full.double().requires_grad_(True)
        qvf = qv_full.double().requires_grad_(True)
        kh = kf.view(B, T, H, D).transpose(1, 2)
        qh = qvf[..., :Cg].reshape(B, T, Hg, D).transpose(1, 2).repeat_interleave(G, dim=1)
        vh = qvf[..., Cg:].reshape(B, T, Hg, D).transpose(1, 2).repeat_interleave(G, dim=1)
        s = (kh @ qh.transpose(-1, -2) * scale).masked_fill(mask.unsqueeze(1), -float("inf"))
        ref = (s.softmax(-1) @ vh).transpose(1, 2).reshape(B, T, C)
        ref.backward(do_full.double())
        errs = {"o": _rel(gather_sequence(o, -2), ref.detach()), "dk": _rel(gather_sequence(dk, -2), kf.grad),
                "d[q|v]": _rel(gather_sequence(dqv, -2), qvf.grad)}
        if rank == 1:
            print(f"gqa expanding [{path} {family} chunks={chunks} B={B}]:", {n: f"{e:.2e}" for n, e in errs.items()})
        for n, e in errs.items():
            assert e <= tol, f"{family} {n}: {e:.3e} > {tol:.0e}"


@pytest.mark.parametrize("chunks,B", [(1, 1), (2, 1), (2, 2)])
def test_expanding_families_flash_three_ranks(gpu, chunks, B):
    """The flash path where the gathered heads are repeated for the kernels and the gradients folded, on a
    middle rank of 3: wide bf16 (D = 160, no score buffer: the segmented forward) and exact fp32 (D = 64, one
    kernel on the score buffer); one gather chunk, two chunks in one buffer (the per-chunk fold of one
    kernel's partial) and two chunks as separate buffers (B = 2: a column kernel and a fold per chunk)."""
    from _dist import run_gloo

    run_gloo(_expanding_case, 3, "flash", chunks, B, timeout=400)


def test_expanding_families_ring_three_ranks(gpu):
    """The ring's per-block expansion and fold on 3 ranks (B = 1: the bidirectional merged-lane schedule),
    same families and checks."""
    from _dist import run_gloo

    run_gloo(_expanding_case, 3, "ring", 1, 1, timeout=400)


def test_module_padded_heads(gpu):
    """Head dims no kernel takes (40): the Hg gathered heads and the H row heads are zero-padded
    separately to 64.  bf16, H = 2, Hg = 1, against the fp64 module with tests/test_module_gpu.py's
    bf16 bounds (output 2e-2, gradients 3e-2)."""
    import xdot
    from xdot.utils.comm import LocalComm, use_comm

    torch.manual_seed(0)
    with use_comm(LocalComm()):
        m = xdot.DistributedDotProductAttn(80, num_heads=2, num_gathered_heads=1, impl="flash", add_bias=True).to(gpu, torch.bfloat16)
        x = torch.randn(1, 200, 80, generator=torch.Generator().manual_seed(1)).to(gpu, torch.bfloat16)
        mask = torch.rand(1, 200, 200, generator=torch.Generator().manual_seed(2)) < 0.3
        mask[..., 0] = False
        mask = mask.to(gpu)
        e = _errors(_step(m, x, mask), _step(_fp64_twin(m, gpu), x.double(), mask))
    print("gqa padded heads:", {k: f"{v:.2e}" for k, v in e.items()})
    for k, v in e.items():
        assert v <= (2e-2 if k == "out" else 3e-2), (k, v)


# ---- capture -----------------------------------------------------------------------------------------
def _train(gpu, graphed, steps=5, warmup=2):
    import xdot
    from xdot.utils.graphs import GraphedStep

    torch.manual_seed(0)
    m = xdot.DistributedDotProductAttn(256, num_heads=4, num_gathered_heads=2, impl="flash").to(gpu, torch.bfloat16)
    opt = xdot.FusedAdamW(m.parameters(), lr=1e-3, capturable=graphed)
    crit = xdot.MSELoss()
    g = torch.Generator(device=gpu).manual_seed(1)
    x = torch.rand(1, 512, 256, device=gpu, dtype=torch.bfloat16, generator=g)
    y = torch.rand(1, 512, 256, device=gpu, dtype=torch.bfloat16, generator=g)
    mask = torch.rand(1, 512, 512, device=gpu, generator=g) < 0.2
    mask[..., 0] = False

    def body():
        loss = crit(m(x, x, x, mask), y)
        loss.backward()
        opt.step()
        return loss

    losses = []
    if graphed:
        st = GraphedStep(body, zero_grad=opt.zero_grad, warmup=warmup)
        losses.append(st().float().item())          # warmup + 1 steps
        for _ in range(steps - warmup - 1):
            losses.append(st().float().item())
    else:
        for i in range(steps):
            opt.zero_grad(set_to_none=True)
            l = body().float().item()
            if i >= warmup:
                losses.append(l)
    torch.cuda.synchronize()
    return losses, [p.detach().float().clone() for p in m.parameters()]


def test_graphed_step_matches_eager(gpu):
    """As tests/test_graphs_gpu.py, with grouped heads."""
    le, pe = _train(gpu, False)
    lg, pg = _train(gpu, True)
    assert len(le) == len(lg) == 3
    for a, b in zip(le, lg):
        assert abs(a - b) <= 2e-2 * abs(a) + 1e-6, (le, lg)
    for a, b in zip(pe, pg):
        assert ((a - b).norm() / a.norm()).item() < 1e-2
