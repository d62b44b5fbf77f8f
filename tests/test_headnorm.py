"""QK-norm on the CPU paths: the formula and its gradients, the rounding model of
``tests/_headnorm_ref.py`` against an emulation of the kernels (and against five wrong ones), and
the module with ``qk_norm=True`` on every ``impl`` over in-process ranks against the single-device
module and a dense torch reference."""
import math

import pytest
import torch

import _headnorm_ref as ref
from _headnorm_ref import BF16, DT_IDS, F32, FP16

DIM = 64
LENGTH = 6


# ---------------------------------------------------------------------------------- formula
@pytest.mark.parametrize("off,alpha", [(None, 1.0), (None, 0.7), (3, 1.0), (3, 0.7)])
def test_formula_elementwise(off, alpha):
    """``xdot.head_rms_norm`` in fp64 against the definition written out feature by feature."""
    import xdot

    B, R, H, D = 2, 5, 3, 6
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(B, R, H * D, dtype=torch.float64, generator=gen)
    w = torch.rand(D, dtype=torch.float64, generator=gen) + 0.5
    got = xdot.head_rms_norm(x, H, w, 1e-3, rotary=None if off is None else xdot.Rotary(), offset=off, alpha=alpha)
    eps, al = 1e-3, alpha
    xv = x.view(B, R, H, D)
    want = torch.empty(B, R, H, D, dtype=torch.float64)
    for b in range(B):
        for r in range(R):
            for h in range(H):
                row = xv[b, r, h]
                rs = 1.0 / (sum(float(v) ** 2 for v in row) / D + eps) ** 0.5
                y = [float(row[i]) * rs * float(w[i]) for i in range(D)]
                if off is not None:
                    o = list(y)
                    for i in range(D // 2):
                        th = (off + r) * 10000.0 ** (-2 * i / D)
                        o[i] = y[i] * math.cos(th) - y[i + D // 2] * math.sin(th)
                        o[i + D // 2] = y[i + D // 2] * math.cos(th) + y[i] * math.sin(th)
                    y = o
                want[b, r, h] = torch.tensor([al * v for v in y], dtype=torch.float64)
    torch.testing.assert_close(got, want.view(B, R, H * D), rtol=1e-12, atol=0)
    # the module form is the same function
    mod = xdot.HeadRMSNorm(D, 1e-3).double()
    with torch.no_grad():
        mod.weight.copy_(w)
    torch.testing.assert_close(mod(x, rotary=None if off is None else xdot.Rotary(), offset=off, alpha=alpha), got,
                               rtol=0, atol=0)
    # and so is the reference helper, up to its fp32 eps / alpha
    r64, _r, _s = ref.ref_forward(x, H, w, 1e-3, off, alpha)
    torch.testing.assert_close(r64, got, rtol=1e-6, atol=0)


def test_gradcheck():
    import xdot
    from xdot.ops.headnorm import norm_packed

    rot = xdot.Rotary()
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(2, 5, 12, dtype=torch.float64, generator=gen).requires_grad_(True)
    w = (torch.rand(6, dtype=torch.float64, generator=gen) + 0.5).requires_grad_(True)
    w3 = (torch.rand(3, dtype=torch.float64, generator=gen) + 0.5).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t, g: xdot.head_rms_norm(t, 2, g, 1e-3), (x, w))
    assert torch.autograd.gradcheck(lambda t, g: xdot.head_rms_norm(t, 4, g, 1e-3, alpha=0.7), (x, w3))  # odd D
    # with the rotation
    assert torch.autograd.gradcheck(lambda t, g: xdot.head_rms_norm(t, 2, g, 1e-3, rotary=rot, offset=3, alpha=0.7), (x, w))
    # on the q half of a packed [q | v] view, and as the packed node with a backward factor of its own
    assert torch.autograd.gradcheck(lambda t, g: xdot.head_rms_norm(t[..., :6], 1, g, 1e-3, rotary=rot, offset=3), (x, w))
    assert torch.autograd.gradcheck(lambda t, g: norm_packed(t, 6, 1, g, 1e-3, rot, 3, alpha=0.5), (x, w))

    # in place (on a copy: a leaf cannot be overwritten), and into another tensor
    def inplace(t, g):
        y = t * 1.0
        return xdot.head_rms_norm(y, 2, g, 1e-3, rotary=rot, offset=3, alpha=0.7, out=y)

    assert torch.autograd.gradcheck(inplace, (x, w))
    assert torch.autograd.gradcheck(lambda t, g: xdot.head_rms_norm(t, 2, g, 1e-3, out=torch.empty_like(t)), (x, w))


@pytest.mark.parametrize("gain", [True, False], ids=["gain", "no_gain"])
def test_prep_prefix_of_a_packed_tensor(gain):
    """The one autograd node of ``xdot.ops.qkprep`` on the first 6 of 10 features (a packed
    ``[q | v]``), with a gain (norm and rotation) and without (the rotation alone): the prefix is
    what the op gives on the prefix alone, the tail is copied bit for bit into a new tensor, and the
    backward hands the tail's gradient through unchanged."""
    import xdot
    from xdot.ops.qkprep import prep

    gen = torch.Generator().manual_seed(6)
    x = torch.randn(1, 3, 10, dtype=torch.float64, generator=gen).requires_grad_(True)
    w = (torch.rand(6, dtype=torch.float64, generator=gen) + 0.5).requires_grad_(True) if gain else None
    g = torch.randn(1, 3, 10, dtype=torch.float64, generator=gen)
    rot = xdot.Rotary()
    tab = rot.table(3, 6, 3, x.device, torch.float64)
    out = prep(x, 6, 1, tab, w, 1e-3, alpha=0.5, bwd_alpha=1.0)
    assert out.data_ptr() != x.data_ptr() and out.shape == x.shape
    assert torch.equal(out[..., 6:], x.detach()[..., 6:])
    xp = x.detach()[..., :6].clone().requires_grad_(True)
    if gain:
        wp = w.detach().clone().requires_grad_(True)
        alone = xdot.head_rms_norm(xp, 1, wp, 1e-3, rotary=rot, offset=3, alpha=0.5)
    else:
        alone = xdot.rope(xp, 1, rot, offset=3, alpha=0.5)
    assert torch.equal(out[..., :6], alone)
    out.backward(g)
    assert torch.equal(x.grad[..., 6:], g[..., 6:])
    alone.backward(2.0 * g[..., :6])  # (bwd_alpha = 1 against the whole op's alpha = 0.5)
    torch.testing.assert_close(x.grad[..., :6], xp.grad, rtol=1e-12, atol=1e-12)
    if gain:
        torch.testing.assert_close(w.grad, wp.grad, rtol=1e-12, atol=1e-12)


def test_scale_invariance():
    """With ``eps`` -> 0 the norm forgets the scale of its input."""
    import xdot
    from xdot.ops.headnorm import head_rms_norm_apply

    gen = torch.Generator().manual_seed(3)
    x = torch.randn(2, 7, 24, dtype=torch.float64, generator=gen)
    w = torch.rand(8, dtype=torch.float64, generator=gen) + 0.5
    tiny = 1e-300  # (eps = 0 itself is refused: the formula's only guard against a zero row)
    a, _, _ = head_rms_norm_apply(x, 3, w, tiny)
    for c in (3.7, 1e-3, 250.0):
        b, _, _ = head_rms_norm_apply(c * x, 3, w, tiny)
        torch.testing.assert_close(b, a, rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError):
        xdot.head_rms_norm(x, 3, w, 0.0)


def test_zero_rows_and_zero_gains():
    """A row of zeros gives zeros and a finite gradient (``dx = g w / sqrt(eps)`` there: the norm's
    Jacobian at 0 is ``diag(w) / sqrt(eps)``, not 0); a gain with a zero entry gives the exact ``dx`` (nothing
    is reconstructed by dividing by the gain)."""
    import xdot

    gen = torch.Generator().manual_seed(4)
    x = torch.randn(1, 6, 16, dtype=torch.float64, generator=gen)
    x[:, 2] = 0.0
    w = torch.rand(8, dtype=torch.float64, generator=gen) + 0.5
    w[3] = 0.0
    g = torch.randn(1, 6, 16, dtype=torch.float64, generator=gen)
    eps = 2.0 ** -20  # (exact in fp32, to which the reference rounds it as the kernels' launch struct does)
    for rot in (None, xdot.Rotary()):
        for inplace in (False, True):
            xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
            y = xr * 1.0
            out = xdot.head_rms_norm(y, 2, wr, eps, rotary=rot, offset=5, out=y if inplace else None)
            out.backward(g)
            assert torch.isfinite(out).all() and torch.isfinite(xr.grad).all() and torch.isfinite(wr.grad).all()
            assert bool((out[:, 2] == 0).all())
            dx, dw, _s, _t = ref.ref_backward(g, x, 2, w, eps, None if rot is None else 5)
            torch.testing.assert_close(xr.grad, dx, rtol=1e-9, atol=1e-12)
            torch.testing.assert_close(wr.grad, dw, rtol=1e-9, atol=1e-12)
            if rot is None:
                torch.testing.assert_close(xr.grad[:, 2], g[:, 2] * w.repeat(2) * 2.0 ** 10, rtol=1e-12, atol=0)
            assert bool((out.view(1, 6, 2, 8)[..., 3] == 0).all()) or rot is not None


# ---------------------------------------------------------------------------------- rounding model
EMU_SHAPES = [(2, 9, 3, 96), (1, 70, 2, 7), (1, 300, 2, 160)]


def _emu_inputs(shape, dtype, seed=0):
    B, R, H, D = shape
    gen = torch.Generator().manual_seed(seed + R)
    x = torch.randn(B, R, H * D, generator=gen).to(dtype)
    g = torch.randn(B, R, H * D, generator=gen).to(dtype)
    w = (torch.rand(D, generator=gen) + 0.5).to(dtype)
    return x, g, w


def _emu_errors(shape, dtype, off, alpha, eps, fbug=None, bbug=None):
    """Worst |error| / bound (the asserted bound, F included) of the emulation: out, dx, dw."""
    B, R, H, D = shape
    x, g, w = _emu_inputs(shape, dtype)
    p = ref.plan(B, R, H, D, x.element_size())
    out, rstd = ref.emulate_forward(x, H, w, eps, off, alpha, bug=fbug)
    o64, r64, sc = ref.ref_forward(x, H, w, eps, off, alpha)
    eo = ((out.double() - o64).abs() / ref.forward_bound(sc, dtype, p, off is not None, alpha)).max().item()
    good_rstd = ref.emulate_forward(x, H, w, eps, off, alpha)[1]
    dx, dw = ref.emulate_backward(g, x, good_rstd, H, w, off, alpha, bug=bbug)
    dx64, dw64, sx, sw = ref.ref_backward(g, x, H, w, eps, off, alpha)
    ex = ((dx.double() - dx64).abs() / ref.dx_bound(dx64, sx, dtype, p, off is not None, alpha)).max().item()
    ew = ((dw.double() - dw64).abs() / ref.dw_bound(dw64, sw, w.dtype, p, off is not None, alpha, B, R, H)).max().item()
    return eo, ex, ew


@pytest.mark.parametrize("dtype", [F32, BF16, FP16], ids=DT_IDS.get)
@pytest.mark.parametrize("shape", EMU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_model_holds_the_emulation(shape, dtype):
    """The kernels' algorithm, emulated in fp32 torch in their order of operations, stays inside
    the bounds: forward, dx and dw, with and without the rotation and ``alpha``."""
    D = shape[3]
    for off, alpha in [(None, 1.0), (None, 0.37)] + ([(1000, 1.0), (1000, 0.1803)] if D % 2 == 0 else []):
        eo, ex, ew = _emu_errors(shape, dtype, off, alpha, 1e-6)
        print(f"emulation {DT_IDS[dtype]} {shape} off={off} alpha={alpha}: out {eo:.2f} dx {ex:.2f} dw {ew:.2f} of the bound")
        assert eo <= 1.0 and ex <= 1.0 and ew <= 1.0, (eo, ex, ew)


@pytest.mark.parametrize("dtype", [F32, BF16, FP16], ids=DT_IDS.get)
def test_model_catches_wrong_kernels(dtype):
    """Five wrong kernels leave the bounds (in every dtype): ``eps`` added after the square root, a
    mean over ``H D`` instead of ``D``, rotate-then-normalise with a non-constant gain, a ``dx``
    without the projection term, a ``dw`` missing one workgroup's partial."""
    shape = (2, 9, 3, 96)
    eo, _, _ = _emu_errors(shape, dtype, None, 1.0, 0.1, fbug="eps_after_sqrt")
    assert eo > 1.0, eo
    assert _emu_errors(shape, dtype, None, 1.0, 0.1)[0] <= 1.0
    eo, _, _ = _emu_errors(shape, dtype, None, 1.0, 1e-6, fbug="mean_over_hd")
    assert eo > 1.0, eo
    eo, _, _ = _emu_errors(shape, dtype, 1000, 1.0, 1e-6, fbug="rotate_first")
    assert eo > 1.0, eo
    _, ex, ew = _emu_errors(shape, dtype, 1000, 1.0, 1e-6, bbug="no_projection")
    assert ex > 1.0 and ew <= 1.0, (ex, ew)
    _, ex, ew = _emu_errors((1, 300, 2, 160), dtype, None, 1.0, 1e-6, bbug="drop_partial")
    assert ew > 1.0 and ex <= 1.0, (ex, ew)


# ---------------------------------------------------------------------------------- module
def _make_mask(kind, B, T, gen):
    import xdot

    if kind == "none":
        return None, None
    if kind == "causal":
        m = xdot.StructuredMask(causal=True)
        return m, m.dense(B, T, T, 0)
    mask = torch.rand(B, T, T, generator=gen) < 0.35
    mask[..., torch.arange(T), torch.arange(T)] = False
    return mask, mask


def _gains(m, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n in ("keys_norm", "queries_norm"):
            wt = getattr(m, n).weight
            wt.copy_(torch.rand(wt.shape, generator=gen, dtype=torch.float64) + 0.5)


def _rank_parity(rank, ws, impl, chunks, kind, rope, Hg=None, layout="contiguous", sync=False, tol=1e-9):
    """``tests/test_rope.py``'s module parity (1e-9; 1e-8 on the Sum-reduced parameter gradients) with
    ``qk_norm=True``: every rank's rows against the ``distributed=False`` module on the whole
    sequence, which rank 0 also holds against the dense torch reference.  ``sync``: the gradients
    are reduced by a ``GradSync`` (hooks, early delivery) and compared after its ``wait()``."""
    import xdot
    from xdot import DistributedDotProductAttn, Rotary
    from xdot.parallel import GradSync, allreduce_gradients, broadcast_parameters

    dtype, H, B = torch.float64, 4, 1
    torch.manual_seed(100 + rank)
    kw = dict(num_heads=H, add_bias=True, num_gathered_heads=Hg, qk_norm=True, qk_norm_eps=1e-5)
    model = DistributedDotProductAttn(DIM, impl=impl, chunk_plan=chunks, layout=layout, rope=Rotary() if rope else None,
                                      **kw).to(dtype)
    gt_model = DistributedDotProductAttn(DIM, distributed=False, impl="materialized", rope=Rotary() if rope else None,
                                         **kw).to(dtype)
    _gains(model, 40 + rank)
    broadcast_parameters(model)
    gt_model.load_state_dict(model.state_dict())
    gs = GradSync(model) if sync else None
    gen = torch.Generator().manual_seed(7)
    T = LENGTH * ws
    x_full = torch.rand(B, T, DIM, generator=gen, dtype=dtype)
    mask, dense = _make_mask(kind, B, T, gen)
    comm = xdot.get_comm()
    x = xdot.shard_rows(x_full, rank, ws, layout=layout).clone().requires_grad_(True)
    local = xdot.shard_rows(mask, rank, ws, layout=layout) if isinstance(mask, torch.Tensor) else mask
    out = model(x, x, x, local)
    out.sum().backward()
    xg = x_full.clone().requires_grad_(True)
    gt_out = gt_model(xg, xg, xg, dense)
    gt_out.sum().backward()
    outs = xdot.unshard_rows(comm.all_gather_object(out.detach()), layout=layout)
    dxs = xdot.unshard_rows(comm.all_gather_object(x.grad), layout=layout)
    torch.testing.assert_close(outs, gt_out.detach(), atol=tol, rtol=tol)
    torch.testing.assert_close(dxs, xg.grad, atol=tol, rtol=tol)
    if gs is not None:
        gs.wait()
    else:
        allreduce_gradients(model)
    names = [n for n, _ in model.named_parameters()]
    assert "keys_norm.weight" in names and "queries_norm.weight" in names
    for (n1, p1), (n2, p2) in zip(gt_model.named_parameters(), model.named_parameters()):
        assert n1 == n2 and p2.grad is not None
        torch.testing.assert_close(p2.grad, p1.grad, atol=tol * 10, rtol=tol * 10, msg=lambda m: f"d{n1}: {m}")
    if rank == 0:
        params = {n: p.detach().clone().requires_grad_(True) for n, p in gt_model.named_parameters()}
        xd = x_full.clone().requires_grad_(True)
        want = ref.dense_attn(params, xd, xd, xd, dense, H, Hg, rope=rope, eps=1e-5)
        want.sum().backward()
        torch.testing.assert_close(gt_out.detach(), want.detach(), atol=tol, rtol=tol)
        torch.testing.assert_close(xg.grad, xd.grad, atol=tol, rtol=tol)
        for n, p in gt_model.named_parameters():
            torch.testing.assert_close(p.grad, params[n].grad, atol=tol * 10, rtol=tol * 10, msg=lambda m: f"dense d{n}: {m}")


IMPLS = {"flash_whole": ("flash", 1), "flash_chunked": ("flash", 2), "ring": ("ring", None),
         "materialized": ("materialized", None)}


@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("impl", list(IMPLS))
@pytest.mark.parametrize("ws", [2, 3])
def test_module_ranks(ws, impl, rope):
    """Every ``impl`` (flash whole and chunked), with and without ``rope``, a causal ``StructuredMask``."""
    from xdot.utils.comm import ThreadGroup

    ThreadGroup(ws).run(lambda r: _rank_parity(r, ws, *IMPLS[impl], "causal", rope))


@pytest.mark.parametrize("impl", ["flash_chunked", "ring", "materialized"])
def test_module_ranks_grouped_heads_zigzag(impl):
    """``num_gathered_heads < num_heads`` under ``layout='zigzag'`` with ``rope``, and a dense mask."""
    from xdot.utils.comm import ThreadGroup

    Hg = None if impl == "materialized" else 2
    ThreadGroup(3).run(lambda r: _rank_parity(r, 3, *IMPLS[impl], "causal", True, Hg=Hg, layout="zigzag"))
    ThreadGroup(2).run(lambda r: _rank_parity(r, 2, *IMPLS[impl], "dense", True, Hg=2))


@pytest.mark.parametrize("fused", [True, False])
def test_module_grad_sync_and_per_op_graph(fused, monkeypatch):
    """``XDOT_FUSED_MODULE=1`` and ``=0`` both equal the single-device module (hence each other),
    with the gradients -- the two gains' included -- reduced by a ``GradSync`` and read after
    ``wait()``."""
    from xdot.utils.comm import ThreadGroup
    from xdot.utils.env import FLAGS

    monkeypatch.setattr(FLAGS, "fused_module", fused)
    ThreadGroup(3).run(lambda r: _rank_parity(r, 3, "flash", 2, "causal", True, sync=True))


@pytest.mark.parametrize("impl", ["flash", "ring", "materialized"])
def test_off_is_bitwise_the_module_without_the_argument(impl):
    """``qk_norm=False``: output, every gradient and the ``state_dict`` keys are those of a module
    built without the argument."""
    import xdot

    res = []
    for kw in ({}, {"qk_norm": False, "qk_norm_eps": 1e-3}):
        torch.manual_seed(0)
        m = xdot.DistributedDotProductAttn(DIM, num_heads=4, distributed=False, impl=impl, add_bias=True,
                                           rope=xdot.Rotary(), **kw).double()
        x = torch.randn(2, 11, DIM, dtype=torch.float64, generator=torch.Generator().manual_seed(5)).requires_grad_(True)
        out = m(x, x, x, xdot.StructuredMask(causal=True))
        out.sum().backward()
        res.append((list(m.state_dict()), [out.detach(), x.grad] + [p.grad for p in m.parameters()]))
    assert res[0][0] == res[1][0] == [f"{n}.{p}" for n in ("keys", "queries", "values", "composition")
                                      for p in ("weight", "bias")]
    for a, b in zip(res[0][1], res[1][1]):
        assert torch.equal(a, b)


def test_state_dict():
    import xdot

    m = xdot.DistributedDotProductAttn(DIM, num_heads=4, qk_norm=True)
    assert tuple(m.keys_norm.weight.shape) == tuple(m.queries_norm.weight.shape) == (DIM // 4,)
    assert bool((m.keys_norm.weight == 1).all()) and bool((m.queries_norm.weight == 1).all())
    _gains(m, 1)
    sd = m.state_dict()
    assert [k for k in sd if "norm" in k] == ["keys_norm.weight", "queries_norm.weight"]
    m2 = xdot.DistributedDotProductAttn(DIM, num_heads=4, qk_norm=True)
    m2.load_state_dict(sd)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, sd[k])
    # a reference-shaped dict: exactly the two gains are missing
    plain = xdot.DistributedDotProductAttn(DIM, num_heads=4).state_dict()
    res = m2.load_state_dict(plain, strict=False)
    assert sorted(res.missing_keys) == ["keys_norm.weight", "queries_norm.weight"] and not res.unexpected_keys
    with pytest.raises(RuntimeError):
        m2.load_state_dict(plain)
    # and without qk_norm the reference's dict loads strictly
    xdot.DistributedDotProductAttn(DIM, num_heads=4, qk_norm=False).load_state_dict(plain)
    assert "qk_norm=True" in repr(m) and "qk_norm" not in repr(xdot.DistributedDotProductAttn(DIM, num_heads=4))


def test_validation():
    import xdot

    with pytest.raises(ValueError):
        xdot.DistributedDotProductAttn(8, num_heads=2, qk_norm=True, qk_norm_eps=0.0)
    with pytest.raises(ValueError):
        xdot.DistributedDotProductAttn(8, num_heads=2, qk_norm=True, qk_norm_eps=-1e-6)
    with pytest.raises(ValueError):
        xdot.HeadRMSNorm(4, eps=0.0)
    x = torch.zeros(1, 5, 12)
    with pytest.raises(ValueError):
        xdot.head_rms_norm(x, 2, torch.ones(4))  # weight shape
    with pytest.raises(ValueError):
        xdot.head_rms_norm(x, 2, torch.ones(6), eps=0.0)
    with pytest.raises(ValueError):
        xdot.head_rms_norm(x, 4, torch.ones(3), rotary=xdot.Rotary())  # odd D with a rotary
    xdot.head_rms_norm(x, 4, torch.ones(3))  # odd D without one
    with pytest.raises(TypeError):
        xdot.head_rms_norm(x, 2, torch.ones(6), rotary="rotary")
    with pytest.raises(ValueError):
        xdot.head_rms_norm(x, 2, torch.ones(6), out=torch.zeros(1, 5, 6))  # out mismatch
    with pytest.raises(ValueError):
        xdot.head_rms_norm(x, 2, torch.ones(6), out=torch.zeros(1, 5, 12, dtype=torch.float64))
    with pytest.raises(ValueError):
        xdot.head_rms_norm(x, 5, torch.ones(2))  # 12 features over 5 heads
