"""Gated attention on the CPU paths: ``xdot.sigmoid_gate`` and the module's ``gate=`` against autograd
of the definition in fp64, the rounding model of ``tests/_gate_ref.py`` against an emulation of the
kernels (and against six wrong algorithms), and the module on every ``impl`` over in-process ranks
against the single-device module and the dense definition."""
import pytest
import torch

import _gate_ref as ref
from _gate_ref import BF16, DT_IDS, F32, F64, FP16, INF

DIM = 64
LENGTH = 6
KINDS = ["elementwise", "headwise"]


def _ops_inputs(kind, B=2, R=5, H=3, D=4, seed=0):
    gen = torch.Generator().manual_seed(seed)
    o = torch.randn(B, R, H * D, dtype=F64, generator=gen)
    g = 2 * torch.randn(B, R, H if kind == "headwise" else H * D, dtype=F64, generator=gen)
    dy = torch.randn(B, R, H * D, dtype=F64, generator=gen)
    return o, g, dy


# ---------------------------------------------------------------------------------- the function
@pytest.mark.parametrize("kind", KINDS)
def test_function_against_autograd_of_the_definition(kind):
    """Forward, ``do`` and ``dg`` of ``xdot.sigmoid_gate`` against autograd of ``o * sigmoid(g)`` in
    fp64 at the 1e-12 of ``tests/test_sinks.py``; exported from ``xdot`` and ``xdot.ops``."""
    import xdot
    import xdot.ops

    assert xdot.sigmoid_gate is xdot.ops.sigmoid_gate
    H = 3
    o, g, dy = _ops_inputs(kind)
    res = []
    for fn in (lambda o, g: xdot.sigmoid_gate(o, g, H), lambda o, g: ref.gate(o, g, H)):
        oo, gg = o.clone().requires_grad_(True), g.clone().requires_grad_(True)
        out = fn(oo, gg)
        out.backward(dy)
        res.append((out.detach(), oo.grad, gg.grad))
    for a, b, n in zip(res[0], res[1], ("out", "do", "dg")):
        assert a.shape == b.shape and a.dtype == b.dtype, n
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12, msg=lambda m: f"{n}: {m}")


@pytest.mark.parametrize("kind", KINDS)
def test_gradcheck(kind):
    import xdot

    o, g, _ = _ops_inputs(kind, B=1, R=3, H=2, D=3, seed=3)
    ins = [o.requires_grad_(True), g.requires_grad_(True)]
    assert torch.autograd.gradcheck(lambda o, g: xdot.sigmoid_gate(o, g, 2), ins, eps=1e-6, atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize("dtype", [F64, F32, BF16], ids=["fp64", "fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_extreme_gates_and_nan_rows(kind, dtype):
    """``g = +inf`` gives ``o`` bit for bit, ``-inf`` gives +-0, +-100 and 0 are finite (0 halves), the
    gradients at +-inf and +-100 are finite zeros or tiny, and a NaN row of ``o`` stays NaN without
    touching the other rows."""
    import xdot

    H, D = 2, 4
    o = torch.randn(1, 7, H * D, generator=torch.Generator().manual_seed(1)).to(dtype)
    o[0, 6] = float("nan")
    vals = [INF, -INF, 100.0, -100.0, 0.0, 30.0]
    g = torch.tensor(vals, dtype=dtype).view(1, 6, 1).expand(1, 6, H if kind == "headwise" else H * D)
    g = torch.cat([g, torch.zeros(1, 1, g.shape[-1], dtype=dtype)], dim=1).contiguous()
    oo, gg = o.clone().requires_grad_(True), g.clone().requires_grad_(True)
    out = xdot.sigmoid_gate(oo, gg, H)
    assert torch.equal(out[0, 0], o[0, 0])                                   # +inf: o itself
    assert bool((out[0, 1] == 0).all()) and torch.equal(torch.signbit(out[0, 1]), torch.signbit(o[0, 1]))  # -inf: +-0
    assert torch.equal(out[0, 2], o[0, 2])                                   # sigmoid(100) rounds to 1
    assert bool(torch.isfinite(out[0, :6]).all())
    torch.testing.assert_close(out[0, 4].double(), o[0, 4].double() / 2, rtol=2.0 ** -8, atol=0)  # zero halves
    assert bool(torch.isnan(out[0, 6]).all())
    out[:, :6].double().sum().backward()
    assert bool(torch.isfinite(oo.grad).all()) and bool(torch.isfinite(gg.grad[:, :6]).all())
    assert bool((gg.grad[0, :2] == 0).all())                                 # sigma'(+-inf) = 0
    assert bool((oo.grad[0, 1] == 0).all()) and bool((oo.grad[0, 0] == 1).all())


def test_argument_checks():
    import xdot

    o = torch.zeros(2, 3, 12, dtype=F64)
    with pytest.raises(ValueError):
        xdot.sigmoid_gate(o, torch.zeros(2, 3, 5, dtype=F64), 3)   # neither C nor heads
    with pytest.raises(ValueError):
        xdot.sigmoid_gate(o, torch.zeros(2, 4, 12, dtype=F64), 3)  # rows
    with pytest.raises(ValueError):
        xdot.sigmoid_gate(o, torch.zeros(2, 3, 12, dtype=F64), 5)  # heads do not divide C
    with pytest.raises(ValueError):
        xdot.sigmoid_gate(o[0], torch.zeros(3, 12, dtype=F64), 3)  # rank
    with pytest.raises(ValueError):
        xdot.sigmoid_gate(o, torch.zeros(2, 3, 12, dtype=F64), 0)
    for bad in ("sigmoid", "tanh", True, 1):
        with pytest.raises(ValueError):
            xdot.DistributedDotProductAttn(DIM, num_heads=4, gate=bad)
    assert xdot.sigmoid_gate(o, torch.zeros(2, 3, 3), 3).dtype == F64  # g of another float dtype is cast


# ---------------------------------------------------------------------------------- model and emulation
EMU_SHAPES = [(1, 1, 1, 8), (2, 5, 3, 96), (1, 67, 8, 96), (1, 130, 2, 128), (1, 9, 1, 1024), (1, 9, 1, 260),
              (1, 33, 4, 20), (2, 3, 5, 2)]


def _emu_ratios(shape, dtype, kind, bug=None, inputs=None):
    """(o', do, dg) errors of the emulation in units of the unit bounds."""
    B, R, H, D = shape
    o, g, dy = inputs if inputs is not None else ref.gate_inputs(B, R, H, D, dtype, kind == "headwise", seed=R + D)
    y64, by = ref.ref_apply(o, g, H, dtype)
    do64, dg64, bdo, bdg = ref.ref_backward(dy, o, g, H, dtype)
    y = ref.emulate_apply(o, g, H, bug)
    do, dg = ref.emulate_backward(dy, o, g, H, bug)
    return ref.ratio(y, y64, by), ref.ratio(do, do64, bdo), ref.ratio(dg, dg64, bdg)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [F32, BF16, FP16], ids=DT_IDS.get)
@pytest.mark.parametrize("shape", EMU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_model_holds_the_emulation(shape, dtype, kind):
    """The kernels' algorithm, emulated in fp32 torch in their order of operations, stays inside F
    times the unit bounds on the GPU test's shapes and planted values."""
    from xdot.ops.gate import gate_apply, gate_backward

    r = _emu_ratios(shape, dtype, kind)
    print(f"RATIO emulation {DT_IDS[dtype]} {shape} {kind}: o' {r[0]:.2f} do {r[1]:.2f} dg {r[2]:.2f}")
    assert max(r) <= ref.F, r
    # the emulation is xdot's own torch path, operation for operation, wherever no sum is involved
    B, R, H, D = shape
    o, g, dy = ref.gate_inputs(B, R, H, D, dtype, kind == "headwise", seed=R + D)
    bits = lambda t: torch.nan_to_num(t.float(), nan=12345.0).view(torch.int32)
    assert torch.equal(bits(gate_apply(o, g, H)), bits(ref.emulate_apply(o, g, H)))
    do, dg = gate_backward(dy, o, g, H)
    edo, edg = ref.emulate_backward(dy, o, g, H)
    assert torch.equal(bits(do), bits(edo))
    if kind == "elementwise":
        assert torch.equal(bits(dg), bits(edg))


def _large_gates(shape, dtype, kind, sign):
    """|g| in [8, 14] of one sign (where ``sigma - sigma^2`` and ``1 - sigma`` cancel), o and do' of
    order 64 so that every result is a normal number in fp16 too."""
    B, R, H, D = shape
    gen = torch.Generator().manual_seed(11)
    o = (64 * torch.randn(B, R, H * D, generator=gen)).to(dtype)
    dy = (64 * torch.randn(B, R, H * D, generator=gen)).to(dtype)
    g = (sign * (8 + 6 * torch.rand(B, R, H if kind == "headwise" else H * D, generator=gen))).to(dtype)
    return o, g, dy


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [F32, BF16, FP16], ids=DT_IDS.get)
def test_model_catches_wrong_kernels(dtype, kind):
    """Six wrong algorithms leave the bounds, in every dtype: ``sigma - sigma^2`` for ``sigma'``,
    ``1.f - sigma`` for the other sign, ``do`` left ungated, and -- headwise -- the sum kept in 16 bits
    (16-bit dtypes), the sum without its last lane step, ``g`` read with the wrong head stride."""
    from xdot.ops.gate import gate_apply, gate_backward

    shape = (2, 37, 3, 96)
    assert max(_emu_ratios(shape, dtype, kind)) <= ref.F
    for sign in (1.0, -1.0):
        # xdot's torch path on the inputs that expose the cancellations: inside the bounds
        o, g, dy = _large_gates(shape, dtype, kind, sign)
        y64, by = ref.ref_apply(o, g, 3, dtype)
        do64, dg64, bdo, bdg = ref.ref_backward(dy, o, g, 3, dtype, K=96)
        do, dg = gate_backward(dy, o, g, 3)
        assert max(ref.ratio(gate_apply(o, g, 3), y64, by), ref.ratio(do, do64, bdo), ref.ratio(dg, dg64, bdg)) <= ref.F
        assert max(_emu_ratios(shape, dtype, kind, inputs=_large_gates(shape, dtype, kind, sign))) <= ref.F
    _, _, rdg = _emu_ratios(shape, dtype, kind, "sigma_minus_sq", _large_gates(shape, dtype, kind, 1.0))
    assert rdg > ref.F, rdg
    ry, rdo, _ = _emu_ratios(shape, dtype, kind, "one_minus", _large_gates(shape, dtype, kind, -1.0))
    assert ry > ref.F and rdo > ref.F, (ry, rdo)
    _, rdo, _ = _emu_ratios(shape, dtype, kind, "ungated")
    assert rdo > ref.F, rdo
    if kind == "headwise":
        ry, rdo, rdg = _emu_ratios(shape, dtype, kind, "head_stride")
        assert ry > ref.F and rdo > ref.F and rdg > ref.F, (ry, rdo, rdg)
        _, _, rdg = _emu_ratios(shape, dtype, kind, "last_chunk")
        assert rdg > ref.F, rdg
        if dtype != F32:
            _, _, rdg = _emu_ratios(shape, dtype, kind, "sum16", ref.gate_inputs(2, 37, 3, 96, dtype, True, plant=False))
            assert rdg > ref.F, rdg


@pytest.mark.parametrize("kind", KINDS)
def test_torch_path_is_inside_the_model(kind):
    """The torch path of ``xdot.ops.gate`` (CPU tensors, ``backend='torch'``): fp32 math and one cast,
    inside the same bounds in bf16 and fp32 (the headwise sum's order is torch's: its longest chain is
    taken as D, which covers any order)."""
    from xdot.ops.gate import gate_apply, gate_backward

    for dtype in (F32, BF16):
        o, g, dy = ref.gate_inputs(2, 37, 3, 96, dtype, kind == "headwise", seed=2)
        y64, by = ref.ref_apply(o, g, 3, dtype)
        do64, dg64, bdo, bdg = ref.ref_backward(dy, o, g, 3, dtype, K=96)
        ref.check(f"torch path o' {kind}", gate_apply(o, g, 3), y64, by)
        do, dg = gate_backward(dy, o, g, 3)
        ref.check(f"torch path do {kind}", do, do64, bdo)
        ref.check(f"torch path dg {kind}", dg, dg64, bdg)


# ---------------------------------------------------------------------------------- module
@pytest.mark.parametrize("impl", ["flash", "ring", "materialized"])
@pytest.mark.parametrize("kind", KINDS)
def test_module_against_autograd_of_the_definition(kind, impl):
    """``dW_g``, ``db_g``, ``dx`` and every other gradient of the single-device module against
    autograd of the dense definition in fp64 (1e-12 / 1e-11 on the parameter gradients), with sinks,
    grouped heads, bias and a causal window; the gate reads the ROW-side input."""
    import xdot

    torch.manual_seed(0)
    Hg = None if impl == "materialized" else 2
    m = xdot.DistributedDotProductAttn(DIM, num_heads=4, distributed=False, impl=impl, add_bias=True, sinks=True,
                                       num_gathered_heads=Hg, gate=kind).double()
    assert tuple(m.gate.weight.shape) == ((DIM, DIM) if kind == "elementwise" else (4, DIM))
    gen = torch.Generator().manual_seed(5)
    xk, xq = (torch.randn(2, 9, DIM, dtype=F64, generator=gen) for _ in range(2))
    spec = xdot.StructuredMask(causal=True, window=4)
    dense = spec.dense(2, 9, 9, 0)
    a, b = (t.clone().requires_grad_(True) for t in (xk, xq))
    out = m(a, b, b, spec)
    out.pow(2).mean().backward()
    params = {n: p.detach().clone().requires_grad_(True) for n, p in m.named_parameters()}
    c, d = (t.clone().requires_grad_(True) for t in (xk, xq))
    want = ref.dense_attn(params, c, d, d, dense, 4, Hg)
    want.pow(2).mean().backward()
    torch.testing.assert_close(out.detach(), want.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(a.grad, c.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(b.grad, d.grad, rtol=1e-12, atol=1e-12)
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        torch.testing.assert_close(p.grad, params[n].grad, rtol=1e-11, atol=1e-11, msg=lambda s: f"d{n}: {s}")
    assert float(m.gate.weight.grad.abs().max()) > 0 and float(m.gate.bias.grad.abs().max()) > 0


def _make_mask(kind, B, T, gen):
    import xdot

    if kind in ("causal", "window"):
        m = xdot.StructuredMask(causal=True, window=4 if kind == "window" else None)
        return m, m.dense(B, T, T, 0)
    if kind == "documents":
        m = xdot.StructuredMask(causal=True, doc_starts=[0, 5, T - 3])
        return m, m.dense(B, T, T, 0)
    mask = torch.rand(B, T, T, generator=gen) < 0.35
    mask[..., torch.arange(T), torch.arange(T)] = False
    return mask, mask


def _rank_parity(rank, ws, impl, chunks, kind, mask_kind, rope=False, norm=False, Hg=None, layout="contiguous", sinks=False,
                 sync=False, tol=1e-9):
    """Every rank's rows of the module with a gate against the ``distributed=False`` module on the
    whole sequence (1e-9; 1e-8 on the Sum-reduced parameter gradients, the gate's among them), which
    rank 0 also holds against the dense definition."""
    import xdot
    from xdot import DistributedDotProductAttn, Rotary
    from xdot.parallel import GradSync, allreduce_gradients, broadcast_parameters

    dtype, H, B = F64, 4, 1
    torch.manual_seed(100 + rank)
    kw = dict(num_heads=H, add_bias=True, num_gathered_heads=Hg, qk_norm=norm, sinks=sinks, gate=kind)
    model = DistributedDotProductAttn(DIM, impl=impl, chunk_plan=chunks, layout=layout, rope=Rotary() if rope else None,
                                      **kw).to(dtype)
    gt_model = DistributedDotProductAttn(DIM, distributed=False, impl="materialized", rope=Rotary() if rope else None,
                                         **kw).to(dtype)
    broadcast_parameters(model)
    gt_model.load_state_dict(model.state_dict())
    gs = GradSync(model) if sync else None
    gen = torch.Generator().manual_seed(7)
    T = LENGTH * ws
    x_full = torch.rand(B, T, DIM, generator=gen, dtype=dtype)
    mask, dense = _make_mask(mask_kind, B, T, gen)
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
    local_dw = model.gate.weight.grad.detach().clone() if gs is None else None
    if gs is not None:
        gs.wait()
    else:
        allreduce_gradients(model)
    names = [n for n, _ in model.named_parameters()]
    assert "gate.weight" in names and "gate.bias" in names
    for (n1, p1), (n2, p2) in zip(gt_model.named_parameters(), model.named_parameters()):
        assert n1 == n2 and p2.grad is not None, n1
        torch.testing.assert_close(p2.grad, p1.grad, atol=tol * 10, rtol=tol * 10, msg=lambda m: f"d{n1}: {m}")
    if local_dw is not None and ws > 1:  # each rank's gradient is the partial over its rows
        parts = comm.all_gather_object(local_dw)
        torch.testing.assert_close(sum(parts), gt_model.gate.weight.grad, atol=tol * 10, rtol=tol * 10)
    if rank == 0:
        params = {n: p.detach().clone().requires_grad_(True) for n, p in gt_model.named_parameters()}
        xd = x_full.clone().requires_grad_(True)
        want = ref.dense_attn(params, xd, xd, xd, dense, H, Hg, rope=rope)
        want.sum().backward()
        torch.testing.assert_close(gt_out.detach(), want.detach(), atol=tol, rtol=tol)
        torch.testing.assert_close(xg.grad, xd.grad, atol=tol, rtol=tol)
        for n, p in gt_model.named_parameters():
            torch.testing.assert_close(p.grad, params[n].grad, atol=tol * 10, rtol=tol * 10, msg=lambda m: f"dense d{n}: {m}")


IMPLS = {"flash_whole": ("flash", 1), "flash_chunked": ("flash", 2), "ring": ("ring", None),
         "materialized": ("materialized", None)}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("impl", list(IMPLS))
@pytest.mark.parametrize("ws", [2, 3, 4])
def test_module_ranks(ws, impl, kind):
    """Every ``impl`` (flash whole and chunked, ring, materialized) on 2..4 ranks: a causal window with
    the elementwise gate, a dense random mask with the headwise gate."""
    from xdot.utils.comm import ThreadGroup

    ThreadGroup(ws).run(lambda r: _rank_parity(r, ws, *IMPLS[impl], kind, "window" if kind == "elementwise" else "dense"))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("impl", ["flash_chunked", "ring", "materialized"])
def test_module_ranks_with_the_other_features(impl, kind):
    """With ``rope``, ``qk_norm`` and ``sinks``, ``num_gathered_heads < num_heads`` under
    ``layout='zigzag'``, and a document mask."""
    from xdot.utils.comm import ThreadGroup

    Hg = None if impl == "materialized" else 2
    ThreadGroup(3).run(lambda r: _rank_parity(r, 3, *IMPLS[impl], kind, "window", True, True, Hg=Hg, layout="zigzag",
                                              sinks=True))
    ThreadGroup(2).run(lambda r: _rank_parity(r, 2, *IMPLS[impl], kind, "documents", True, False, Hg=2 if Hg else None))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fused", [True, False])
def test_module_grad_sync_sums_the_gate_gradients(fused, kind, monkeypatch):
    """``XDOT_FUSED_MODULE=1`` and ``=0`` with the gradients -- the gate projection's included --
    reduced by a ``GradSync`` and read after ``wait()``."""
    from xdot.utils.comm import ThreadGroup
    from xdot.utils.env import FLAGS

    monkeypatch.setattr(FLAGS, "fused_module", fused)
    ThreadGroup(3).run(lambda r: _rank_parity(r, 3, "flash", 2, kind, "causal", True, sinks=True, sync=True))


@pytest.mark.parametrize("impl", ["flash", "ring", "materialized"])
def test_none_is_bitwise_the_module_without_the_keyword(impl):
    """``gate=None``: output, every gradient and the ``state_dict`` keys are those of a module built
    without the keyword."""
    import xdot

    res = []
    for kw in ({}, {"gate": None}):
        torch.manual_seed(0)
        m = xdot.DistributedDotProductAttn(DIM, num_heads=4, distributed=False, impl=impl, add_bias=True, **kw).double()
        x = torch.randn(2, 11, DIM, dtype=F64, generator=torch.Generator().manual_seed(5)).requires_grad_(True)
        out = m(x, x, x, xdot.StructuredMask(causal=True))
        out.sum().backward()
        res.append((list(m.state_dict()), [out.detach(), x.grad] + [p.grad for p in m.parameters()]))
    assert res[0][0] == res[1][0] == [f"{n}.{p}" for n in ("keys", "queries", "values", "composition")
                                      for p in ("weight", "bias")]
    for a, b in zip(res[0][1], res[1][1]):
        assert torch.equal(a, b)


def test_state_dict_and_repr():
    import xdot

    plain_m = xdot.DistributedDotProductAttn(DIM, num_heads=4, num_gathered_heads=2)
    plain = plain_m.state_dict()
    assert not any("gate" in k for k in plain) and not hasattr(plain_m, "gate") and "gate" not in repr(plain_m)
    for kind, rows in (("elementwise", DIM), ("headwise", 4)):
        for bias in (False, True):
            m = xdot.DistributedDotProductAttn(DIM, num_heads=4, num_gathered_heads=2, gate=kind, add_bias=bias)
            keys = ["gate.weight"] + (["gate.bias"] if bias else [])
            assert [k for k in m.state_dict() if "gate" in k] == keys
            assert tuple(m.gate.weight.shape) == (rows, DIM)  # one per ROW head: grouped heads do not change it
            assert f"gate={kind}" in repr(m)
            m2 = xdot.DistributedDotProductAttn(DIM, num_heads=4, num_gathered_heads=2, gate=kind, add_bias=bias)
            m2.load_state_dict(m.state_dict())
            for k, v in m2.state_dict().items():
                assert torch.equal(v, m.state_dict()[k])
        # a reference-shaped dict: exactly the gate is missing
        m = xdot.DistributedDotProductAttn(DIM, num_heads=4, num_gathered_heads=2, gate=kind)
        res = m.load_state_dict(plain, strict=False)
        assert res.missing_keys == ["gate.weight"] and not res.unexpected_keys
        with pytest.raises(RuntimeError):
            m.load_state_dict(plain)
    xdot.DistributedDotProductAttn(DIM, num_heads=4, num_gathered_heads=2, gate=None).load_state_dict(plain)


def test_zero_preactivation_halves_the_output():
    import xdot

    x = torch.randn(1, 7, DIM, dtype=F64, generator=torch.Generator().manual_seed(2))
    outs = []
    for kind in (None, "elementwise", "headwise"):
        torch.manual_seed(0)
        m = xdot.DistributedDotProductAttn(DIM, num_heads=4, distributed=False, impl="flash", gate=kind).double()
        if kind is not None:
            torch.nn.init.zeros_(m.gate.weight)
        outs.append(m(x, x, x, None))
    for o in outs[1:]:
        torch.testing.assert_close(o, outs[0] / 2, rtol=1e-13, atol=1e-14)


def test_compute_dtype_policy_casts_the_gate_weight():
    """Under ``dtype=`` the gate projection runs in the compute dtype and its fp32 master weight gets an
    fp32 gradient."""
    import xdot

    torch.manual_seed(0)
    m = xdot.DistributedDotProductAttn(DIM, num_heads=4, distributed=False, impl="flash", gate="headwise", dtype=BF16)
    x = torch.randn(1, 7, DIM)
    out = m(x, x, x, None)
    out.sum().backward()
    assert out.dtype == F32 and m.gate.weight.dtype == F32 and m.gate.weight.grad.dtype == F32
    assert float(m.gate.weight.grad.abs().max()) > 0


@pytest.mark.parametrize("impl", ["flash", "ring", "materialized"])
def test_check_raises_when_ranks_disagree_on_the_gate(impl, monkeypatch):
    import xdot
    from xdot.utils.checks import RankDivergenceError
    from xdot.utils.comm import ThreadGroup
    from xdot.utils.env import FLAGS

    monkeypatch.setattr(FLAGS, "check", True)

    def body(r, kinds):
        x = torch.rand(1, LENGTH, DIM, dtype=F64)
        m = xdot.DistributedDotProductAttn(DIM, num_heads=4, impl=impl, gate=kinds[r]).double()
        return m(x, x, x, xdot.StructuredMask(causal=True))

    for kinds in (("headwise", None), ("headwise", "elementwise")):
        with pytest.raises(RankDivergenceError):
            ThreadGroup(2).run(body, kinds)
    ThreadGroup(2).run(body, ("headwise", "headwise"))
