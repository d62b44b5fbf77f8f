"""Rotary position embedding on the CPU paths: the formula, the relative-position property,
gradients, and the module on every ``impl`` over in-process ranks against the single-device
module and a dense torch reference."""
import math

import pytest
import torch

from _rope_ref import dense_attn

DIM = 64
LENGTH = 6


def test_formula_elementwise():
    """``xdot.rope`` in fp64 against the definition, element by element."""
    import xdot

    B, R, H, D, off = 2, 5, 2, 6, 3
    x = torch.rand(B, R, H * D, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    got = xdot.rope(x, H, xdot.Rotary(), offset=off)
    want = torch.empty_like(x)
    for r in range(R):
        for h in range(H):
            for i in range(D // 2):
                th = (off + r) * 10000.0 ** (-2 * i / D)
                a, b = h * D + i, h * D + i + D // 2
                want[:, r, a] = x[:, r, a] * math.cos(th) - x[:, r, b] * math.sin(th)
                want[:, r, b] = x[:, r, b] * math.cos(th) + x[:, r, a] * math.sin(th)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=0)
    # the offset of the description, and a base of its own
    torch.testing.assert_close(xdot.rope(x, H, xdot.Rotary(offset=off)), want, rtol=1e-12, atol=0)
    assert not torch.allclose(xdot.rope(x, H, xdot.Rotary(base=500.0), offset=off), want)


def test_relative_position_property():
    """Scores of rotated rows depend on the position difference only: the same at p and p + 17."""
    import xdot

    g = torch.Generator().manual_seed(1)
    a = torch.randn(1, 9, 32, dtype=torch.float64, generator=g)
    b = torch.randn(1, 9, 32, dtype=torch.float64, generator=g)
    rot = xdot.Rotary()

    def scores(p):
        ra, rb = xdot.rope(a, 2, rot, offset=p), xdot.rope(b, 2, rot, offset=p)
        ra, rb = ra.view(1, 9, 2, 16).transpose(1, 2), rb.view(1, 9, 2, 16).transpose(1, 2)
        return torch.matmul(ra, rb.transpose(-1, -2))

    torch.testing.assert_close(scores(5), scores(5 + 17), rtol=0, atol=1e-10)
    assert not torch.allclose(scores(5), torch.matmul(a.view(1, 9, 2, 16).transpose(1, 2),
                                                      b.view(1, 9, 2, 16).transpose(1, 2).transpose(-1, -2)))


def test_gradcheck():
    import xdot

    rot = xdot.Rotary()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 5, 12, dtype=torch.float64, generator=g).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: xdot.rope(t, 2, rot, offset=3, alpha=0.7), (x,))
    base = torch.randn(2, 5, 24, dtype=torch.float64, generator=g).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: xdot.rope(t[..., :12], 2, rot, offset=3, alpha=0.7), (base,))
    assert torch.autograd.gradcheck(lambda t: xdot.rope(t, 2, rot, offset=3, alpha=0.7, inverse=True), (x,))


def test_inverse_and_inplace():
    import xdot

    rot = xdot.Rotary()
    x = torch.randn(2, 7, 24, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    y = xdot.rope(x, 3, rot, offset=11)
    torch.testing.assert_close(xdot.rope(y, 3, rot, offset=11, inverse=True), x, rtol=0, atol=1e-12)
    # in place on the first half of a packed buffer: the other half is untouched
    buf = torch.cat([x, x], dim=-1)
    half = buf[..., :24]
    assert xdot.rope(half, 3, rot, offset=11, out=half) is half
    assert torch.equal(buf[..., :24], y) and torch.equal(buf[..., 24:], x)
    out = torch.zeros_like(x)
    xdot.rope(x, 3, rot, offset=11, alpha=0.5, out=out)
    torch.testing.assert_close(out, 0.5 * y, rtol=1e-15, atol=0)


def test_table_cached_and_fp32():
    import xdot

    rot = xdot.Rotary()
    c1, s1 = rot.table(5, 8, 3, "cpu")
    c2, s2 = rot.table(5, 8, 3, "cpu")
    assert c1 is c2 and s1 is s2 and c1.dtype == torch.float32 and tuple(c1.shape) == (5, 4)
    ang = torch.arange(3, 8, dtype=torch.float64).view(5, 1) * torch.tensor(rot.inv_freq(8), dtype=torch.float64)
    assert torch.equal(c1, torch.cos(ang).float()) and torch.equal(s1, torch.sin(ang).float())
    assert rot.table(5, 8, 4, "cpu")[0] is not c1


def _make_mask(kind, B, T, g):
    import xdot

    if kind == "none":
        return None, None
    if kind == "causal":
        m = xdot.StructuredMask(causal=True)
        return m, m.dense(B, T, T, 0)
    mask = torch.rand(B, T, T, generator=g) < 0.35
    mask[..., torch.arange(T), torch.arange(T)] = False  # no fully-masked row
    return mask, mask


def _rank_parity(rank, ws, heads, impl, kind, call, tol=1e-9):
    """As ``tests/test_gradient.py``'s module parity (same tolerances), with ``rope`` set."""
    import xdot
    from xdot import DistributedDotProductAttn, Rotary
    from xdot.parallel import allreduce_gradients, broadcast_parameters, gather_sequence

    dtype = torch.float64
    torch.manual_seed(100 + rank)
    model = DistributedDotProductAttn(DIM, DIM, DIM, num_heads=heads, impl=impl, add_bias=True,
                                      rope=Rotary()).to(dtype)
    gt_model = DistributedDotProductAttn(DIM, DIM, DIM, num_heads=heads, distributed=False, impl="materialized",
                                         add_bias=True, rope=Rotary()).to(dtype)
    broadcast_parameters(model)
    gt_model.load_state_dict(model.state_dict())
    g = torch.Generator().manual_seed(7)
    T = LENGTH * ws
    k_full = torch.rand(1, T, DIM, generator=g, dtype=dtype)
    q_full = torch.rand(1, T, DIM, generator=g, dtype=dtype)
    mask, dense = _make_mask(kind, 1, T, g)
    sl = slice(rank * LENGTH, (rank + 1) * LENGTH)
    k = k_full[:, sl].clone().requires_grad_(True)
    q = q_full[:, sl].clone().requires_grad_(True)
    pick = {"kqk": lambda a, b: (a, b, a), "kqq": lambda a, b: (a, b, b)}[call]
    local_mask = mask[:, sl] if isinstance(mask, torch.Tensor) else mask
    out = model(*pick(k, q), local_mask)
    out.sum().backward()
    kg = k_full.clone().requires_grad_(True)
    qg = q_full.clone().requires_grad_(True)
    gt_out = gt_model(*pick(kg, qg), mask)
    gt_out.sum().backward()
    torch.testing.assert_close(gather_sequence(out.detach(), -2), gt_out.detach(), atol=tol, rtol=tol)
    torch.testing.assert_close(gather_sequence(k.grad, -2), kg.grad, atol=tol, rtol=tol)
    torch.testing.assert_close(gather_sequence(q.grad, -2), qg.grad, atol=tol, rtol=tol)
    allreduce_gradients(model)
    for (n1, p1), (n2, p2) in zip(gt_model.named_parameters(), model.named_parameters()):
        assert n1 == n2
        # (with the rotation the scores are no longer shift invariant in the queries' bias: its
        # gradient is a real one and is compared like the others)
        torch.testing.assert_close(p2.grad, p1.grad, atol=tol * 10, rtol=tol * 10)
    if rank == 0:
        # the single-device module against the dense torch reference, on the same inputs
        params = {n: p.detach().clone().requires_grad_(True) for n, p in gt_model.named_parameters()}
        kd = k_full.clone().requires_grad_(True)
        qd = q_full.clone().requires_grad_(True)
        xk, xq, xv = pick(kd, qd)
        ref = dense_attn(params, xk, xq, xv, dense, heads, rope=True)
        ref.sum().backward()
        torch.testing.assert_close(gt_out.detach(), ref.detach(), atol=tol, rtol=tol)
        torch.testing.assert_close(kg.grad, kd.grad, atol=tol, rtol=tol)
        torch.testing.assert_close(qg.grad, qd.grad, atol=tol, rtol=tol)
        for n, p in gt_model.named_parameters():
            torch.testing.assert_close(p.grad, params[n].grad, atol=tol * 10, rtol=tol * 10)


@pytest.mark.parametrize("kind", ["none", "dense", "causal"])
@pytest.mark.parametrize("impl", ["flash", "ring", "materialized"])
@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("ws", [2, 3])
def test_module_ranks(ws, heads, impl, kind):
    """Each rank's rows and the Sum-reduced parameter gradients equal the ``distributed=False``
    module on the whole sequence, which in turn equals the dense torch reference.  ``kqq``
    (queries is values) takes the one-node module on the flash path."""
    from xdot.utils.comm import ThreadGroup

    ThreadGroup(ws).run(lambda r: _rank_parity(r, ws, heads, impl, kind, "kqq"))


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("call", ["kqq", "kqk"])
def test_module_flash_per_op_graph(call, fused, monkeypatch):
    """The flash path as one node per op (``XDOT_FUSED_MODULE=0``, or queries is not values)."""
    from xdot.utils.comm import ThreadGroup
    from xdot.utils.env import FLAGS

    monkeypatch.setattr(FLAGS, "fused_module", fused)
    ThreadGroup(3).run(lambda r: _rank_parity(r, 3, 4, "flash", "causal", call))


@pytest.mark.parametrize("impl", ["flash", "ring", "materialized"])
def test_single_device_vs_dense_reference(impl):
    """``distributed=False`` on every impl, the ``dtype=`` policy and the functional entry, against
    the dense reference (B = 2, dense mask)."""
    import xdot

    g = torch.Generator().manual_seed(5)
    B, T, H = 2, 11, 4
    x = torch.randn(B, T, DIM, dtype=torch.float64, generator=g)
    mask, dense = _make_mask("dense", B, T, g)
    m = xdot.DistributedDotProductAttn(DIM, num_heads=H, distributed=False, impl=impl, rope=xdot.Rotary()).double()
    params = dict(m.named_parameters())
    ref = dense_attn(params, x, x, x, dense, H, rope=True)
    torch.testing.assert_close(m(x, x, x, mask), ref, atol=1e-9, rtol=1e-9)
    with torch.no_grad():
        torch.testing.assert_close(m(x, x, x, mask), ref, atol=1e-9, rtol=1e-9)
    # without rope the module is what it was
    m0 = xdot.DistributedDotProductAttn(DIM, num_heads=H, distributed=False, impl=impl).double()
    m0.load_state_dict(m.state_dict())
    torch.testing.assert_close(m0(x, x, x, mask), dense_attn(params, x, x, x, dense, H, rope=False), atol=1e-9,
                               rtol=1e-9)
    # compute-dtype policy: fp32 parameters and inputs, fp64 compute
    m32 = xdot.DistributedDotProductAttn(DIM, num_heads=H, distributed=False, impl=impl, rope=xdot.Rotary(),
                                         dtype=torch.float64)
    m32.load_state_dict({k: v.float() for k, v in m.state_dict().items()})
    p32 = {n: p.double() for n, p in m32.named_parameters()}
    x32 = x.float()
    ref32 = dense_attn(p32, x32.double(), x32.double(), x32.double(), dense, H, rope=True)
    out32 = m32(x32, x32, x32, mask)
    assert out32.dtype == torch.float32
    torch.testing.assert_close(out32.double(), ref32, atol=1e-6, rtol=1e-6)


def test_functional_entry():
    import xdot
    from _rope_ref import rotate

    g = torch.Generator().manual_seed(6)
    B, T, H, C = 1, 9, 2, 16
    k, q, v = (torch.randn(B, T, C, dtype=torch.float64, generator=g) for _ in range(3))
    scale = 1.0 / math.sqrt(C // H)
    got = xdot.seq_parallel_attention(k, q, v, None, H, scale, comm=xdot.LocalComm(), rope=xdot.Rotary())
    want = xdot.seq_parallel_attention(rotate(k, H), rotate(q, H), v, None, H, scale, comm=xdot.LocalComm())
    torch.testing.assert_close(got, want, atol=1e-12, rtol=1e-12)
    assert not torch.allclose(got, xdot.seq_parallel_attention(k, q, v, None, H, scale, comm=xdot.LocalComm()))


def test_repacked_weights_survive():
    """The ``queries`` / ``values`` parameters stay packed in one storage after a forward with
    ``rope`` set (the rotation touches the projected q, never the weights)."""
    import xdot
    from xdot.models.attention import _adjacent, _stacked_rows

    m = xdot.DistributedDotProductAttn(DIM, num_heads=4, distributed=False, impl="flash", add_bias=True,
                                       rope=xdot.Rotary()).double()
    x = torch.randn(1, 7, DIM, dtype=torch.float64, generator=torch.Generator().manual_seed(8)).requires_grad_(True)
    wq, wv = m.queries.weight.detach().clone(), m.values.weight.detach().clone()
    m(x, x, x, None).sum().backward()
    assert _adjacent(m.queries.weight, m.values.weight) and _adjacent(m.queries.bias, m.values.bias)
    packed = _stacked_rows(m.queries.weight, m.values.weight)
    assert packed.data_ptr() == m.queries.weight.data_ptr()
    assert torch.equal(packed.detach(), torch.cat([wq, wv], 0))
    assert set(m.state_dict()) == {f"{n}.{p}" for n in ("keys", "queries", "values", "composition")
                                   for p in ("weight", "bias")}


def test_validation():
    import xdot

    with pytest.raises(ValueError):
        xdot.DistributedDotProductAttn(6, num_heads=2, rope=xdot.Rotary())  # head dim 3
    with pytest.raises(TypeError):
        xdot.DistributedDotProductAttn(8, num_heads=2, rope="rotary")
    x = torch.zeros(1, 5, 8)
    with pytest.raises(ValueError):
        xdot.rope(x, 2, xdot.Rotary(), offset=2**31 - 5)  # offset + R = 2^31
    with pytest.raises(ValueError):
        xdot.rope(x, 2, xdot.Rotary(offset=2**31 - 1))
    xdot.rope(x, 2, xdot.Rotary(), offset=2**31 - 6)  # offset + R = 2^31 - 1: the last position allowed
    with pytest.raises(ValueError):
        xdot.rope(torch.zeros(1, 5, 6), 2, xdot.Rotary())  # odd head dim
    with pytest.raises(ValueError):
        xdot.Rotary(offset=-1)
    m = xdot.DistributedDotProductAttn(8, num_heads=2, rope=xdot.Rotary(base=500.0))
    assert "rope=Rotary(base=500, offset=None)" in repr(m)
    assert "rope" not in repr(xdot.DistributedDotProductAttn(8, num_heads=2))
