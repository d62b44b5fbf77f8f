"""Grouped-query attention (``num_gathered_heads`` < ``num_heads``) on the CPU: the shared torch
reference with grouped heads against autograd of a dense attention with the gathered heads
repeated, the module against a ``num_heads``-only module with repeated weights, emulated ranks
(flash whole / chunked, ring, materialized) against the single-device module with the width of
every collective recorded, and the argument checks."""
import pytest
import torch

B, R, T, H, DH, DV, SCALE = 2, 5, 7, 4, 4, 6, 0.3
TOL = dict(rtol=1e-12, atol=1e-12)  # fp64 round-off on sums of at most 7 x 4 terms, as tests/test_attention_ref.py


def _case(Hg):
    g = torch.Generator().manual_seed(11 + Hg)
    k = torch.randn(B, R, H * DH, generator=g, dtype=torch.float64)
    q = torch.randn(B, T, Hg * DH, generator=g, dtype=torch.float64)
    v = torch.randn(B, T, Hg * DV, generator=g, dtype=torch.float64)
    do = torch.randn(B, R, H * DV, generator=g, dtype=torch.float64)
    mask = torch.rand(B, R, T, generator=g) < 0.4
    mask[..., 5] = False                        # every row alive, also within the segment [3, 7)
    return k, q, v, do, mask


def _dense(k, q, v, mask, Hg):
    """softmax(mask(k qᵀ·scale)) v per head, gathered heads repeated for their group -> (out, lse)"""
    kh = k.view(B, R, H, DH).transpose(1, 2)
    qh = q.view(B, T, Hg, DH).transpose(1, 2).repeat_interleave(H // Hg, dim=1)
    vh = v.view(B, T, Hg, DV).transpose(1, 2).repeat_interleave(H // Hg, dim=1)
    s = (kh @ qh.transpose(-1, -2) * SCALE).masked_fill(mask.unsqueeze(1), -float("inf"))
    return (s.softmax(-1) @ vh).transpose(1, 2).reshape(B, R, H * DV), s.logsumexp(-1)


@pytest.mark.parametrize("Hg", [1, 2])
def test_ref_block_fwd_bwd_match_autograd(Hg):
    from xdot.parallel import _ref

    k, q, v, do, mask = _case(Hg)
    ka, qa, va = (t.clone().requires_grad_(True) for t in (k, q, v))
    ref_o, ref_lse = _dense(ka, qa, va, mask, Hg)
    ref_o.backward(do)
    o, lse = _ref.block_fwd(k, q, v, mask, H, SCALE, Hg)
    torch.testing.assert_close(o, ref_o.detach(), **TOL)
    torch.testing.assert_close(lse, ref_lse.detach(), **TOL)
    dk, dq, dv = _ref.block_bwd(do, k, q, v, lse, _ref.delta(do, o, H, torch.float64), mask, H, SCALE, Hg)
    assert dq.shape == q.shape and dv.shape == v.shape
    torch.testing.assert_close(dk, ka.grad, **TOL)
    torch.testing.assert_close(dq, qa.grad, **TOL)
    torch.testing.assert_close(dv, va.grad, **TOL)


@pytest.mark.parametrize("Hg", [1, 2])
def test_ref_column_split_is_exact(Hg):
    from xdot.parallel import _ref

    k, q, v, do, mask = _case(Hg)
    mask = mask.clone()
    mask[0, 2, :3] = True                       # a row the first segment masks entirely
    parts = [_ref.block_fwd(k, q[:, a:b], v[:, a:b], mask[..., a:b], H, SCALE, Hg) for a, b in ((0, 3), (3, 7))]
    o, lse = _ref.combine(parts, torch.float64)
    ref_o, ref_lse = _dense(k, q, v, mask, Hg)
    torch.testing.assert_close(o, ref_o, **TOL)
    torch.testing.assert_close(lse, ref_lse, **TOL)
    # the segments' gradients, given the whole row's lse / delta, add up to the whole's
    delta = _ref.delta(do, o, H, torch.float64)
    whole = _ref.block_bwd(do, k, q, v, lse, delta, mask, H, SCALE, Hg)
    segs = [_ref.block_bwd(do, k, q[:, a:b], v[:, a:b], lse, delta, mask[..., a:b], H, SCALE, Hg) for a, b in ((0, 3), (3, 7))]
    torch.testing.assert_close(segs[0][0] + segs[1][0], whole[0], **TOL)
    torch.testing.assert_close(torch.cat([segs[0][1], segs[1][1]], 1), whole[1], **TOL)
    torch.testing.assert_close(torch.cat([segs[0][2], segs[1][2]], 1), whole[2], **TOL)


# ---- module oracle, single device -------------------------------------------------------------
DIM, HEADS, LENGTH = 64, 4, 18


def _repeat_rows(w, Hg, G):
    """(Hg * d, ...) -> (Hg * G * d, ...): every head's rows repeated G times (repeat_interleave of heads)."""
    d = w.shape[0] // Hg
    return w.reshape(Hg, 1, d, *w.shape[1:]).expand(Hg, G, d, *w.shape[1:]).reshape(Hg * G * d, *w.shape[1:])


def _fold_rows(g, Hg, G):
    """gradient of the repeated rows -> the sum over the G copies of every head"""
    d = g.shape[0] // (Hg * G)
    return g.reshape(Hg, G, d, *g.shape[1:]).sum(1).reshape(Hg * d, *g.shape[1:])


def _mha_twin(m, Hg, **kw):
    """A ``num_heads``-only module computing what the grouped module ``m`` computes: its ``queries`` /
    ``values`` parameters are ``m``'s with each head's rows repeated G times."""
    import xdot

    ref = xdot.DistributedDotProductAttn(DIM, num_heads=HEADS, add_bias=True, **kw).double()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    for n in ("queries.weight", "queries.bias", "values.weight", "values.bias"):
        sd[n] = _repeat_rows(sd[n], Hg, HEADS // Hg).clone()
    ref.load_state_dict(sd)
    return ref


@pytest.mark.parametrize("impl", ["flash", "ring", "materialized"])
@pytest.mark.parametrize("Hg,rope", [(1, False), (2, False), (4, False), (2, True)])
def test_module_matches_repeated_weights(impl, Hg, rope):
    import xdot

    torch.manual_seed(3 + Hg)
    kw = dict(distributed=False, impl=impl, rope=xdot.Rotary() if rope else None)
    m = xdot.DistributedDotProductAttn(DIM, num_heads=HEADS, num_gathered_heads=Hg, add_bias=True, **kw).double()
    ref = _mha_twin(m, Hg, **kw)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, LENGTH, DIM, generator=g, dtype=torch.float64)
    mask = torch.rand(2, LENGTH, LENGTH, generator=g) < 0.35
    mask[..., torch.arange(LENGTH), torch.arange(LENGTH)] = False
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    w = torch.randn(2, LENGTH, DIM, generator=g, dtype=torch.float64)
    ya, yb = m(xa, xa, xa, mask), ref(xb, xb, xb, mask)
    (ya * w).sum().backward()
    (yb * w).sum().backward()
    # the fp64 tolerances of tests/test_module_options.py::test_packed_qv_parameters_share_storage
    tol = dict(rtol=1e-9, atol=1e-11)
    torch.testing.assert_close(ya, yb, **tol)
    torch.testing.assert_close(xa.grad, xb.grad, **tol)
    for (n, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        want = _fold_rows(q.grad, Hg, HEADS // Hg) if n.split(".")[0] in ("queries", "values") else q.grad
        assert p.grad.shape == p.shape
        torch.testing.assert_close(p.grad, want, msg=lambda s, n=n: f"{n}: {s}", **tol)


# ---- emulated ranks -------------------------------------------------------------------------------
def _recording(group, rank, log):
    """A rank's communicator that notes the last-dim width of everything it moves."""
    from xdot.utils.comm import ThreadComm

    class Rec(ThreadComm):
        def all_gather_into(self, out, inp, async_op=False):
            log.append(("all_gather", inp.shape[-1]))
            return super().all_gather_into(out, inp, async_op)

        def reduce_scatter(self, out, inp, async_op=False):
            log.append(("reduce_scatter", inp.shape[-1]))
            return super().reduce_scatter(out, inp, async_op)

        def sendrecv(self, send, recv, dst, src, async_op=False):
            log.append(("hop", send.shape[-1]))
            return super().sendrecv(send, recv, dst, src, async_op)

    return Rec(group, rank)


def _rank_parity(rank, ws, group, impl, Hg, chunk_plan, logs, tol=1e-9):
    """As tests/test_gradient.py::_module_parity (same bounds), with grouped heads and a recording
    communicator."""
    import xdot
    from xdot.parallel import allreduce_gradients, broadcast_parameters, gather_sequence

    comm = _recording(group, rank, logs[rank])
    torch.manual_seed(100 + rank)
    model = xdot.DistributedDotProductAttn(DIM, num_heads=HEADS, num_gathered_heads=Hg, impl=impl, add_bias=True,
                                           chunk_plan=chunk_plan, comm=comm).double()
    gt = xdot.DistributedDotProductAttn(DIM, num_heads=HEADS, num_gathered_heads=Hg, distributed=False,
                                        impl="materialized", add_bias=True).double()
    broadcast_parameters(model)
    gt.load_state_dict(model.state_dict())
    g = torch.Generator().manual_seed(7)
    T = LENGTH * ws
    x_full = torch.rand(1, T, DIM, generator=g, dtype=torch.float64)
    mask_full = torch.rand(1, T, T, generator=g) < 0.35
    mask_full[..., torch.arange(T), torch.arange(T)] = False
    sl = slice(rank * LENGTH, (rank + 1) * LENGTH)
    x = x_full[:, sl].clone().requires_grad_(True)
    logs[rank].clear()  # (the parameter broadcast is not attention traffic)
    out = model(x, x, x, mask_full[:, sl])
    out.sum().backward()
    xg = x_full.clone().requires_grad_(True)
    gt_out = gt(xg, xg, xg, mask_full)
    gt_out.sum().backward()
    moved = list(logs[rank])
    torch.testing.assert_close(gather_sequence(out.detach(), -2), gt_out.detach(), atol=tol, rtol=tol)
    torch.testing.assert_close(gather_sequence(x.grad, -2), xg.grad, atol=tol, rtol=tol)
    allreduce_gradients(model)
    for (n1, p1), (n2, p2) in zip(gt.named_parameters(), model.named_parameters()):
        assert n1 == n2
        if n1 == "queries.bias":  # exactly 0 in exact arithmetic (softmax shift invariance): noise only
            assert p2.grad.abs().max() <= 1e-6 * max(1.0, p1.grad.abs().max().item()) + 1e3 * tol
            continue
        torch.testing.assert_close(p2.grad, p1.grad, atol=tol * 10, rtol=tol * 10)
    return moved


@pytest.mark.parametrize("ws", [2, 3])
@pytest.mark.parametrize("impl,chunk_plan", [("flash", None), ("flash", 2), ("ring", None), ("materialized", None)])
@pytest.mark.parametrize("Hg", [1, 2])
def test_ranks_match_single_device(ws, impl, chunk_plan, Hg):
    from xdot.utils.comm import ThreadGroup

    group = ThreadGroup(ws)
    logs = [[] for _ in range(ws)]
    moved = group.run(lambda r: _rank_parity(r, ws, group, impl, Hg, chunk_plan, logs))
    d = DIM // HEADS
    for m in moved:
        if impl == "materialized":
            continue  # (the reference's structure: per-head operands move through its own chunked products)
        kinds = {kind for kind, _ in m}
        assert kinds == ({"all_gather", "reduce_scatter"} if impl == "flash" else {"hop"}), m
        # everything on the wire is the packed [q | v] (or its gradient) of the Hg gathered heads
        assert all(width == 2 * Hg * d for _, width in m), (m, 2 * Hg * d, 2 * HEADS * d)


# ---- validation and defaults ------------------------------------------------------------------------
def test_indivisible_heads_raise():
    import xdot

    with pytest.raises(ValueError):
        xdot.DistributedDotProductAttn(64, num_heads=4, num_gathered_heads=3)
    with pytest.raises(ValueError):
        xdot.DistributedDotProductAttn(64, num_heads=4, num_gathered_heads=0)


def test_shapes_and_state_dict_keys():
    import xdot

    m = xdot.DistributedDotProductAttn(64, value_dim=32, query_dim=48, num_heads=4, num_gathered_heads=2, add_bias=True)
    assert set(m.state_dict()) == {f"{n}.{p}" for n in ("keys", "queries", "values", "composition")
                                   for p in ("weight", "bias")}
    assert m.queries.weight.shape == (2 * 16, 48)
    assert m.values.weight.shape == (2 * 8, 32)
    assert m.keys.weight.shape == (64, 64) and m.composition.weight.shape == (32, 32)
    assert "num_gathered_heads=2" in m.extra_repr()


def test_default_argument_changes_no_shape():
    import xdot

    kw = dict(value_dim=32, query_dim=48, num_heads=4, add_bias=True)
    a = xdot.DistributedDotProductAttn(64, **kw)
    for b in (xdot.DistributedDotProductAttn(64, num_gathered_heads=None, **kw),
              xdot.DistributedDotProductAttn(64, num_gathered_heads=4, **kw)):
        assert {n: p.shape for n, p in a.named_parameters()} == {n: p.shape for n, p in b.named_parameters()}
    assert a.queries.weight.shape == (64, 48) and a.values.weight.shape == (32, 32)
    assert "num_gathered_heads" not in a.extra_repr()


def test_packed_entry_points_check_the_width():
    from xdot.parallel.attention import seq_parallel_attention_packed
    from xdot.parallel.ring import ring_attention_packed
    from xdot.utils.comm import LocalComm

    k = torch.randn(1, 6, 32, dtype=torch.float64)
    qv = torch.randn(1, 6, 2 * 16, dtype=torch.float64)  # two gathered heads of 8 (+ 8 value) columns
    for fn in (seq_parallel_attention_packed, ring_attention_packed):
        o = fn(k, qv, None, 4, 0.3, comm=LocalComm(), gathered_heads=2)
        assert o.shape == (1, 6, 32)
        with pytest.raises(ValueError):
            fn(k, qv, None, 4, 0.3, comm=LocalComm(), gathered_heads=3)


# ---- the gathered side as the kernels read it --------------------------------------------------
@pytest.mark.parametrize("grad_fp32", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32, torch.float64])
def test_wire_dtype_is_the_three_rules_it_replaces(monkeypatch, dtype, grad_fp32):
    """``wire_dtype`` against the three expressions it replaced, written out: the ring's accumulator
    dtype, the rounding of the flash torch path's partials (else they stay in the compute dtype), and
    the flash HIP path's ``gdt`` (on the dtypes that path takes: fp64 never reaches a kernel)."""
    from xdot.parallel import _ref
    from xdot.parallel._gathered import wire_dtype
    from xdot.parallel.attention import FLASH_DTYPES
    from xdot.utils.env import FLAGS

    monkeypatch.setattr(FLAGS, "grad_fp32", grad_fp32)
    k = torch.empty(0, dtype=dtype)
    got = wire_dtype(dtype)
    ring = k.dtype if (k.dtype in (torch.bfloat16, torch.float16) and not FLAGS.grad_fp32) else (
        torch.float32 if k.dtype != torch.float64 else k.dtype)
    assert got == ring
    parts = torch.empty(0, dtype=_ref.compute_dtype(k))
    if k.dtype in (torch.bfloat16, torch.float16) and not FLAGS.grad_fp32:
        parts = parts.to(k.dtype)
    assert got == parts.dtype
    if dtype in FLASH_DTYPES:
        assert got == (k.dtype if not FLAGS.grad_fp32 else torch.float32)


def test_gathered_side_view_and_fold():
    """H = 4, Hg = 2, D = 2 on the CPU, ``expand`` forced: every gathered head stands G = 2 times in the
    kernel view, the halves split at H * D, and a partial of distinct integers folds to the group sums in
    head order; without ``expand`` the view is the buffer itself, the halves split at Hg * D and the fold
    is the identity."""
    from xdot.parallel._gathered import GatheredSide

    k = torch.zeros(1, 1, 8)
    g = torch.arange(8.0).view(1, 1, 8)            # [q0 q1 | v0 v1], two columns a head
    gs = GatheredSide(k, 4, 2, 0.5, False, expand=True)
    assert (gs.Cq, gs.kC, gs.kHg, gs.Hg) == (4, 8, None, 2)
    x = gs.view(g)
    assert x.tolist() == [[[0, 1, 0, 1, 2, 3, 2, 3, 4, 5, 4, 5, 6, 7, 6, 7]]]
    q, v = gs.halves(x)
    assert q.tolist() == [[[0, 1, 0, 1, 2, 3, 2, 3]]] and v.tolist() == [[[4, 5, 4, 5, 6, 7, 6, 7]]]
    part = torch.arange(16.0).view(1, 1, 16)       # [dq of row heads 0..3 | dv of row heads 0..3]
    folded = gs.fold(part, torch.float64)
    assert folded.dtype == torch.float64 and folded.tolist() == [[[2, 4, 10, 12, 18, 20, 26, 28]]]

    same = GatheredSide(k, 4, 2, 0.5, False)       # a CPU tensor never expands by itself
    assert not same.expand and (same.Cq, same.kC, same.kHg) == (4, 4, 2)
    assert same.view(g) is g and same.fold(part, torch.float64) is part
    q, v = same.halves(g)
    assert q.tolist() == [[[0, 1, 2, 3]]] and v.tolist() == [[[4, 5, 6, 7]]]
    plain = GatheredSide(k, 4, None, 0.5, False)   # no grouping: the q half is as wide as k
    assert (plain.Cq, plain.kC, plain.kHg) == (8, 8, None) and not plain.expand
