"""Zigzag row sharding (``layout="zigzag"``, :mod:`xdot.parallel.layout`) on the CPU: the layout
functions, ``StructuredMask.dense_at``, and the module on CPU ranks (float64) against the
single-device module on the full sequence."""
import pytest
import torch

from _dist import run_gloo

LAYOUT = "zigzag"


# ---- layout functions ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,R", [(1, 5), (2, 4), (3, 7), (4, 1), (5, 2), (8, 3125)])
def test_runs_cover_every_row_once(n, R):
    from xdot.parallel.layout import gathered_cols, global_rows, row_runs

    h0 = (R + 1) // 2
    h1 = R - h0
    seen = []
    for r in range(n):
        runs = row_runs(LAYOUT, r, n, R)
        # the definition, run by run: local rows [0, h0) are chunk r, [h0, R) chunk 2n-1-r
        want = [(0, h0, r * h0)] + ([(h0, h1, n * h0 + (n - 1 - r) * h1)] if h1 else [])
        if len(want) == 2 and want[0][2] + h0 == want[1][2]:  # adjacent in global order: merged
            want = [(0, R, want[0][2])]
        assert runs == want, (r, runs)
        assert sum(ln for _ls, ln, _gs in runs) == R and runs[0][0] == 0
        rows = global_rows(LAYOUT, r, n, R)
        assert rows.dtype == torch.int64 and rows.tolist() == [g + i for _ls, ln, g in runs for i in range(ln)]
        seen += rows.tolist()
    assert sorted(seen) == list(range(n * R))
    assert gathered_cols(LAYOUT, n, R).tolist() == seen
    assert gathered_cols("contiguous", n, R).tolist() == list(range(n * R))
    assert [row_runs("contiguous", r, n, R) for r in range(n)] == [[(0, R, r * R)] for r in range(n)]


def test_one_rank_is_the_identity():
    from xdot.parallel.layout import global_rows, row_runs

    assert row_runs(LAYOUT, 0, 1, 7) == [(0, 7, 0)] and global_rows(LAYOUT, 0, 1, 7).tolist() == list(range(7))
    with pytest.raises(ValueError):
        row_runs("striped", 0, 1, 7)
    with pytest.raises(ValueError):
        row_runs(LAYOUT, 2, 2, 7)


@pytest.mark.parametrize("layout", ["contiguous", LAYOUT])
@pytest.mark.parametrize("n,R,dim", [(1, 5, 1), (2, 4, 1), (3, 7, 1), (4, 5, 2), (3, 1, 0)])
def test_shard_unshard_round_trip(layout, n, R, dim):
    import xdot
    from xdot.parallel.layout import global_rows

    shape = [2, 3, 4]
    shape[dim] = n * R
    x = torch.arange(torch.Size(shape).numel(), dtype=torch.float64).view(shape)
    parts = [xdot.shard_rows(x, r, n, dim=dim, layout=layout) for r in range(n)]
    for r, p in enumerate(parts):
        assert p.shape[dim] == R
        assert torch.equal(p, x.index_select(dim, global_rows(layout, r, n, R)))
    assert torch.equal(xdot.unshard_rows(parts, dim=dim, layout=layout), x)
    with pytest.raises(ValueError):
        xdot.shard_rows(torch.zeros(1, 7, 1), 0, 2, layout=layout)  # 7 rows over 2 ranks


# ---- dense_at -----------------------------------------------------------------------------------
def _python_mask(B, rows, cols, causal, window, lengths, starts):
    """Element by element, from the definition in StructuredMask's docstring."""
    def doc(b, x):
        s = starts if not starts or not isinstance(starts[0], list) else starts[b]
        return sum(1 for e in s if e <= x)

    out = torch.zeros(B, len(rows), len(cols), dtype=torch.bool)
    for b in range(B):
        for i, gr in enumerate(rows):
            for j, gc in enumerate(cols):
                m = False
                if causal and gc > gr:
                    m = True
                if window is not None and (gc < gr - (window - 1) or (not causal and gc > gr + (window - 1))):
                    m = True
                if lengths is not None and gc >= lengths[b]:
                    m = True
                if starts is not None and doc(b, gc) != doc(b, gr):
                    m = True
                out[b, i, j] = m
    return out


@pytest.mark.parametrize("kw", [
    dict(causal=True), dict(window=3), dict(causal=True, window=4), dict(lengths=[17, 9]),
    dict(doc_starts=[4, 11, 11, 30]), dict(doc_starts=[[2, 9], [13, 13]]),
    dict(causal=True, window=5, lengths=[20, 12], doc_starts=[[0, 6, 14], [3, 8, 19]]),
])
def test_dense_at_matches_the_definition(kw):
    from xdot import StructuredMask
    from xdot.parallel.layout import gathered_cols, global_rows

    B, n, R = 2, 3, 7
    spec = StructuredMask(**kw)
    cols = gathered_cols(LAYOUT, n, R)
    for rank in range(n):
        rows = global_rows(LAYOUT, rank, n, R)
        ref = _python_mask(B, rows.tolist(), cols.tolist(), kw.get("causal", False), kw.get("window"),
                           kw.get("lengths"), kw.get("doc_starts"))
        got = spec.dense_at(B, rows, cols)
        assert got.dtype == torch.bool and got.is_contiguous() and torch.equal(got, ref), (rank, kw)
        assert torch.equal(spec.dense_at(B, rows.tolist(), cols.tolist()), ref)
    # dense() is a call of it at consecutive rows and columns: unchanged, bit for bit
    for ro in (0, 5, 14):
        ref = _python_mask(B, list(range(ro, ro + R)), list(range(n * R)), kw.get("causal", False), kw.get("window"),
                           kw.get("lengths"), kw.get("doc_starts"))
        assert torch.equal(spec.dense(B, R, n * R, ro), ref), (ro, kw)
        assert torch.equal(StructuredMask(row_offset=ro, **kw).dense(B, R, n * R), ref)


def test_bind_runs_and_cache_key():
    from xdot import StructuredMask
    from xdot.parallel.layout import gathered_cols, row_runs

    spec = StructuredMask(causal=True)
    one = spec.bind([(0, 7, 14)], 21)
    assert one is spec.bind(14, 21) and one.row_offset == 14 and one._rows is None and one._cols is None
    runs = row_runs(LAYOUT, 0, 3, 7)
    cols = ((LAYOUT, 3, 7), gathered_cols(LAYOUT, 3, 7))
    two = spec.bind(runs, 21, cols)
    assert two is spec.bind(tuple(runs), 21, cols) and two is not one and two._rows == tuple(runs)
    assert two._cols.tolist() == cols[1].tolist() and two.row_offset is None
    # the last rank's rows are one run, its columns are still in zigzag order: a different object
    last = spec.bind(row_runs(LAYOUT, 2, 3, 7), 21, cols)
    assert last.row_offset == 8 and last._cols is not None and last is not spec.bind(8, 21)
    with pytest.raises(ValueError):
        StructuredMask(causal=True, row_offset=3).bind(runs, 21, cols)


def test_segments_follow_the_gathered_order():
    from xdot.ops.mask import expand_segments, segments_of
    from xdot.parallel.attention import _mask_cols, _perm_cols
    from xdot.parallel.layout import gathered_cols

    n, R = 3, 7
    cols = gathered_cols(LAYOUT, n, R)
    assert expand_segments(segments_of(None, n * R, cols)).tolist() == cols.tolist()
    assert segments_of(None, n * R) == [(0, n * R, 0)]
    for view in (_perm_cols(1, R, n, [(0, 4), (4, 3)]), _mask_cols(1, R, n, 1, 3, 2, 4)):
        want = view(cols.view(1, 1, -1)).reshape(-1)
        assert expand_segments(segments_of(view, n * R, cols)).tolist() == want.tolist()


# ---- the module on CPU ranks ----------------------------------------------------------------------
DIM, LENGTH = 16, 7  # odd rows per rank: h0 = 4, h1 = 3


def _masks(ws, B, g):
    """name -> (what the ranks pass (StructuredMask or full dense tensor), the full dense mask)."""
    from xdot import StructuredMask

    T = ws * LENGTH
    h0 = (LENGTH + 1) // 2
    specs = {
        "causal": StructuredMask(causal=True),
        "causal_window": StructuredMask(causal=True, window=5),
        # a boundary on a chunk boundary (h0: chunk 0 | chunk 1; ws * h0: the low | high chunks) and
        # strictly inside chunks (2, ws * h0 + 1)
        "docs": StructuredMask(causal=True, doc_starts=[2, h0, ws * h0, ws * h0 + 1]),
        "lengths": StructuredMask(lengths=[T - 2, T - 5][:B]),
    }
    out = {k: (s, s.dense(B, T, T, 0)) for k, s in specs.items()}
    dense = torch.rand(B, T, T, generator=g) < 0.35
    dense[..., torch.arange(T), torch.arange(T)] = False  # no fully-masked row
    out["dense"] = (dense, dense)
    return out


def _rank_parity(rank, ws, impl, chunks, rope, gathered_heads=None, names=None, tol=1e-9):
    """The bounds of tests/test_rope.py and tests/test_document_mask.py for the same comparison:
    1e-9 on outputs and input gradients, 1e-8 on the Sum-reduced parameter gradients (fp64)."""
    import xdot
    from xdot import DistributedDotProductAttn, Rotary
    from xdot.parallel import allreduce_gradients, broadcast_parameters

    dtype, B, H = torch.float64, 2, 4
    torch.manual_seed(100 + rank)
    kw = dict(num_heads=H, add_bias=True, num_gathered_heads=gathered_heads)
    model = DistributedDotProductAttn(DIM, impl=impl, chunk_plan=chunks, layout=LAYOUT,
                                      rope=Rotary() if rope else None, **kw).to(dtype)
    gt_model = DistributedDotProductAttn(DIM, distributed=False, impl="materialized",
                                         rope=Rotary() if rope else None, **kw).to(dtype)
    broadcast_parameters(model)
    gt_model.load_state_dict(model.state_dict())
    g = torch.Generator().manual_seed(7)
    T = LENGTH * ws
    x_full = torch.rand(B, T, DIM, generator=g, dtype=dtype)
    comm = xdot.get_comm()
    for name, (mask, dense) in _masks(ws, B, g).items():
        if names is not None and name not in names:
            continue
        model.zero_grad()
        gt_model.zero_grad()
        x = xdot.shard_rows(x_full, rank, ws, layout=LAYOUT).clone().requires_grad_(True)
        local = xdot.shard_rows(mask, rank, ws, layout=LAYOUT) if isinstance(mask, torch.Tensor) else mask
        out = model(x, x, x, local)
        out.sum().backward()
        xg = x_full.clone().requires_grad_(True)
        gt_out = gt_model(xg, xg, xg, dense)
        gt_out.sum().backward()
        outs = xdot.unshard_rows(comm.all_gather_object(out.detach()), layout=LAYOUT)
        dxs = xdot.unshard_rows(comm.all_gather_object(x.grad), layout=LAYOUT)
        torch.testing.assert_close(outs, gt_out.detach(), atol=tol, rtol=tol, msg=lambda m: f"{name} out: {m}")
        torch.testing.assert_close(dxs, xg.grad, atol=tol, rtol=tol, msg=lambda m: f"{name} dx: {m}")
        allreduce_gradients(model)
        for (n1, p1), (_n2, p2) in zip(gt_model.named_parameters(), model.named_parameters()):
            torch.testing.assert_close(p2.grad, p1.grad, atol=tol * 10, rtol=tol * 10,
                                       msg=lambda m: f"{name} d{n1}: {m}")


IMPLS = {"flash_whole": ("flash", 1), "flash_chunked": ("flash", 2), "ring": ("ring", None),
         "materialized": ("materialized", None)}


@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("impl", list(IMPLS))
@pytest.mark.parametrize("ws", [2, 3, 4])
def test_module_ranks(ws, impl, rope):
    """Inputs sharded with ``shard_rows``, outputs unsharded: every mask kind, every impl."""
    from xdot.utils.comm import ThreadGroup

    ThreadGroup(ws).run(lambda r: _rank_parity(r, ws, *IMPLS[impl], rope))


@pytest.mark.parametrize("impl", ["flash_chunked", "ring"])
def test_module_ranks_grouped_heads(impl):
    from xdot.utils.comm import ThreadGroup

    ThreadGroup(3).run(lambda r: _rank_parity(r, 3, *IMPLS[impl], True, gathered_heads=2))


@pytest.mark.parametrize("fused", [True, False])
def test_module_flash_per_op_graph(fused, monkeypatch):
    """The one-node module and the per-op graph of the flash path."""
    from xdot.utils.comm import ThreadGroup
    from xdot.utils.env import FLAGS

    monkeypatch.setattr(FLAGS, "fused_module", fused)
    ThreadGroup(3).run(lambda r: _rank_parity(r, 3, "flash", 2, True, names=("causal", "docs", "dense")))


def _gloo_case(rank, ws):
    _rank_parity(rank, ws, "flash", 2, True, names=("causal", "docs"))


def test_module_ranks_gloo():
    run_gloo(_gloo_case, 2)


def test_functional_entries_follow_the_layout():
    """seq_parallel_attention / ring_attention with rope and a StructuredMask, 3 ranks, against
    the contiguous one-rank call on the full sequence."""
    import xdot
    from xdot.parallel.ring import ring_attention
    from xdot.utils.comm import ThreadGroup

    ws, H, C = 3, 2, 8
    T = ws * LENGTH
    g = torch.Generator().manual_seed(3)
    k, q, v = (torch.randn(1, T, C, dtype=torch.float64, generator=g) for _ in range(3))
    spec = xdot.StructuredMask(causal=True, doc_starts=[5])
    want = xdot.seq_parallel_attention(k, q, v, spec, H, 0.5, comm=xdot.LocalComm(), rope=xdot.Rotary())
    want_plain = xdot.seq_parallel_attention(k, q, v, spec, H, 0.5, comm=xdot.LocalComm())

    def body(r):
        ks, qs, vs = (xdot.shard_rows(t, r, ws, layout=LAYOUT) for t in (k, q, v))
        a = xdot.seq_parallel_attention(ks, qs, vs, spec, H, 0.5, rope=xdot.Rotary(), layout=LAYOUT)
        b = ring_attention(ks, qs, vs, spec, H, 0.5, layout=LAYOUT)
        return a, b

    res = ThreadGroup(ws).run(body)
    torch.testing.assert_close(xdot.unshard_rows([a for a, _b in res], layout=LAYOUT), want, atol=1e-10, rtol=1e-10)
    torch.testing.assert_close(xdot.unshard_rows([b for _a, b in res], layout=LAYOUT), want_plain, atol=1e-10,
                               rtol=1e-10)


# ---- defaults, contradictions, consistency check ----------------------------------------------------
@pytest.mark.parametrize("impl", ["flash", "ring", "materialized"])
def test_contiguous_is_the_default_bit_for_bit(impl):
    import xdot
    from xdot.utils.comm import ThreadGroup

    def body(r):
        torch.manual_seed(0)
        a = xdot.DistributedDotProductAttn(DIM, num_heads=4, impl=impl, rope=xdot.Rotary()).double()
        b = xdot.DistributedDotProductAttn(DIM, num_heads=4, impl=impl, rope=xdot.Rotary(), layout="contiguous").double()
        b.load_state_dict(a.state_dict())
        assert repr(a) == repr(b) and "layout" not in repr(a)
        x = torch.rand(1, LENGTH, DIM, dtype=torch.float64, generator=torch.Generator().manual_seed(r))
        res = []
        for m in (a, b):
            xi = x.clone().requires_grad_(True)
            out = m(xi, xi, xi, xdot.StructuredMask(causal=True))
            out.sum().backward()
            res.append([out.detach(), xi.grad] + [p.grad for p in m.parameters()])
        for u, v in zip(*res):
            assert torch.equal(u, v)

    ThreadGroup(2).run(body)


def test_distributed_false_ignores_the_layout():
    import xdot

    torch.manual_seed(0)
    a = xdot.DistributedDotProductAttn(DIM, num_heads=4, distributed=False, impl="flash", rope=xdot.Rotary()).double()
    b = xdot.DistributedDotProductAttn(DIM, num_heads=4, distributed=False, impl="flash", rope=xdot.Rotary(offset=0),
                                       layout=LAYOUT).double()
    b.load_state_dict(a.state_dict())
    x = torch.rand(1, 9, DIM, dtype=torch.float64)
    spec = xdot.StructuredMask(causal=True, row_offset=0)  # explicit offsets are fine in a world of one
    assert torch.equal(a(x, x, x, spec), b(x, x, x, spec))
    assert "layout=zigzag" in repr(b)
    with pytest.raises(ValueError):
        xdot.DistributedDotProductAttn(DIM, layout="striped")


@pytest.mark.parametrize("impl", ["flash", "ring", "materialized"])
def test_explicit_offsets_contradict_zigzag(impl):
    import xdot
    from xdot.utils.comm import ThreadGroup

    def body(r):
        x = torch.rand(1, LENGTH, DIM, dtype=torch.float64)
        m = xdot.DistributedDotProductAttn(DIM, num_heads=4, impl=impl, layout=LAYOUT).double()
        with pytest.raises(ValueError, match="row_offset"):
            m(x, x, x, xdot.StructuredMask(causal=True, row_offset=r * LENGTH))
        m = xdot.DistributedDotProductAttn(DIM, num_heads=4, impl=impl, layout=LAYOUT,
                                           rope=xdot.Rotary(offset=r * LENGTH)).double()
        with pytest.raises(ValueError, match="offset"):
            m(x, x, x, None)

    ThreadGroup(2).run(body)
    with pytest.raises(ValueError):
        xdot.Rotary(offset=3).resolve(0, LENGTH, 1, LAYOUT)
    assert xdot.Rotary().resolve(1, LENGTH, 3, LAYOUT) == ((0, 4, 4), (4, 3, 15))
    assert xdot.Rotary().resolve(2, LENGTH, 3, LAYOUT) == 8 and xdot.Rotary().resolve(2, LENGTH) == 14


def test_rotary_table_of_runs():
    import xdot

    rot = xdot.Rotary()
    runs = ((0, 4, 4), (4, 3, 15))
    c, s = rot.table(7, 8, runs, "cpu", torch.float64)
    assert rot.table(7, 8, list(runs), "cpu", torch.float64)[0] is c  # cached on the runs
    for (ls, ln, gs) in runs:
        cr, sr = xdot.Rotary().table(ln, 8, gs, "cpu", torch.float64)
        assert torch.equal(c[ls:ls + ln], cr) and torch.equal(s[ls:ls + ln], sr)
    assert torch.equal(rot.table(7, 8, [(0, 7, 5)], "cpu")[0], rot.table(7, 8, 5, "cpu")[0])
    with pytest.raises(ValueError):
        rot.table(7, 8, ((0, 4, 4), (4, 2, 15)), "cpu")
    x = torch.rand(1, 7, 16, dtype=torch.float64)
    got = xdot.rope(x, 2, rot, offset=runs)
    want = torch.cat([xdot.rope(x[:, :4], 2, rot, offset=4), xdot.rope(x[:, 4:], 2, rot, offset=15)], dim=1)
    assert torch.equal(got, want)


@pytest.mark.parametrize("impl", ["flash", "ring"])
def test_check_raises_on_a_layout_mismatch(impl, monkeypatch):
    import xdot
    from xdot.utils.checks import RankDivergenceError
    from xdot.utils.comm import ThreadGroup
    from xdot.utils.env import FLAGS

    monkeypatch.setattr(FLAGS, "check", True)

    def body(r, layouts):
        x = torch.rand(1, LENGTH, DIM, dtype=torch.float64)
        m = xdot.DistributedDotProductAttn(DIM, num_heads=4, impl=impl, layout=layouts[r]).double()
        return m(x, x, x, xdot.StructuredMask(causal=True))

    with pytest.raises(RankDivergenceError, match="zigzag"):
        ThreadGroup(2).run(body, ("contiguous", LAYOUT))
    ThreadGroup(2).run(body, (LAYOUT, LAYOUT))
