"""Document masks of packed sequences (``StructuredMask(doc_starts=...)``) without a GPU: the
dense oracle against an element-wise construction, validation, the cache key, the defining
property (a packed row computes what each document computes alone) and the module on CPU ranks."""
import pytest
import torch

from _dist import run_gloo


def _independent(B, R, T, ro, causal=False, window=None, lengths=None, doc_starts=None):
    """Element by element from the definition; ``doc_starts``: a list (shared) or a list of B lists."""
    per_batch = bool(doc_starts) and isinstance(doc_starts[0], (list, tuple))
    m = torch.zeros(B, R, T, dtype=torch.bool)
    for b in range(B):
        starts = [] if doc_starts is None else (doc_starts[b] if per_batch else doc_starts)

        def doc(x):
            return sum(s <= x for s in starts)

        for r in range(R):
            gr = ro + r
            for gc in range(T):
                masked = causal and gc > gr
                if window is not None:
                    masked = masked or gc < gr - (window - 1) or (not causal and gc > gr + (window - 1))
                if lengths is not None:
                    masked = masked or gc >= lengths[b]
                masked = masked or doc(gc) != doc(gr)
                m[b, r, gc] = masked
    return m


# (B, R, T, row_offset, doc_starts)
DOC_CASES = [
    (1, 12, 12, 0, [0, 5, 9]),                       # first start 0
    (1, 12, 12, 0, [4, 9]),                          # first start > 0: position 0 begins a document anyway
    (2, 9, 30, 0, [3, 3, 3, 10, 10, 22]),            # duplicates = empty documents
    (1, 8, 20, 0, [6, 20, 25, 1000]),                # starts >= T have no effect
    (1, 8, 20, 0, []),                               # n = 0: one document
    (1, 10, 10, 0, [2, 3, 4, 5, 9]),                 # one-row documents
    (2, 7, 24, 0, [[5, 11, 11], [8, 24, 24]]),       # per batch, padded by repeating / by T
    (2, 6, 40, 30, [[5, 33], [31, 34]]),             # per batch, nonzero row offset
    (1, 5, 15, 5, [7, 12]),                          # the middle rank of 3
    (2, 6, 0, 0, [1]),                               # no columns
]
RULES = [dict(), dict(causal=True), dict(causal=True, window=4), dict(window=5), dict(lengths=True),
         dict(causal=True, lengths=True), dict(causal=True, window=3, lengths=True)]


@pytest.mark.parametrize("case", DOC_CASES, ids=lambda c: "x".join(map(str, c[:4])) + "-" + str(c[4]).replace(" ", ""))
def test_dense_matches_independent_construction(case):
    from xdot import StructuredMask

    B, R, T, ro, starts = case
    for rule in RULES:
        kw = dict(rule)
        if kw.pop("lengths", False):
            kw["lengths"] = [max(0, T - 3 - 9 * b) for b in range(B)]
        ref = _independent(B, R, T, ro, doc_starts=starts, **kw)
        assert torch.equal(StructuredMask(doc_starts=starts, **kw).dense(B, R, T, ro), ref), kw
        assert torch.equal(StructuredMask(row_offset=ro, doc_starts=starts, **kw).dense(B, R, T), ref), kw
        for dt in (torch.int32, torch.int64):  # as a tensor
            t = torch.tensor(starts, dtype=dt)
            assert torch.equal(StructuredMask(doc_starts=t, **kw).dense(B, R, T, ro), ref), (kw, dt)
        if not starts:  # n = 0 is doc_starts=None
            assert torch.equal(StructuredMask(**kw).dense(B, R, T, ro), ref), kw


def test_documents_restrict_an_existing_mask():
    """Adding documents only ever masks more, and never the diagonal of an unpadded row."""
    from xdot import StructuredMask

    T = 20
    base = StructuredMask(causal=True).dense(1, T, T, 0)
    docs = StructuredMask(causal=True, doc_starts=[6, 13]).dense(1, T, T, 0)
    assert (docs | base).equal(docs) and not docs[0].diagonal().any()
    assert not docs[0, 12, 6:13].any() and docs[0, 12, :6].all() and docs[0, 13, :13].all()


def test_from_doc_lengths():
    from xdot import StructuredMask

    s = StructuredMask.from_doc_lengths([5, 4, 0, 3], causal=True)
    assert s.causal and s.doc_starts.tolist() == [0, 5, 9, 9]
    assert torch.equal(s.dense(1, 12, 12, 0), StructuredMask(causal=True, doc_starts=[0, 5, 9, 9]).dense(1, 12, 12, 0))
    s2 = StructuredMask.from_doc_lengths(torch.tensor([[5, 7], [2, 10]], dtype=torch.int32), lengths=[12, 12], row_offset=3)
    assert s2.doc_starts.tolist() == [[0, 5], [0, 2]] and s2.row_offset == 3 and s2.lengths.tolist() == [12, 12]
    assert not s2.doc_starts.is_floating_point()
    with pytest.raises(TypeError):
        StructuredMask.from_doc_lengths([1, 2], doc_starts=[0, 1])
    with pytest.raises(ValueError):
        StructuredMask.from_doc_lengths([1.5, 2.0])
    with pytest.raises(ValueError):
        StructuredMask.from_doc_lengths([3, -1])


def test_positional_arguments_keep_working():
    from xdot import StructuredMask

    s = StructuredMask(True, 3, [4], 2)
    assert (s.causal, s.window, s.lengths.tolist(), s.row_offset, s.doc_starts) == (True, 3, [4], 2, None)
    s = StructuredMask(True, None, None, None, [2, 4])
    assert s.doc_starts.tolist() == [2, 4]


def test_validation():
    from xdot import DistributedDotProductAttn, StructuredMask, seq_parallel_attention
    from xdot.utils.comm import LocalComm

    for bad in (torch.zeros(3), torch.zeros(3, dtype=torch.bool), torch.zeros(3, dtype=torch.complex64),
                [0.5, 2.0],                                    # floating / bool / complex
                torch.zeros((), dtype=torch.int64), torch.zeros(1, 2, 3, dtype=torch.int64), [[[1]]],  # rank
                [3, -1], torch.tensor([-2, 4]), [[0, 1], [-1, 2]],           # negative
                [5, 3], torch.tensor([0, 7, 6]), [[0, 1], [4, 2]]):          # decreasing
        with pytest.raises(ValueError):
            StructuredMask(doc_starts=bad)
    StructuredMask(doc_starts=[3, 3, 3])            # duplicates are fine
    StructuredMask(doc_starts=[[], []])             # (B, 0)
    StructuredMask(doc_starts=[[5, 6], [0, 1]])     # order is per row
    spec = StructuredMask(doc_starts=[[1, 2], [3, 4], [5, 6]])
    with pytest.raises(ValueError):
        spec.check(2)
    with pytest.raises(ValueError):
        spec.dense(2, 4, 8, 0)
    spec.check(3)
    StructuredMask(doc_starts=[1, 2]).check(7)      # a shared table serves any batch
    x = torch.randn(2, 4, 8)
    for impl in ("flash", "ring", "materialized"):
        m = DistributedDotProductAttn(8, num_heads=2, impl=impl, distributed=False)
        with pytest.raises(ValueError):
            m(x, x, x, spec)
    with pytest.raises(ValueError):
        seq_parallel_attention(x, x, x, spec, 2, 1.0, comm=LocalComm())


def test_immutable_repr_slots():
    from xdot import StructuredMask

    s = StructuredMask(causal=True, doc_starts=[2, 5])
    with pytest.raises(AttributeError):
        s.doc_starts = None
    with pytest.raises(AttributeError):
        s.other = 1
    assert "doc_starts" in StructuredMask.__slots__ and not hasattr(s, "__dict__")
    assert repr(StructuredMask(causal=True, window=4, row_offset=2)) == \
        "StructuredMask(causal=True, window=4, lengths=None, row_offset=2)"
    assert repr(StructuredMask(lengths=[3, 4])) == \
        "StructuredMask(causal=False, window=None, lengths=<2 lengths on cpu>, row_offset=None)"
    assert "doc_starts" in repr(s)


def test_bind_and_version():
    from xdot import StructuredMask

    ds, ln = torch.tensor([[2, 5], [3, 3]]), torch.tensor([8, 7])
    spec = StructuredMask(causal=True, lengths=ln, doc_starts=ds)
    a = spec.bind(8, 32)
    assert a is spec.bind(8, 32) and a.doc_starts is ds and a.lengths is ln and a.row_offset == 8
    assert torch.equal(a.dense(2, 4, 32), spec.dense(2, 4, 32, 8))
    v0 = a._version
    assert a._version == v0
    ds[0, 1] = 6
    v1 = a._version
    assert v1 != v0
    ln.add_(1)
    v2 = a._version
    assert v2 != v1 and v2 != v0
    only_docs = StructuredMask(doc_starts=ds)
    v = only_docs._version
    ds.add_(1)
    assert only_docs._version != v
    dd = a.device_doc_starts("cpu")
    assert dd.dtype == torch.int32 and dd.is_contiguous() and dd.tolist() == ds.tolist()
    big = StructuredMask(doc_starts=torch.tensor([1, 2**40])).device_doc_starts("cpu")
    assert big.tolist() == [1, 2**31 - 1]
    assert StructuredMask().device_doc_starts("cpu") is None and StructuredMask(doc_starts=[]).device_doc_starts("cpu") is None


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", ["flash", "ring", "materialized"])
def test_packed_documents_compute_what_each_document_computes_alone(impl):
    """The defining property: three documents of unequal length packed into one row, causal."""
    from xdot import DistributedDotProductAttn, StructuredMask

    dim, lens, tol = 16, [5, 2, 6], 1e-9  # tests/test_structured_mask.py's fp64 module tolerance
    torch.manual_seed(3)
    m = DistributedDotProductAttn(dim, num_heads=2, impl=impl, distributed=False).to(torch.float64)
    x = torch.rand(1, sum(lens), dim, dtype=torch.float64)
    with torch.no_grad():
        packed = m(x, x, x, StructuredMask.from_doc_lengths(lens, causal=True))
        at = 0
        for n in lens:
            xd = x[:, at:at + n]
            alone = m(xd, xd, xd, StructuredMask(causal=True))
            torch.testing.assert_close(packed[:, at:at + n], alone, atol=tol, rtol=tol)
            at += n
        plain = m(x, x, x, StructuredMask(causal=True))
    assert not torch.allclose(packed[:, lens[0]:], plain[:, lens[0]:], atol=1e-6)  # the boundary does something


def _module_docs(rank, ws, impl, length=6, dim=16):
    """tests/test_structured_mask.py's ``_module_causal`` with documents: a boundary strictly inside
    rank 0's rows (3), one exactly at the rank boundary (6), one inside rank 1 (10)."""
    from xdot import DistributedDotProductAttn, StructuredMask
    from xdot.parallel import allreduce_gradients, broadcast_parameters, gather_sequence

    dtype, tol = torch.float64, 1e-9
    torch.manual_seed(100 + rank)
    model = DistributedDotProductAttn(dim, num_heads=2, impl=impl).to(dtype)
    gt_model = DistributedDotProductAttn(dim, num_heads=2, distributed=False, impl="materialized").to(dtype)
    broadcast_parameters(model)
    gt_model.load_state_dict(model.state_dict())
    T = length * ws
    g = torch.Generator().manual_seed(7)
    x_full = torch.rand(1, T, dim, generator=g, dtype=dtype)
    spec = StructuredMask(causal=True, doc_starts=[3, length, T - 2])
    mask_full = spec.dense(1, T, T, 0)
    sl = slice(rank * length, (rank + 1) * length)

    def run(mask):
        model.zero_grad()
        x = x_full[:, sl].clone().requires_grad_(True)
        out = model(x, x, x, mask)
        out.sum().backward()
        return out.detach(), x.grad, [p.grad.clone() for p in model.parameters()]

    out_s, dx_s, gp_s = run(spec)
    out_d, dx_d, gp_d = run(mask_full[:, sl])
    for a, b in zip([out_s, dx_s] + gp_s, [out_d, dx_d] + gp_d):
        assert torch.equal(a, b)
    xg = x_full.clone().requires_grad_(True)
    gt_out = gt_model(xg, xg, xg, mask_full)
    gt_out.sum().backward()
    torch.testing.assert_close(gather_sequence(out_s, -2), gt_out.detach(), atol=tol, rtol=tol)
    torch.testing.assert_close(gather_sequence(dx_s, -2), xg.grad, atol=tol, rtol=tol)
    allreduce_gradients(model)
    for p1, p2 in zip(gt_model.parameters(), model.parameters()):
        torch.testing.assert_close(p2.grad, p1.grad, atol=tol * 10, rtol=tol * 10)


@pytest.mark.parametrize("impl", ["flash", "ring", "materialized"])
def test_module_two_ranks_threads(impl):
    from xdot.utils.comm import ThreadGroup

    ThreadGroup(2).run(lambda r: _module_docs(r, 2, impl))


def test_module_two_ranks_gloo():
    run_gloo(_module_docs, 2, "flash")


def test_seq_parallel_attention_and_torch_backend():
    """The functional entry point and ``backend="torch"`` take the description through ``dense()``."""
    from xdot import DistributedDotProductAttn, StructuredMask, seq_parallel_attention
    from xdot.utils.comm import LocalComm

    B, T, H, D = 2, 10, 2, 4
    g = torch.Generator().manual_seed(2)
    q, k, v = (torch.randn(B, T, H * D, generator=g, dtype=torch.float64) for _ in range(3))
    spec = StructuredMask(causal=True, doc_starts=[[4, 7], [1, 10]])
    got = seq_parallel_attention(q, k, v, spec, H, 0.5, comm=LocalComm())
    ref = seq_parallel_attention(q, k, v, spec.dense(B, T, T, 0), H, 0.5, comm=LocalComm())
    assert torch.equal(got, ref)
    m = DistributedDotProductAttn(H * D, num_heads=H, distributed=False, backend="torch").to(torch.float64)
    assert torch.equal(m(q, q, q, spec), m(q, q, q, spec.dense(B, T, T, 0)))
