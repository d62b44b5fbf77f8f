"""xdot.StructuredMask without a GPU: the dense oracle against an independent construction, the
column segment tables of every mask view, the module on CPU ranks, argument validation."""
import pytest
import torch

from _dist import run_gloo


def _spec_args(B, T):
    ln = [max(0, T - 13 - 40 * b) for b in range(B)]
    return [dict(causal=True), dict(causal=True, window=5), dict(window=70), dict(lengths=ln),
            dict(causal=True, lengths=ln), dict(window=1), dict()]


def _independent(B, R, T, ro, causal=False, window=None, lengths=None):
    """Element by element from the definition (no broadcasting tricks shared with dense())."""
    m = torch.zeros(B, R, T, dtype=torch.bool)
    for b in range(B):
        for r in range(R):
            gr = ro + r
            for gc in range(T):
                masked = causal and gc > gr
                if window is not None:
                    masked = masked or gc < gr - (window - 1) or (not causal and gc > gr + (window - 1))
                if lengths is not None:
                    masked = masked or gc >= lengths[b]
                m[b, r, gc] = masked
    return m


@pytest.mark.parametrize("shape", [(1, 7, 21, 0), (2, 9, 90, 0), (1, 5, 15, 5), (2, 6, 100, 80)])
def test_dense_matches_independent_construction(shape):
    from xdot import StructuredMask

    B, R, T, ro = shape
    for kw in _spec_args(B, T):
        ref = _independent(B, R, T, ro, **kw)
        assert torch.equal(StructuredMask(**kw).dense(B, R, T, ro), ref), kw
        assert torch.equal(StructuredMask(row_offset=ro, **kw).dense(B, R, T), ref), kw
        if "lengths" in kw:  # a tensor of lengths
            kt = dict(kw, lengths=torch.tensor(kw["lengths"], dtype=torch.int32))
            assert torch.equal(StructuredMask(**kt).dense(B, R, T, ro), ref), kw


def test_arange_construction_of_causal_and_padding():
    from xdot import StructuredMask

    B, R, T, ro = 2, 8, 24, 8
    gr = ro + torch.arange(R)[:, None]
    gc = torch.arange(T)[None, :]
    ln = torch.tensor([24, 10])
    causal = (gc > gr).expand(B, R, T)
    assert torch.equal(StructuredMask(causal=True).dense(B, R, T, ro), causal)
    assert torch.equal(StructuredMask(causal=True, lengths=ln).dense(B, R, T, ro), causal | (gc[None] >= ln[:, None, None]))
    band = (gc - gr).abs() > 2
    assert torch.equal(StructuredMask(window=3).dense(1, R, T, ro), band[None])


def _views():
    from xdot.parallel import attention as pa
    from xdot.parallel.ring import _block_mask

    n, R, rank, h = 3, 96, 1, 40
    chunks = [(0, 48), (48, 48)]

    def own_excluded(m):
        m = pa._mask_cols(1, R, n, 0, n, 48, 48)(m).clone()
        m[..., rank * 48:(rank + 1) * 48] = True if m.dtype == torch.bool else -1
        return m

    return n * R, {
        "identity": None,
        "mask_cols_peer": pa._mask_cols(1, R, n, 2, 3, 48, 48),
        "mask_cols_chunk": pa._mask_cols(1, R, n, 0, n, 0, 48),
        "perm_cols": pa._perm_cols(1, R, n, chunks),
        "own_excluded": own_excluded,
        "ring_merged": lambda m: torch.cat([_block_mask(m, 0, R, 0, h), _block_mask(m, 2, R, h, R)], -1),
    }


@pytest.mark.parametrize("vname", ["identity", "mask_cols_peer", "mask_cols_chunk", "perm_cols", "own_excluded",
                                   "ring_merged"])
def test_segments_round_trip(vname):
    from xdot.ops.mask import expand_segments, segments_of

    T, views = _views()
    view = views[vname]
    idx = torch.arange(T, dtype=torch.int64).view(1, 1, T)
    row = (idx if view is None else view(idx)).reshape(-1)
    segs = segments_of(view, T)
    assert torch.equal(expand_segments(segs), row)
    # back to back, maximal runs
    at = 0
    for p, ln, g in segs:
        assert p == at and ln > 0 and g >= -1
        at += ln
    assert at == row.numel()
    for (p0, l0, g0), (_p1, _l1, g1) in zip(segs, segs[1:]):
        assert not (g0 >= 0 and g1 == g0 + l0) and not (g0 < 0 and g1 < 0)
    expect = {"identity": 1, "mask_cols_peer": 1, "mask_cols_chunk": 3, "perm_cols": 6, "own_excluded": 3,
              "ring_merged": 2}
    assert len(segs) == expect[vname]


def test_views_keep_bool_results():
    """The generalised view helpers on a (B, R, T) bool tensor: the reshapes they used to spell out."""
    from xdot.parallel import attention as pa

    B, R, n = 2, 6, 3
    g = torch.Generator().manual_seed(0)
    m = torch.rand(B, R, n * R, generator=g) < 0.5
    assert torch.equal(pa._mask_cols(B, R, n, 1, 3, 2, 3)(m), m.reshape(B, R, n, R)[..., 1:3, 2:5].reshape(B, R, 6))
    chunks = [(0, 4), (4, 2)]
    old = torch.cat([m.reshape(B, R, n, R)[..., r0:r0 + rc].reshape(B, R, n * rc) for r0, rc in chunks], dim=-1)
    assert torch.equal(pa._perm_cols(B, R, n, chunks)(m), old)


def _module_causal(rank, ws, impl, length=6, dim=16):
    from xdot import DistributedDotProductAttn, StructuredMask
    from xdot.parallel import allreduce_gradients, broadcast_parameters, gather_sequence

    dtype, tol = torch.float64, 1e-9  # tests/test_gradient.py's fp64 tolerances
    torch.manual_seed(100 + rank)
    model = DistributedDotProductAttn(dim, num_heads=2, impl=impl).to(dtype)
    gt_model = DistributedDotProductAttn(dim, num_heads=2, distributed=False, impl="materialized").to(dtype)
    broadcast_parameters(model)
    gt_model.load_state_dict(model.state_dict())
    T = length * ws
    g = torch.Generator().manual_seed(7)
    x_full = torch.rand(1, T, dim, generator=g, dtype=dtype)
    mask_full = torch.arange(T)[None, :] > torch.arange(T)[:, None]   # hand-built causal, (T, T)
    sl = slice(rank * length, (rank + 1) * length)

    def run(mask):
        model.zero_grad()
        x = x_full[:, sl].clone().requires_grad_(True)
        out = model(x, x, x, mask)
        out.sum().backward()
        return out.detach(), x.grad, [p.grad.clone() for p in model.parameters()]

    out_s, dx_s, gp_s = run(StructuredMask(causal=True))
    out_d, dx_d, gp_d = run(mask_full[None, sl])
    for a, b in zip([out_s, dx_s] + gp_s, [out_d, dx_d] + gp_d):
        assert torch.equal(a, b)
    xg = x_full.clone().requires_grad_(True)
    gt_out = gt_model(xg, xg, xg, mask_full[None])
    gt_out.sum().backward()
    torch.testing.assert_close(gather_sequence(out_s, -2), gt_out.detach(), atol=tol, rtol=tol)
    torch.testing.assert_close(gather_sequence(dx_s, -2), xg.grad, atol=tol, rtol=tol)
    allreduce_gradients(model)
    for p1, p2 in zip(gt_model.parameters(), model.parameters()):
        torch.testing.assert_close(p2.grad, p1.grad, atol=tol * 10, rtol=tol * 10)


@pytest.mark.parametrize("impl", ["flash", "ring", "materialized"])
def test_module_two_ranks_threads(impl):
    from xdot.utils.comm import ThreadGroup

    ThreadGroup(2).run(lambda r: _module_causal(r, 2, impl))


def test_module_two_ranks_gloo():
    run_gloo(_module_causal, 2, "flash")


def test_argument_validation():
    from xdot import DistributedDotProductAttn, StructuredMask, seq_parallel_attention
    from xdot.utils.comm import LocalComm

    with pytest.raises(ValueError):
        StructuredMask(window=0)
    with pytest.raises(ValueError):
        StructuredMask(causal=True, window=-3)
    with pytest.raises(ValueError):
        StructuredMask(lengths=torch.zeros(2, 2, dtype=torch.int64))
    with pytest.raises(ValueError):
        StructuredMask(lengths=torch.zeros(2))
    with pytest.raises(ValueError):
        StructuredMask(lengths=[3, 4, 5]).dense(2, 4, 8, 0)
    with pytest.raises(ValueError):
        StructuredMask(causal=True).dense(1, 4, 8)  # no row offset anywhere
    with pytest.raises(AttributeError):
        StructuredMask().causal = True
    x = torch.randn(2, 4, 8)
    for impl in ("flash", "ring", "materialized"):
        m = DistributedDotProductAttn(8, num_heads=2, impl=impl, distributed=False)
        with pytest.raises(ValueError):
            m(x, x, x, StructuredMask(lengths=[4, 4, 4]))
    with pytest.raises(ValueError):
        seq_parallel_attention(x, x, x, StructuredMask(lengths=[4]), 2, 1.0, comm=LocalComm())


def test_fully_masked_row_matches_dense():
    """lengths[b] == 0: the NaN rows of the equivalent dense mask."""
    from xdot import DistributedDotProductAttn, StructuredMask

    x = torch.randn(2, 4, 16)
    spec = StructuredMask(lengths=[0, 3])
    for impl in ("materialized", "flash", "ring"):
        m = DistributedDotProductAttn(16, num_heads=2, impl=impl)
        y = m(x, x, x, spec)
        torch.testing.assert_close(y, m(x, x, x, spec.dense(2, 4, 4, 0)), rtol=0, atol=0, equal_nan=True)
        assert torch.isnan(y[0]).all() and not torch.isnan(y[1]).any()


def test_cache_key():
    from xdot import StructuredMask

    ln = torch.tensor([3, 4])
    spec = StructuredMask(causal=True, lengths=ln)
    a = spec.bind(8, 32)
    assert a is spec.bind(8, 32) and a is not spec.bind(16, 32)
    assert a.row_offset == 8 and a.lengths is ln and spec.row_offset is None
    v = a._version
    ln.add_(1)
    assert a._version != v
    assert StructuredMask(row_offset=5).bind(8, 32).row_offset == 5  # an explicit offset wins
