"""Attention sinks on the CPU paths: the fold identities against autograd of the definition, the
rounding model of ``tests/_sink_ref.py`` against an emulation of the kernels (and against six wrong
algorithms), and the module with ``sinks=True`` on every ``impl`` over in-process ranks against the
single-device module and the dense definition."""
import math

import pytest
import torch

import _sink_ref as ref
from _sink_ref import BF16, DT_IDS, F32, FP16, NINF

DIM = 64
LENGTH = 6
F64 = torch.float64


def _local():
    from xdot.utils.comm import LocalComm

    return LocalComm()


def _problem(B=2, H=3, R=5, T=5, D=4, Hg=None, seed=0, dead=True):
    gen = torch.Generator().manual_seed(seed)
    k = torch.randn(B, R, H * D, dtype=F64, generator=gen)
    q = torch.randn(B, T, (Hg or H) * D, dtype=F64, generator=gen)
    v = torch.randn(B, T, (Hg or H) * D, dtype=F64, generator=gen)
    mask = torch.rand(B, R, T, generator=gen) < 0.4
    mask[..., 0] = False
    if dead:
        mask[0, 2, :] = True  # a fully masked row
    s = torch.randn(H, dtype=F64, generator=gen)
    do = torch.randn(B, R, H * D, dtype=F64, generator=gen)
    return k, q, v, mask, s, do


def _grads(fn, *ts):
    ts = [t.detach().clone().requires_grad_(True) for t in ts]
    return fn(*ts), ts


# ---------------------------------------------------------------------------------- identities
@pytest.mark.parametrize("path", ["flash", "ring"])
@pytest.mark.parametrize("Hg", [None, 1])
def test_identities_against_autograd_of_the_definition(path, Hg):
    """lse' = logaddexp(lse, s), o' = exp(lse - lse') o, the unchanged backward on (o', lse') and
    ds = -sum exp(s - lse') delta' against autograd of softmax(cat([scores, s]))[..., :T] @ v in
    fp64: a random mask, one fully masked row, B = 2.  Plain attention has a NaN there; with sinks
    nothing is NaN."""
    from xdot.parallel.attention import seq_parallel_attention
    from xdot.parallel.ring import ring_attention

    H, D = 3, 4
    k, q, v, mask, s, do = _problem(H=H, D=D, Hg=Hg)
    scale = 1.0 / math.sqrt(D)
    want, wt = _grads(lambda k, q, v, s: ref.definition(k, q, v, mask, H, scale, s, Hg), k, q, v, s)
    want.backward(do)
    if path == "flash":
        fn = lambda k, q, v, s: seq_parallel_attention(k, q, v, mask, H, scale, comm=_local(), gathered_heads=Hg, sinks=s)
    else:
        fn = lambda k, q, v, s: ring_attention(k, q, v, mask, H, scale, comm=_local(), gathered_heads=Hg, sinks=s)
    got, gt = _grads(fn, k, q, v, s)
    got.backward(do)
    assert bool(torch.isfinite(got).all())
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    for a, b, n in zip(gt, wt, ("dk", "dq", "dv", "ds")):
        assert a.grad is not None and bool(torch.isfinite(a.grad).all()), n
        torch.testing.assert_close(a.grad, b.grad, rtol=1e-12, atol=1e-12, msg=lambda m: f"{n}: {m}")
    plain = seq_parallel_attention(k, q, v, mask, H, scale, comm=_local(), gathered_heads=Hg)
    assert bool(torch.isnan(plain[0, 2]).all()) and bool(torch.equal(got[0, 2], torch.zeros_like(got[0, 2])))


def test_the_formulas_on_their_own():
    """The four formulas written out on (o, lse) of plain attention, without xdot's functions."""
    from xdot.parallel import _ref

    H, D = 3, 4
    k, q, v, mask, s, do = _problem(H=H, D=D)
    scale = 1.0 / math.sqrt(D)
    want, wt = _grads(lambda k, q, v, s: ref.definition(k, q, v, mask, H, scale, s), k, q, v, s)
    want.backward(do)
    o, lse = _ref.block_fwd(k, q, v, mask, H, scale)
    l2 = torch.logaddexp(lse, s.view(1, H, 1))
    g = torch.sigmoid(lse - s.view(1, H, 1))
    o2 = (o.view(2, 5, H, D) * g.transpose(1, 2).unsqueeze(-1)).reshape(2, 5, H * D)
    torch.testing.assert_close(o2, want.detach(), rtol=1e-12, atol=1e-12)
    delta = _ref.delta(do, o2, H, F64)
    dk, dq, dv = _ref.block_bwd(do, k, q, v, l2, delta, mask, H, scale)
    ds = -(torch.exp(s.view(1, H, 1) - l2) * delta).sum(dim=(0, 2))
    for a, b in zip((dk, dq, dv, ds), wt):
        torch.testing.assert_close(a, b.grad, rtol=1e-12, atol=1e-12)
    # and xdot's torch functions are these formulas
    fo, fl = _ref.sink_fold(o, lse, s, H)
    torch.testing.assert_close(fo, o2, rtol=1e-14, atol=1e-14)
    torch.testing.assert_close(fl, l2, rtol=1e-14, atol=0)
    torch.testing.assert_close(_ref.sink_grad(delta, l2, s), ds, rtol=1e-13, atol=1e-14)


@pytest.mark.parametrize("path", ["flash", "ring"])
def test_gradcheck_of_the_torch_path(path):
    from xdot.parallel.attention import seq_parallel_attention
    from xdot.parallel.ring import ring_attention

    H, D = 2, 3
    k, q, v, mask, s, _ = _problem(B=1, H=H, R=4, T=4, D=D, seed=3)
    f = seq_parallel_attention if path == "flash" else ring_attention
    fn = lambda k, q, v, s: f(k, q, v, mask, H, 0.7, comm=_local(), sinks=s)
    ins = [t.clone().requires_grad_(True) for t in (k, q, v, s)]
    assert torch.autograd.gradcheck(fn, ins, eps=1e-6, atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize("path", ["flash", "ring"])
def test_minus_inf_is_no_sink_and_large_logits_stay_finite(path):
    from xdot.parallel.attention import seq_parallel_attention
    from xdot.parallel.ring import ring_attention

    H, D = 3, 4
    k, q, v, mask, s, do = _problem(H=H, D=D, dead=False)
    f = seq_parallel_attention if path == "flash" else ring_attention

    def run(sinks):
        kk, qq, vv = (t.clone().requires_grad_(True) for t in (k, q, v))
        out = f(kk, qq, vv, mask, H, 0.5, comm=_local(), **({} if sinks is None else {"sinks": sinks}))
        out.backward(do)
        return [out.detach(), kk.grad, qq.grad, vv.grad]

    base = run(None)
    off = torch.full((H,), NINF, dtype=F64, requires_grad=True)
    for a, b in zip(run(off), base):
        assert torch.equal(a, b)
    assert bool((off.grad == 0).all())
    for val in (200.0, -200.0):
        sk = torch.full((H,), val, dtype=F64, requires_grad=True)
        res = run(sk)
        assert all(bool(torch.isfinite(t).all()) for t in res) and bool(torch.isfinite(sk.grad).all())
    # a fully masked row with a sink of -inf stays what it was (NaN), as without the argument
    mask2 = mask.clone()
    mask2[1, 1] = True
    a = f(k, q, v, mask2, H, 0.5, comm=_local(), sinks=off.detach())
    b = f(k, q, v, mask2, H, 0.5, comm=_local())
    assert torch.equal(torch.isnan(a), torch.isnan(b)) and bool(torch.isnan(a[1, 1]).all())


def test_shift_property():
    """A constant added to all scores of a head's rows and to its sink leaves the output unchanged:
    in the definition, and in the fold (lse shifts with the scores)."""
    from xdot.parallel import _ref

    gen = torch.Generator().manual_seed(1)
    B, H, R, T, D = 2, 3, 4, 6, 5
    sc = torch.randn(B, H, R, T, dtype=F64, generator=gen)
    v = torch.randn(B, H, T, D, dtype=F64, generator=gen)
    s = torch.randn(H, dtype=F64, generator=gen)
    c = torch.tensor([3.0, -7.5, 40.0], dtype=F64)
    torch.testing.assert_close(ref.attend(sc + c.view(1, H, 1, 1), s + c, v), ref.attend(sc, s, v), rtol=1e-12, atol=1e-13)
    o = torch.randn(B, R, H * D, dtype=F64, generator=gen)
    lse = torch.randn(B, H, R, dtype=F64, generator=gen)
    o1, l1 = _ref.sink_fold(o, lse, s, H)
    o2, l2 = _ref.sink_fold(o, lse + c.view(1, H, 1), s + c, H)
    torch.testing.assert_close(o2, o1, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(l2, l1 + c.view(1, H, 1), rtol=1e-12, atol=1e-12)
    # the logit is NOT scaled: the function's scale multiplies the scores only
    from xdot.parallel.attention import seq_parallel_attention

    k, q, vv, mask, sk, _ = _problem(H=H, D=4)
    a = seq_parallel_attention(k, q, vv, mask, H, 0.25, comm=_local(), sinks=sk)
    b = seq_parallel_attention(k * 0.25, q, vv, mask, H, 1.0, comm=_local(), sinks=sk)
    torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-13)


# ---------------------------------------------------------------------------------- model and emulation
EMU_SHAPES = [(1, 1, 1, 32), (2, 37, 3, 96), (1, 130, 8, 96), (1, 65, 2, 160), (1, 33, 1, 384), (1, 2100, 2, 32)]


def _emu_case(shape, dtype, gap, sink_dtype=F32, seed=0):
    B, R, H, D = shape
    out, lse, sinks = ref.fold_inputs(B, R, H, D, dtype, seed=seed, gap=gap, sink_dtype=sink_dtype)
    gen = torch.Generator().manual_seed(seed + 1)
    dout = torch.randn(B, R, H * D, generator=gen).to(dtype)
    return out, lse, sinks, dout


def _emu_ratios(shape, dtype, gap, fbug=None, gbug=None, delta_from="folded", sink_dtype=F32):
    """(o', lse', ds) errors of the emulation in units of the unit bounds."""
    B, R, H, D = shape
    out, lse, sinks, dout = _emu_case(shape, dtype, gap, sink_dtype)
    o64, l64, g, x = ref.ref_fold(out, lse, sinks, H)
    bo, bl = ref.fold_bounds(o64, l64, g, x, dtype)
    o2, l2 = ref.emulate_fold(out, lse, sinks, H, bug=fbug, scale=1.0 / math.sqrt(D))
    ro, rl = ref.ratio(o2, o64, bo), ref.ratio(l2, l64, bl)
    # ds from the CORRECT folded pair (the backward's inputs as stored), whatever the forward's bug
    good_o, good_l = ref.emulate_fold(out, lse, sinks, H)
    src = good_o if delta_from == "folded" else out
    finite = lambda t: torch.where(torch.isnan(t), torch.zeros_like(t), t)
    delta = ref.delta64(dout, finite(src.float()), H).float()
    want, term, gapv = ref.ref_grad(ref.delta64(dout, finite(good_o.float()), H).float(), good_l, sinks)
    ds = ref.emulate_grad(delta, good_l, sinks, bug=gbug)
    return ro, rl, ref.ratio(ds, want, ref.grad_bound(term, gapv, B, R))


@pytest.mark.parametrize("dtype", [F32, BF16, FP16], ids=DT_IDS.get)
@pytest.mark.parametrize("shape", EMU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_model_holds_the_emulation(shape, dtype):
    """The kernels' algorithm, emulated in fp32 torch in their order of operations, stays inside F
    times the unit bounds: o', lse' and ds, with |lse - s| up to 6 and up to 200, fp32 and 16-bit sinks."""
    for gap, sdt in ((6.0, F32), (200.0, F32), (6.0, dtype)):
        ro, rl, rd = _emu_ratios(shape, dtype, gap, sink_dtype=sdt)
        print(f"RATIO emulation {DT_IDS[dtype]} {shape} gap={gap:g} sinks={DT_IDS[sdt]}: o' {ro:.2f} lse' {rl:.2f} ds {rd:.2f}")
        assert ro <= ref.F and rl <= ref.F and rd <= ref.F, (ro, rl, rd)


@pytest.mark.parametrize("dtype", [F32, BF16, FP16], ids=DT_IDS.get)
def test_model_catches_wrong_kernels(dtype):
    """Six wrong algorithms leave the bounds, in every dtype: the sink scaled by 1/sqrt(d), lse not
    updated, delta taken from the un-folded o, ds with the wrong sign, fully masked rows multiplied
    instead of selected, ds summed over heads."""
    shape = (2, 37, 3, 96)
    ro, rl, rd = _emu_ratios(shape, dtype, 2.0)
    assert ro <= ref.F and rl <= ref.F and rd <= ref.F
    ro, rl, _ = _emu_ratios(shape, dtype, 2.0, fbug="scaled_sink")
    assert ro > ref.F and rl > ref.F, (ro, rl)
    _, rl, _ = _emu_ratios(shape, dtype, 2.0, fbug="lse_kept")
    assert rl > ref.F, rl
    ro, _, _ = _emu_ratios(shape, dtype, 2.0, fbug="multiplied")
    assert ro > ref.F, ro
    for kw in (dict(delta_from="unfolded"), dict(gbug="sign"), dict(gbug="all_heads")):
        _, _, rd = _emu_ratios(shape, dtype, 2.0, **kw)
        assert rd > ref.F, (kw, rd)


# ---------------------------------------------------------------------------------- module
def _make_mask(kind, B, T, gen):
    import xdot

    if kind == "none":
        return None, None
    if kind in ("causal", "window"):
        m = xdot.StructuredMask(causal=True, window=4 if kind == "window" else None)
        return m, m.dense(B, T, T, 0)
    if kind == "documents":
        m = xdot.StructuredMask(causal=True, doc_starts=[0, 5, T - 3])
        return m, m.dense(B, T, T, 0)
    mask = torch.rand(B, T, T, generator=gen) < 0.35
    mask[..., torch.arange(T), torch.arange(T)] = False
    mask[:, 1, :] = True  # a fully masked row: finite with sinks
    return mask, mask


def _draw_sinks(m, seed):
    with torch.no_grad():
        m.sinks.copy_(torch.rand(m.sinks.shape, generator=torch.Generator().manual_seed(seed), dtype=F64) * 2 - 1)


def _rank_parity(rank, ws, impl, chunks, kind, rope=False, norm=False, Hg=None, layout="contiguous", sync=False, tol=1e-9):
    """Every rank's rows of the module with ``sinks=True`` against the ``distributed=False`` module on
    the whole sequence (1e-9; 1e-8 on the Sum-reduced parameter gradients, ``sinks`` among them),
    which rank 0 also holds against the dense definition where the module has neither rope nor norm."""
    import xdot
    from xdot import DistributedDotProductAttn, Rotary
    from xdot.parallel import GradSync, allreduce_gradients, broadcast_parameters

    dtype, H, B = F64, 4, 1
    torch.manual_seed(100 + rank)
    kw = dict(num_heads=H, add_bias=True, num_gathered_heads=Hg, qk_norm=norm, sinks=True)
    model = DistributedDotProductAttn(DIM, impl=impl, chunk_plan=chunks, layout=layout, rope=Rotary() if rope else None,
                                      **kw).to(dtype)
    gt_model = DistributedDotProductAttn(DIM, distributed=False, impl="materialized", rope=Rotary() if rope else None,
                                         **kw).to(dtype)
    _draw_sinks(model, 40 + rank)
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
    assert bool(torch.isfinite(outs).all()) and bool(torch.isfinite(dxs).all())
    torch.testing.assert_close(outs, gt_out.detach(), atol=tol, rtol=tol)
    torch.testing.assert_close(dxs, xg.grad, atol=tol, rtol=tol)
    local_ds = model.sinks.grad.detach().clone() if gs is None else None
    if gs is not None:
        gs.wait()
    else:
        allreduce_gradients(model)
    names = [n for n, _ in model.named_parameters()]
    assert "sinks" in names
    for (n1, p1), (n2, p2) in zip(gt_model.named_parameters(), model.named_parameters()):
        assert n1 == n2 and p2.grad is not None, n1
        torch.testing.assert_close(p2.grad, p1.grad, atol=tol * 10, rtol=tol * 10, msg=lambda m: f"d{n1}: {m}")
    if local_ds is not None and ws > 1:  # each rank's gradient is the partial over its rows
        parts = comm.all_gather_object(local_ds)
        torch.testing.assert_close(sum(parts), gt_model.sinks.grad, atol=tol * 10, rtol=tol * 10)
    if rank == 0 and not rope and not norm:
        params = {n: p.detach().clone().requires_grad_(True) for n, p in gt_model.named_parameters()}
        xd = x_full.clone().requires_grad_(True)
        want = ref.dense_attn(params, xd, xd, xd, dense, H, Hg)
        want.sum().backward()
        torch.testing.assert_close(gt_out.detach(), want.detach(), atol=tol, rtol=tol)
        torch.testing.assert_close(xg.grad, xd.grad, atol=tol, rtol=tol)
        for n, p in gt_model.named_parameters():
            torch.testing.assert_close(p.grad, params[n].grad, atol=tol * 10, rtol=tol * 10, msg=lambda m: f"dense d{n}: {m}")


IMPLS = {"flash_whole": ("flash", 1), "flash_chunked": ("flash", 2), "ring": ("ring", None),
         "materialized": ("materialized", None)}


@pytest.mark.parametrize("kind", ["window", "dense"])
@pytest.mark.parametrize("impl", list(IMPLS))
@pytest.mark.parametrize("ws", [2, 3, 4])
def test_module_ranks(ws, impl, kind):
    """Every ``impl`` (flash whole and chunked, ring, materialized) on 2..4 ranks: a causal window,
    and a dense random mask with a fully masked row."""
    from xdot.utils.comm import ThreadGroup

    ThreadGroup(ws).run(lambda r: _rank_parity(r, ws, *IMPLS[impl], kind))


@pytest.mark.parametrize("impl", ["flash_chunked", "ring", "materialized"])
def test_module_ranks_with_the_other_features(impl):
    """With ``rope`` and ``qk_norm``, ``num_gathered_heads < num_heads`` under ``layout='zigzag'``, and
    a document mask."""
    from xdot.utils.comm import ThreadGroup

    Hg = None if impl == "materialized" else 2
    ThreadGroup(3).run(lambda r: _rank_parity(r, 3, *IMPLS[impl], "window", True, True, Hg=Hg, layout="zigzag"))
    ThreadGroup(2).run(lambda r: _rank_parity(r, 2, *IMPLS[impl], "documents", True, False, Hg=2 if Hg else None))


@pytest.mark.parametrize("fused", [True, False])
def test_module_grad_sync_sums_the_sinks_gradient(fused, monkeypatch):
    """``XDOT_FUSED_MODULE=1`` and ``=0`` with the gradients -- the sinks' included -- reduced by a
    ``GradSync`` and read after ``wait()``."""
    from xdot.utils.comm import ThreadGroup
    from xdot.utils.env import FLAGS

    monkeypatch.setattr(FLAGS, "fused_module", fused)
    ThreadGroup(3).run(lambda r: _rank_parity(r, 3, "flash", 2, "causal", True, sync=True))


def test_gloo_processes():
    """Two gloo processes (the helpers of tests/_dist.py): the flash module with sinks against the
    single-device module."""
    from _dist import run_gloo

    run_gloo(_gloo_body, 2)


def _gloo_body(rank, ws):
    _rank_parity(rank, ws, "flash", 1, "window")


@pytest.mark.parametrize("impl", ["flash", "ring", "materialized"])
def test_off_is_bitwise_the_module_without_the_argument(impl):
    """``sinks=False``: output, every gradient and the ``state_dict`` keys are those of a module built
    without the argument."""
    import xdot

    res = []
    for kw in ({}, {"sinks": False}):
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


def test_state_dict():
    import xdot

    m = xdot.DistributedDotProductAttn(DIM, num_heads=4, sinks=True, num_gathered_heads=2)
    assert tuple(m.sinks.shape) == (4,) and bool((m.sinks == 0).all())  # one per ROW head, zeros
    _draw_sinks(m, 1)
    sd = m.state_dict()
    assert [k for k in sd if "sink" in k] == ["sinks"]
    m2 = xdot.DistributedDotProductAttn(DIM, num_heads=4, sinks=True, num_gathered_heads=2)
    m2.load_state_dict(sd)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, sd[k])
    # a reference-shaped dict: exactly the sinks are missing
    plain_m = xdot.DistributedDotProductAttn(DIM, num_heads=4, num_gathered_heads=2)
    plain = plain_m.state_dict()
    assert "sinks" not in plain and plain_m.sinks is None
    res = m2.load_state_dict(plain, strict=False)
    assert res.missing_keys == ["sinks"] and not res.unexpected_keys
    with pytest.raises(RuntimeError):
        m2.load_state_dict(plain)
    xdot.DistributedDotProductAttn(DIM, num_heads=4, num_gathered_heads=2, sinks=False).load_state_dict(plain)
    assert "sinks=True" in repr(m) and "sinks" not in repr(plain_m)


def test_zero_sinks_are_one_extra_key_of_score_zero():
    import xdot

    torch.manual_seed(0)
    m = xdot.DistributedDotProductAttn(DIM, num_heads=4, distributed=False, impl="flash", sinks=True).double()
    x = torch.randn(1, 7, DIM, dtype=F64)
    params = {n: p.detach() for n, p in m.named_parameters()}
    k = torch.nn.functional.linear(x, params["keys.weight"])
    q = torch.nn.functional.linear(x, params["queries.weight"])
    v = torch.nn.functional.linear(x, params["values.weight"])
    # an extra key whose score is 0 for every row and whose value is 0
    H, D = 4, DIM // 4
    kh = k.view(1, 7, H, D).transpose(1, 2)
    qh = torch.cat([q.view(1, 7, H, D).transpose(1, 2), torch.zeros(1, H, 1, D, dtype=F64)], dim=2)
    vh = torch.cat([v.view(1, 7, H, D).transpose(1, 2), torch.zeros(1, H, 1, D, dtype=F64)], dim=2)
    o = torch.softmax(kh @ qh.transpose(-1, -2) / math.sqrt(D), -1) @ vh
    want = torch.nn.functional.linear(o.transpose(1, 2).reshape(1, 7, DIM), params["composition.weight"])
    torch.testing.assert_close(m(x, x, x, None), want, rtol=1e-12, atol=1e-12)


def test_argument_checks():
    from xdot.parallel.attention import seq_parallel_attention
    from xdot.parallel.ring import ring_attention

    k, q, v, mask, s, _ = _problem(H=3, D=4)
    for f in (seq_parallel_attention, ring_attention):
        with pytest.raises(ValueError):
            f(k, q, v, mask, 3, 0.5, comm=_local(), sinks=torch.zeros(3, 1, dtype=F64))  # shape
        with pytest.raises(ValueError):
            f(k, q, v, mask, 3, 0.5, comm=_local(), sinks=torch.zeros(4, dtype=F64))  # length
        with pytest.raises(TypeError):
            f(k, q, v, mask, 3, 0.5, comm=_local(), sinks=torch.zeros(3, dtype=torch.int64))  # dtype
        with pytest.raises(TypeError):
            f(k, q, v, mask, 3, 0.5, comm=_local(), sinks=[0.0, 0.0, 0.0])
        f(k, q, v, mask, 3, 0.5, comm=_local(), sinks=torch.zeros(3))  # fp32 logits beside fp64 tensors


@pytest.mark.parametrize("impl", ["flash", "ring"])
def test_check_raises_when_one_rank_has_no_sinks(impl, monkeypatch):
    import xdot
    from xdot.utils.checks import RankDivergenceError
    from xdot.utils.comm import ThreadGroup
    from xdot.utils.env import FLAGS

    monkeypatch.setattr(FLAGS, "check", True)

    def body(r, flags):
        x = torch.rand(1, LENGTH, DIM, dtype=F64)
        m = xdot.DistributedDotProductAttn(DIM, num_heads=4, impl=impl, sinks=flags[r]).double()
        return m(x, x, x, xdot.StructuredMask(causal=True))

    with pytest.raises(RankDivergenceError):
        ThreadGroup(2).run(body, (True, False))
    ThreadGroup(2).run(body, (True, True))
