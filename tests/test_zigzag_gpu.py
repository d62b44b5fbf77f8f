"""Zigzag row sharding on the GPU: ``mask_gen`` with a row-run table (``csrc/mask_pack.hip``) is
BITWISE what ``mask_pack`` makes of ``StructuredMask.dense_at`` at the layout's rows and columns
(checked against an element-by-element construction in ``tests/test_zigzag.py``), for every column
order the flash / ring paths present; the two-run rotary table; and emulated and real ranks with
``layout="zigzag"`` against the same call on the dense tensor and against fp64."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

LAYOUT = "zigzag"


def _assert_packed_equal(got, ref):
    assert got.shape == ref.shape
    for name in ("bits", "flags", "bits_t"):
        a, b = getattr(got, name), getattr(ref, name)
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert torch.equal(a, b), name


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()


# (B, R, n, rank): the run boundary at row 35, inside tile 0; on the tile edge (row 64); odd R with
# h0 = 17, B = 2; the boundary inside the second tile (row 100); one run
SHAPES = [(1, 70, 3, 1), (1, 128, 2, 0), (2, 33, 4, 2), (1, 200, 3, 0), (1, 70, 1, 0)]
_ids = lambda s: "x".join(map(str, s))  # noqa: E731


def _layout(R, n, rank):
    from xdot.parallel.layout import gathered_cols, global_rows, row_runs

    return row_runs(LAYOUT, rank, n, R), global_rows(LAYOUT, rank, n, R), gathered_cols(LAYOUT, n, R)


def _rules(B, T):
    ln = [max(1, T - 13 - 40 * b) for b in range(B)]
    return {"causal": dict(causal=True), "window": dict(window=37), "lengths": dict(lengths=ln),
            "all": dict(causal=True, window=70, lengths=ln)}


def _check_generated(gpu, spec, B, R, n, rank, view=None, tag=None):
    """generate_mask with the row table (and, through the cache, what the attention paths ask for)
    against prepare_mask of the dense oracle at the layout's indices."""
    from xdot.ops import flash
    from xdot.ops.mask import resolve, segments_of

    runs, rows, cols = _layout(R, n, rank)
    T = n * R
    dense = spec.dense_at(B, rows, cols, gpu)
    dense = dense if view is None else view(dense)
    Tp = dense.shape[-1]
    ref = flash.prepare_mask(dense.contiguous(), B, R, Tp)
    got = flash.generate_mask(spec, B, R, Tp, segments=segments_of(view, T, cols), row_segments=runs, device=gpu)
    _assert_packed_equal(got, ref)
    flash.MASK_CACHE.clear()
    bound = resolve(spec, B, R, T, rank, True, gpu, LAYOUT)
    _assert_packed_equal(flash.prepare_mask_cached(bound, B, R, Tp, tag=("t", tag), view=view), ref)
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("rule", ["causal", "window", "lengths", "all"])
def test_generated_equals_packed_dense_at(gpu, rule, shape):
    from xdot import StructuredMask
    from xdot.ops import flash

    B, R, n, rank = shape
    spec = StructuredMask(**_rules(B, n * R)[rule])
    got = _check_generated(gpu, spec, B, R, n, rank)
    runs = _layout(R, n, rank)[0]
    if len(runs) == 1:  # one run: also bitwise the row_offset call
        _assert_packed_equal(got, flash.generate_mask(spec, B, R, n * R, runs[0][2], device=gpu))


def _doc_tables(B, R, n, rank):
    """name -> doc_starts; ``hi``: the first global row of the high run (rows [h0, R)), ``lo_end``
    the last global row of the low run: the straddling tile holds both."""
    T = n * R
    h0 = (R + 1) // 2
    h1 = R - h0
    lo_end = rank * h0 + h0 - 1
    hi = n * h0 + (n - 1 - rank) * h1
    ones = list(range(max(hi - 40, 0), max(hi - 40, 0) + 80))  # 80 one-row documents across `hi`
    out = {
        "at_high_run": [hi],
        "both_sides": [max(lo_end - 2, 0), lo_end, hi + 2],
        "one_row_docs": ones,
        "dups_past_T": [3, 3, hi, hi, hi + 1, T, T + 7, 2**31 - 1],
        "per_batch": [[max(lo_end - 1, 0), hi, hi + 3], ones[:3]][:B] if B > 1 else [[lo_end, hi + 1, T]],
    }
    return out


DOC_NAMES = ["at_high_run", "both_sides", "one_row_docs", "dups_past_T", "per_batch"]


@pytest.mark.parametrize("shape", SHAPES[:4], ids=_ids)
@pytest.mark.parametrize("dname", DOC_NAMES)
def test_documents_across_the_run_boundary(gpu, dname, shape):
    from xdot import StructuredMask

    B, R, n, rank = shape
    ds = _doc_tables(B, R, n, rank)[dname]
    for kw in (dict(), dict(causal=True, window=90)):
        _check_generated(gpu, StructuredMask(doc_starts=ds, **kw), B, R, n, rank)
        # a device table is read by the kernel without validation
        dev = torch.tensor(ds, device=gpu)
        _check_generated(gpu, StructuredMask(doc_starts=dev, **kw), B, R, n, rank)


def _views(B, R, n, rank):
    from xdot.parallel import attention as pa
    from xdot.parallel.ring import _block_mask

    c0 = R // 2
    chunks = [(0, c0), (c0, R - c0)]

    def own_excluded(r0, rc):  # _own_excluded_mask's view of a user mask
        def view(m):
            m = pa._mask_cols(B, R, n, 0, n, r0, rc)(m).clone()
            m[..., rank * rc:(rank + 1) * rc] = True if m.dtype == torch.bool else -1
            return m
        return view

    h = R // 2
    s0, s1 = (rank - 1) % n, (rank + 1) % n
    return {
        "perm_cols": pa._perm_cols(B, R, n, chunks),
        "ring_block": lambda m: _block_mask(m, n - 1, R),
        "ring_merged": lambda m: torch.cat([_block_mask(m, s0, R, 0, h), _block_mask(m, s1, R, h, R)], -1),
        "own_excluded": own_excluded(*chunks[1]),
        "peer_segment": pa._mask_cols(B, R, n, 0, max(rank, 1), *chunks[0]),
    }


VIEW_NAMES = ["perm_cols", "ring_block", "ring_merged", "own_excluded", "peer_segment"]


@pytest.mark.parametrize("shape", SHAPES[:4], ids=_ids)
@pytest.mark.parametrize("vname", VIEW_NAMES)
def test_column_orders(gpu, vname, shape):
    """Every existing view composes with the layout: its segment table starts from the gathered
    side's global indices."""
    from xdot import StructuredMask

    B, R, n, rank = shape
    view = _views(B, R, n, rank)[vname]
    docs = _doc_tables(B, R, n, rank)
    for kw in (dict(causal=True), dict(causal=True, window=70, lengths=_rules(B, n * R)["lengths"]["lengths"]),
               dict(causal=True, doc_starts=docs["one_row_docs"]), dict(doc_starts=docs["both_sides"])):
        _check_generated(gpu, StructuredMask(**kw), B, R, n, rank, view=view, tag=vname)


def test_row_segments_are_validated(gpu):
    from xdot import StructuredMask
    from xdot.ops import flash

    spec = StructuredMask(causal=True)
    for bad in ([(0, 30, 0), (31, 39, 100)], [(0, 30, 0), (30, 41, 100)], [(0, 35, 0), (35, 35, -4)]):
        with pytest.raises(ValueError):
            flash.generate_mask(spec, 1, 70, 210, row_segments=bad, device=gpu)
    with pytest.raises(ValueError):
        flash.generate_mask(StructuredMask(causal=True, row_offset=0), 1, 70, 210, row_segments=[(0, 35, 0), (35, 35, 99)],
                            device=gpu)


def test_no_dense_allocation(gpu):
    """As tests/test_structured_mask_gpu.py: the packed outputs are ~R*T/4 bytes, a dense bool mask
    R*T: the peak stays below R*T/2, row table and zigzag column segments included."""
    from xdot import StructuredMask
    from xdot.ops import flash
    from xdot.ops.mask import resolve

    Rb, n, rank = 4096, 2, 0
    Tb = n * Rb
    spec = StructuredMask(causal=True, doc_starts=[100, 5000])
    bound = resolve(spec, 1, Rb, Tb, rank, True, gpu, LAYOUT)
    assert bound._rows is not None and len(bound._rows) == 2
    flash.MASK_CACHE.clear()
    flash.prepare_mask_cached(resolve(spec, 1, 64, 128, 0, True, gpu, LAYOUT), 1, 64, 128)  # extension, allocator: warmed
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(gpu)
    torch.cuda.reset_peak_memory_stats(gpu)
    out = flash.prepare_mask_cached(bound, 1, Rb, Tb)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated(gpu) - base
    print(f"zigzag generate_mask R={Rb} T={Tb}: peak +{grown} B (dense bool {Rb * Tb} B)")
    assert grown < Rb * Tb // 2
    assert out.bits.numel() * 8 + out.bits_t.numel() * 8 + out.flags.numel() <= grown
    flash.MASK_CACHE.clear()


# ---- rotary ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,D,n,rank", [(70, 96, 3, 1), (33, 40, 4, 0), (3125, 96, 8, 2)])
def test_two_run_table(gpu, R, D, n, rank):
    """The bound of tests/test_rope_gpu.py's ``test_table``: both tables multiply the same doubles,
    what remains is the final rounding, <= 2^-24."""
    import xdot

    runs, rows, _cols = _layout(R, n, rank)
    assert len(runs) == 2
    rot = xdot.Rotary()
    off = rot.resolve(rank, R, n, LAYOUT)
    assert off == tuple(runs)
    c, s = rot.table(R, D, off, gpu)
    assert c.dtype == s.dtype == torch.float32 and tuple(c.shape) == tuple(s.shape) == (R, D // 2)
    assert rot.table(R, D, off, gpu)[0] is c
    inv = torch.tensor(rot.inv_freq(D), dtype=torch.float64)
    ang = rows.double().view(R, 1) * inv.view(1, -1)
    ec, es = (c.cpu().double() - torch.cos(ang)).abs().max().item(), (s.cpu().double() - torch.sin(ang)).abs().max().item()
    print(f"two-run rope_table R={R} D={D} rank {rank}/{n}: max |cos err| {ec:.3e} |sin err| {es:.3e}")
    assert ec <= 2.0 ** -24 and es <= 2.0 ** -24


# ---- emulated ranks ----------------------------------------------------------------------------------
DIM, H = 192, 2


def _spec(R, n, rank):
    from xdot import StructuredMask

    docs = _doc_tables(1, R, n, rank)
    return StructuredMask(causal=True, window=3 * R, doc_starts=[R // 3] + docs["both_sides"])


def _module_step(gpu, impl, mask, comm, chunks, R, dtype, rope=False, dim=DIM):
    import xdot

    torch.manual_seed(0)
    m = xdot.DistributedDotProductAttn(dim, num_heads=H, impl=impl, chunk_plan=chunks, comm=comm, layout=LAYOUT,
                                       rope=xdot.Rotary() if rope else None).to(gpu, dtype)
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(1, R, dim, generator=g).to(gpu, dtype).requires_grad_(True)
    out = m(x, x, x, mask)
    out.float().square().mean().backward()
    torch.cuda.synchronize()
    return m, x, [out.detach(), x.grad] + [p.grad for p in m.parameters()]


RANKS = [(3, 1), (8, 7)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("R", [70, 200])
@pytest.mark.parametrize("n,rank", RANKS)
@pytest.mark.parametrize("path,chunks", [("fused", 1), ("fused", 2), ("per_op", 1), ("per_op", 2), ("ring", None)])
def test_emulated_rank_bitwise_vs_dense(gpu, path, chunks, n, rank, R, dtype, monkeypatch):
    """A StructuredMask under the layout computes bit for bit what the same call computes from the
    dense ``dense_at`` tensor (local rows, GLOBAL columns: the path selects them into gathered order)."""
    from xdot.ops import flash
    from xdot.utils.comm import EmulatedComm
    from xdot.utils.env import FLAGS

    monkeypatch.setattr(FLAGS, "fused_module", path == "fused")
    flash.MASK_CACHE.clear()
    impl = "ring" if path == "ring" else "flash"
    spec = _spec(R, n, rank)
    _runs, rows, _cols = _layout(R, n, rank)
    dense = spec.dense_at(1, rows, torch.arange(n * R), gpu)
    res = [_module_step(gpu, impl, mk, EmulatedComm(n, rank=rank), chunks, R, dtype, rope=True)[2] for mk in (spec, dense)]
    assert len(res[0]) == len(res[1]) == 2 + 4
    for a, b in zip(*res):
        torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)
    assert torch.isfinite(res[0][0].float()).all()


@pytest.mark.parametrize("impl", ["flash", "materialized"])
def test_padded_heads_and_materialized_bitwise_vs_dense(gpu, impl):
    """The padded-head branch of the flash path (head dim 40, zero-padded to 64) and the
    materialised path, rank 1 of 3 with rope: the StructuredMask against its ``dense_at`` tensor."""
    from xdot.ops import flash
    from xdot.utils.comm import EmulatedComm

    flash.MASK_CACHE.clear()
    n, rank, R = 3, 1, 70
    spec = _spec(R, n, rank)
    dense = spec.dense_at(1, _layout(R, n, rank)[1], torch.arange(n * R), gpu)
    res = [_module_step(gpu, impl, mk, EmulatedComm(n, rank=rank), 1, R, torch.bfloat16, rope=True, dim=80)[2]
           for mk in (spec, dense)]
    for a, b in zip(*res):
        torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)
    assert torch.isfinite(res[0][0].float()).all()


def _dense64(k, qv, mask, n, scale, blocks):
    """fp64 dense attention of the rows ``k`` over the replicated shard ``qv`` (what EmulatedComm's
    gather hands out) with ``mask`` (1, R, n * R) -> (o, dk, d qv summed over ``blocks``)."""
    R, C = k.shape[1], k.shape[2]
    D = C // H
    kd = k.detach().double().clone().requires_grad_(True)
    g = qv.detach().double().repeat(1, n, 1).clone().requires_grad_(True)
    kh = kd.view(1, R, H, D).transpose(1, 2)
    qh = g[..., :C].reshape(1, n * R, H, D).transpose(1, 2)
    vh = g[..., C:].reshape(1, n * R, H, D).transpose(1, 2)
    s = (kh @ qh.transpose(-1, -2) * scale).masked_fill(mask.view(1, 1, R, n * R), -float("inf"))
    o = (s.softmax(-1) @ vh).transpose(1, 2).reshape(1, R, C)
    o.square().mean().backward()
    dqv = sum(g.grad[:, j * R:(j + 1) * R] for j in blocks)
    return o.detach(), kd.grad, dqv


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("R", [70, 200])
@pytest.mark.parametrize("n,rank", RANKS)
@pytest.mark.parametrize("impl,chunks", [("flash", 1), ("flash", 2), ("ring", None)])
def test_emulated_rank_vs_fp64(gpu, impl, chunks, n, rank, R, dtype):
    """Against an fp64 dense attention over the replicated shard with the ``dense_at`` mask, within
    the existing bounds: bf16 1e-2 forward / 2e-2 gradients (tests/test_segmented.py), exact fp32
    2e-6 (tests/test_flash_f32_gpu.py).  The emulated reduce-scatter keeps this rank's block of the
    gathered side's gradient; the emulated ring sums every block's."""
    from xdot.ops import flash
    from xdot.parallel.attention import seq_parallel_attention_packed, start_gather
    from xdot.parallel.ring import ring_attention_packed
    from xdot.utils.comm import EmulatedComm

    flash.MASK_CACHE.clear()
    comm = EmulatedComm(n, rank=rank)
    g = torch.Generator().manual_seed(3)
    k = torch.randn(1, R, DIM, generator=g).to(gpu, dtype).requires_grad_(True)
    qv = torch.randn(1, R, 2 * DIM, generator=g).to(gpu, dtype).requires_grad_(True)
    spec = _spec(R, n, rank)
    scale = 1.0 / math.sqrt(DIM // H)
    if impl == "flash":
        o = seq_parallel_attention_packed(k, qv, spec, H, scale, comm=comm, layout=LAYOUT,
                                          pending=start_gather(qv, comm, chunks=chunks))
    else:
        o = ring_attention_packed(k, qv, spec, H, scale, comm=comm, layout=LAYOUT)
    o.float().square().mean().backward()
    torch.cuda.synchronize()
    _runs, rows, cols = _layout(R, n, rank)
    ro, rdk, rdqv = _dense64(k, qv, spec.dense_at(1, rows, cols, gpu), n, scale, [rank] if impl == "flash" else range(n))
    errs = {"out": _rel(o, ro), "dk": _rel(k.grad, rdk), "dqv": _rel(qv.grad, rdqv)}
    print(f"zigzag {impl} rank {rank}/{n} R={R} chunks={chunks} {dtype}:", {a: f"{b:.2e}" for a, b in errs.items()})
    tol_o, tol_g = (1e-2, 2e-2) if dtype == torch.bfloat16 else (2e-6, 2e-6)
    assert errs["out"] <= tol_o and errs["dk"] <= tol_g and errs["dqv"] <= tol_g, errs


def _rotate_at(x, heads, pos, base=10000.0):
    """tests/_rope_ref.py's ``rotate`` at arbitrary positions."""
    B, T, C = x.shape
    D = C // heads
    h = D // 2
    inv = torch.tensor([base ** (-2.0 * i / D) for i in range(h)], dtype=torch.float64, device=x.device)
    ang = pos.to(x.device, torch.float64).view(T, 1) * inv.view(1, h)
    c, s = torch.cos(ang).view(1, T, 1, h), torch.sin(ang).view(1, T, 1, h)
    xv = x.reshape(B, T, heads, D)
    x1, x2 = xv[..., :h], xv[..., h:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).reshape(B, T, C)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_module_with_rope_vs_fp64(gpu, dtype, monkeypatch):
    """The module (one-node flash path, two gather chunks) with rope under the layout, rank 1 of 3,
    against fp64 torch math on the same parameters: projections, the rotation at the rank's GLOBAL
    positions, dense attention over the replicated shard, the output projection.  Bounds: bf16
    2e-2 forward / 3e-2 gradients (tests/test_module_gpu.py).  Exact fp32: the flash kernels' 2e-6
    (tests/test_flash_f32_gpu.py) plus 2^-21 for each of the two rotation passes a gradient goes
    through (tests/test_rope_gpu.py's fp32 bound of one pass: k or q forward, dk or dq back), 2.96e-6;
    measured 2.3e-6 at most (keys.weight; 2e-6 alone, which leaves the rotations out, is missed)."""
    import torch.nn.functional as F

    from xdot.ops import flash
    from xdot.utils.comm import EmulatedComm
    from xdot.utils.env import FLAGS

    monkeypatch.setattr(FLAGS, "fused_module", True)
    flash.MASK_CACHE.clear()
    n, rank, R = 3, 1, 200
    spec = _spec(R, n, rank)
    m, x, got = _module_step(gpu, "flash", spec, EmulatedComm(n, rank=rank), 2, R, dtype, rope=True)
    _runs, rows, cols = _layout(R, n, rank)
    p = {a: b.detach().double().clone().requires_grad_(True) for a, b in m.named_parameters()}
    xd = x.detach().double().clone().requires_grad_(True)
    k = _rotate_at(F.linear(xd, p["keys.weight"]), H, rows)
    q = _rotate_at(F.linear(xd, p["queries.weight"]), H, rows)
    v = F.linear(xd, p["values.weight"])
    own = torch.cat([q, v], -1)
    # the gathered side: this rank's block is the live one, the replicas carry no gradient (the
    # emulated reduce-scatter keeps this rank's block only)
    gath = torch.cat([own if j == rank else own.detach() for j in range(n)], dim=1)
    D = DIM // H
    kh = k.view(1, R, H, D).transpose(1, 2)
    qh = gath[..., :DIM].reshape(1, n * R, H, D).transpose(1, 2)
    vh = gath[..., DIM:].reshape(1, n * R, H, D).transpose(1, 2)
    s = (kh @ qh.transpose(-1, -2) / math.sqrt(D)).masked_fill(spec.dense_at(1, rows, cols, gpu).view(1, 1, R, n * R),
                                                                -float("inf"))
    ref = F.linear((s.softmax(-1) @ vh).transpose(1, 2).reshape(1, R, DIM), p["composition.weight"])
    ref.square().mean().backward()
    errs = {"out": _rel(got[0], ref.detach()), "dx": _rel(got[1], xd.grad)}
    for (name, _p), gr in zip(m.named_parameters(), got[2:]):
        errs[name] = _rel(gr, p[name].grad)
    print(f"zigzag rope module {dtype}:", {a: f"{b:.2e}" for a, b in errs.items()})
    f32 = 2e-6 + 2 * 2.0 ** -21
    tol_o, tol_g = (2e-2, 3e-2) if dtype == torch.bfloat16 else (f32, f32)
    for name, e in errs.items():
        assert e <= (tol_o if name == "out" else tol_g), errs


# ---- real ranks on one device --------------------------------------------------------------------------
def _real_rank(rank, ws):
    """tests/test_module_gpu.py's ``_module_case`` (its bf16 bounds: 2e-2 forward, 3e-2 gradients)
    with rope, a StructuredMask, two gather chunks and the rows sharded by the layout."""
    import xdot
    from xdot.parallel import GradSync

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    R, dim, heads = 70, 192, 2
    T = ws * R
    torch.manual_seed(0)
    kw = dict(num_heads=heads, rope=xdot.Rotary())
    m = xdot.DistributedDotProductAttn(dim, impl="flash", chunk_plan=2, layout=LAYOUT, **kw).to(dev, torch.bfloat16)
    sync = GradSync(m, bucket_mb=0.05, reduce_dtype=torch.float32)
    # ground truth: plain torch ops only, fp32, the whole sequence on one device
    ref = xdot.DistributedDotProductAttn(dim, distributed=False, impl="materialized", backend="torch", **kw).to(dev)
    ref.load_state_dict({k: v.float() for k, v in m.state_dict().items()})
    x_full = torch.randn(1, T, dim, generator=torch.Generator().manual_seed(1)).to(dev, torch.bfloat16)
    spec = xdot.StructuredMask(causal=True, doc_starts=[50, (R + 1) // 2 * ws + 3])
    xf = x_full.float().requires_grad_(True)
    ro = ref(xf, xf, xf, spec)
    ro.pow(2).sum().backward()
    x = xdot.shard_rows(x_full, rank, ws, layout=LAYOUT).clone().requires_grad_(True)
    out = m(x, x, x, spec)
    out.float().pow(2).sum().backward()
    sync.wait()  # Sum all-reduce of the replicated parameters' gradients
    torch.cuda.synchronize()
    mine = lambda t: xdot.shard_rows(t, rank, ws, layout=LAYOUT)  # noqa: E731
    eo, ex = _rel(out, mine(ro.detach())), _rel(x.grad, mine(xf.grad))
    ew = max(_rel(a.grad, b.grad) for a, b in zip(m.parameters(), ref.parameters()))
    print(f"zigzag real rank {rank}/{ws}: out {eo:.2e} dx {ex:.2e} dW {ew:.2e}")
    assert eo <= 2e-2 and ex <= 3e-2 and ew <= 3e-2, (eo, ex, ew)


def test_real_ranks_one_device(gpu):
    """Three gloo ranks sharing the GPU (as tests/test_segmented.py: in-process ranks would deadlock
    in the backward's collective) against the single-device module on the whole sequence."""
    from _dist import run_gloo

    run_gloo(_real_rank, 3, timeout=400)
