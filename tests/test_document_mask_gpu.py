"""Document masks (``StructuredMask(doc_starts=...)``) on the GPU: the generated packed mask is
BITWISE what ``mask_pack`` makes of the dense oracle (``StructuredMask.dense``, checked element by
element in ``tests/test_document_mask.py``) for every column order the flash / ring paths present,
and every path fed the description computes bit for bit what it computes from that dense tensor."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# tests/test_structured_mask_gpu.py's shapes (B, R, T, row_offset): off the 64/128 grid with a
# partial last word; B = 2; T < 128; the exact grid; the middle rank of 3; T % 8 in {0, 4, odd}
SHAPES = [(1, 70, 200, 0), (2, 33, 130, 0), (1, 64, 100, 0), (1, 128, 256, 0), (1, 50, 150, 50),
          (1, 40, 264, 0), (1, 40, 260, 0), (1, 40, 257, 0)]

DOC_NAMES = ["in_word", "on_grid", "n1_in_row_tile", "three_in_row_tile", "one_row", "dups", "beyond_T", "per_batch",
             "window", "combo"]


def _doc_spec(name, B, T, ro, device=None):
    """(rules, starts): ``device``: the starts as a tensor there, else as a list."""
    ln = [max(0, T - 13 - 40 * b) for b in range(B)]
    rules, starts = {
        "in_word": ({}, [5, 70, 100, 135]),                       # strictly inside 64-bit words
        "on_grid": ({}, [64, 128, 192, 256]),                     # whole tiles: flags 0 / 1
        "n1_in_row_tile": ({"causal": True}, [ro + 20]),          # lanes of one wave in two documents
        "three_in_row_tile": ({"causal": True}, [ro + 10, ro + 30, ro + 50]),
        "one_row": ({}, list(range(ro + 3, ro + 12))),            # one-row documents
        "dups": ({"causal": True}, [40, 40, 40, 90, 90, 90]),     # empty documents
        "beyond_T": ({}, [30, T, T + 5, 10 ** 6, 2 ** 40]),       # no effect (and the int32 clamp)
        "per_batch": ({"causal": True, "lengths": ln}, [[7 + 11 * b, 64 + b, 64 + b, 100 + 30 * b] for b in range(B)]),
        "window": ({"window": 70}, [ro + 25, ro + 26, 128]),
        "combo": ({"causal": True, "window": 70, "lengths": ln}, sorted([9, 64, ro + 40, 130])),
    }[name]
    if device is not None:
        starts = torch.tensor(starts, device=device)
    return rules, starts


def _assert_packed_equal(got, ref):
    assert got.shape == ref.shape
    for name in ("bits", "flags", "bits_t"):
        a, b = getattr(got, name), getattr(ref, name)
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert torch.equal(a, b), name


@pytest.mark.parametrize("as_tensor", [False, True], ids=["list", "device_tensor"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", DOC_NAMES)
def test_generated_equals_packed_dense(gpu, name, shape, as_tensor):
    from xdot import StructuredMask
    from xdot.ops import flash

    B, R, T, ro = shape
    rules, starts = _doc_spec(name, B, T, ro, gpu if as_tensor else None)
    spec = StructuredMask(doc_starts=starts, **rules)
    got = flash.generate_mask(spec, B, R, T, ro, device=gpu)
    dense = spec.dense(B, R, T, ro, gpu)
    _assert_packed_equal(got, flash.prepare_mask(dense, B, R, T))
    if name == "on_grid" and ro % 32 == 0:  # boundaries on the tile grid: no partial tile
        assert not (got.flags == 2).any()


@pytest.mark.parametrize("causal", [False, True])
def test_search_depth(gpu, causal):
    """n = 300 starts at T = 320 (one-row documents, a 64-row tile spanning 64 of them), and the
    same with every start repeated."""
    from xdot import StructuredMask
    from xdot.ops import flash

    R = T = 320
    for starts in (list(range(10, 310)), sorted(list(range(10, 160)) * 2)):
        assert len(starts) == 300
        for s in (starts, torch.tensor(starts, device=gpu, dtype=torch.int32)):
            spec = StructuredMask(causal=causal, doc_starts=s)
            got = flash.generate_mask(spec, 1, R, T, 0, device=gpu)
            _assert_packed_equal(got, flash.prepare_mask(spec.dense(1, R, T, 0, gpu), 1, R, T))


def test_empty_tables(gpu):
    """n = 0, shared and per batch, is no documents at all."""
    from xdot import StructuredMask
    from xdot.ops import flash

    ref = flash.generate_mask(StructuredMask(causal=True), 2, 33, 130, 0, device=gpu)
    for s in ([], [[], []], torch.zeros(2, 0, dtype=torch.int64, device=gpu)):
        _assert_packed_equal(flash.generate_mask(StructuredMask(causal=True, doc_starts=s), 2, 33, 130, 0, device=gpu), ref)


# ---------------------------------------------------------------------------------------------
N, R, RANK, CHUNKS, H_RING = 3, 96, 1, [(0, 48), (48, 48)], 40


def _views():
    """The column views of tests/test_structured_mask_gpu.py."""
    from xdot.parallel import attention as pa
    from xdot.parallel.ring import _block_mask

    B = 1

    def own_excluded(r0, rc):  # _own_excluded_mask's view of a user mask
        def view(m):
            m = pa._mask_cols(B, R, N, 0, N, r0, rc)(m).clone()
            m[..., RANK * rc:(RANK + 1) * rc] = True if m.dtype == torch.bool else -1
            return m
        return view

    s0, s1 = 0, 2  # the two lanes' source ranks at some step of the bidirectional ring
    return {
        "mask_cols_peer": pa._mask_cols(B, R, N, 2, 3, 48, 48),
        "mask_cols_chunk": pa._mask_cols(B, R, N, 0, N, 0, 48),
        "perm_cols": pa._perm_cols(B, R, N, CHUNKS),
        "own_excluded": own_excluded(48, 48),
        "ring_merged": lambda m: torch.cat([_block_mask(m, s0, R, 0, H_RING), _block_mask(m, s1, R, H_RING, R)], -1),
    }


VIEW_NAMES = ["mask_cols_peer", "mask_cols_chunk", "perm_cols", "own_excluded", "ring_merged"]
# global rows 96..191 of T = 288: boundaries before, inside (off and on the 32-row grid), after
VIEW_STARTS = [40, 96 + 30, 96 + 64, 200, 250]


@pytest.mark.parametrize("vname", VIEW_NAMES)
@pytest.mark.parametrize("rules", [{}, {"causal": True}, {"causal": True, "window": 130, "lengths": [270]}],
                         ids=["docs", "causal", "causal_window_lengths"])
def test_segment_tables(gpu, rules, vname):
    from xdot import StructuredMask
    from xdot.ops import flash
    from xdot.ops.mask import segments_of

    T = N * R
    spec = StructuredMask(doc_starts=torch.tensor(VIEW_STARTS, device=gpu), **rules)
    view = _views()[vname]
    dense = view(spec.dense(1, R, T, RANK * R, gpu))
    Tp = dense.shape[-1]
    got = flash.generate_mask(spec, 1, R, Tp, RANK * R, segments=segments_of(view, T), device=gpu)
    _assert_packed_equal(got, flash.prepare_mask(dense, 1, R, Tp))
    # and through the cache, as the attention paths ask for it
    flash.MASK_CACHE.clear()
    got = flash.prepare_mask_cached(spec.bind(RANK * R, T), 1, R, Tp, tag=("t", vname), view=view)
    _assert_packed_equal(got, flash.prepare_mask(dense, 1, R, Tp))


# ---------------------------------------------------------------------------------------------
def test_no_dense_allocation(gpu):
    """tests/test_structured_mask_gpu.py's bound at its shape: the peak stays below R*T/2."""
    from xdot import StructuredMask
    from xdot.ops import flash

    Rb = Tb = 4096
    starts = torch.arange(0, Tb, Tb // 8, device=gpu)
    spec = StructuredMask(causal=True, doc_starts=starts)
    flash.generate_mask(spec, 1, 64, 128, 0, device=gpu)  # the extension, the allocator: warmed
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(gpu)
    torch.cuda.reset_peak_memory_stats(gpu)
    out = flash.generate_mask(spec, 1, Rb, Tb, 0, device=gpu)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated(gpu) - base
    print(f"generate_mask with documents R=T=4096: peak +{grown} B (dense bool {Rb * Tb} B)")
    assert grown < Rb * Tb // 2
    # 8 equal documents + causal: of the 64 x 64 (32-row x 64-col) tile pairs only the 8 diagonal
    # blocks keep anything
    fl = out.flags[0, :, :Tb // 64]
    assert float((fl == 1).float().mean()) > 0.9


def _same(a, b):
    torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)


def test_cache(gpu, monkeypatch):
    """The same description hits; an in-place edit of the device ``doc_starts`` re-generates."""
    import xdot
    from xdot import StructuredMask
    from xdot.ops import flash

    calls = []
    real = flash.generate_mask

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(flash, "generate_mask", counting)
    flash.MASK_CACHE.clear()
    torch.manual_seed(0)
    m = xdot.DistributedDotProductAttn(192, num_heads=2, impl="flash").to(gpu, torch.bfloat16)
    x = torch.randn(1, 200, 192, device=gpu, dtype=torch.bfloat16)
    starts = torch.tensor([50, 120], device=gpu)
    spec = StructuredMask(causal=True, doc_starts=starts)
    with torch.no_grad():
        y1 = m(x, x, x, spec)
        n1 = len(calls)
        y2 = m(x, x, x, spec)
        assert n1 == 1 and len(calls) == 1
        _same(y1, y2)
        starts.add_(7)
        y3 = m(x, x, x, spec)
        assert len(calls) == 2
        ref = m(x, x, x, StructuredMask(causal=True, doc_starts=[57, 127]).dense(1, 200, 200, 0, gpu))
        _same(y3, ref)
        assert not torch.equal(y3, y1)
        packed = flash.prepare_mask_cached(spec.bind(0, 200), 1, 200, 200)
        _assert_packed_equal(packed, flash.prepare_mask(StructuredMask(causal=True, doc_starts=[57, 127]).dense(1, 200, 200, 0, gpu),
                                                        1, 200, 200))


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_kernels_see_the_same_mask(gpu, dtype):
    from xdot import StructuredMask
    from xdot.ops import flash

    D, H, B, Rk, T, ro = 96, 2, 1, 96, 288, 96
    C = H * D
    scale = 1.0 / math.sqrt(D)
    g = torch.Generator(device="cpu").manual_seed(5)
    rows, kc, vc, do = (torch.randn(B, s, C, generator=g).to(gpu, dtype) for s in (Rk, T, T, Rk))
    spec = StructuredMask(causal=True, doc_starts=torch.tensor(VIEW_STARTS, device=gpu))
    fm = flash.FP32_MODES["exact"] if dtype == torch.float32 else None
    res = []
    for mk in (flash.generate_mask(spec, B, Rk, T, ro, device=gpu),
               flash.prepare_mask(spec.dense(B, Rk, T, ro, gpu), B, Rk, T)):
        o, lse = flash.fwd(rows, kc, vc, mk, H, scale, fp32_mode=fm)
        dkv, delta = flash.bwd_cols(do, rows, kc, vc, o, lse, mk, H, scale, fp32_mode=fm)
        dr = flash.bwd_rows(do, rows, kc, vc, lse, delta, mk, H, scale, fp32_mode=fm)
        res.append((o, lse, dkv, delta, dr))
    for a, b in zip(*res):
        _same(a, b)
    assert torch.isfinite(res[0][0].float()).all()


def _module_step(gpu, impl, mask, comm=None, chunks=None, dim=192, Rm=200, dtype=torch.bfloat16):
    import xdot

    torch.manual_seed(0)
    kw = {} if comm is None else {"comm": comm}
    m = xdot.DistributedDotProductAttn(dim, num_heads=2, impl=impl, chunk_plan=chunks, **kw).to(gpu, dtype)
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(1, Rm, dim, generator=g).to(gpu, dtype).requires_grad_(True)
    out = m(x, x, x, mask)
    torch.nan_to_num(out.float()).square().sum().backward()
    torch.cuda.synchronize()
    return [out.detach(), x.grad] + [p.grad for p in m.parameters()]


# D = 96 fused node / per-op graph, the ring, the materialised path, and one wide head (D = 160)
@pytest.mark.parametrize("impl,fused,dim", [("flash", True, 192), ("flash", False, 192), ("ring", True, 192),
                                            ("materialized", True, 192), ("flash", True, 320)])
def test_module_one_rank(gpu, impl, fused, dim, monkeypatch):
    from xdot import StructuredMask
    from xdot.ops import flash
    from xdot.utils.env import FLAGS

    monkeypatch.setattr(FLAGS, "fused_module", fused)
    flash.MASK_CACHE.clear()
    spec = StructuredMask(causal=True, lengths=[190], doc_starts=[37, 64, 150])
    got = _module_step(gpu, impl, spec, dim=dim)
    dense = spec.dense(1, 200, 200, 0, gpu)
    assert dense[0, 64, :64].all() and not dense[0, 64, 64]
    ref = _module_step(gpu, impl, dense, dim=dim)
    assert len(got) == len(ref) == 2 + 4
    for a, b in zip(got, ref):
        _same(a, b)
    assert torch.isfinite(got[0].float()).all()  # every row keeps its own column


@pytest.mark.parametrize("impl,chunks,local_first", [("flash", 2, True), ("flash", 2, False), ("ring", None, True)])
def test_module_emulated_middle_rank(gpu, impl, chunks, local_first, monkeypatch):
    """Rank 1 of 3 (EmulatedComm), two gather chunks: the own-block-first segmented forward with the
    merged own-excluded chunk masks, the permuted backward; the merged ring."""
    from xdot import StructuredMask
    from xdot.ops import flash
    from xdot.utils.comm import EmulatedComm
    from xdot.utils.env import FLAGS

    monkeypatch.setattr(FLAGS, "local_first", local_first)
    if chunks is not None:
        monkeypatch.setattr(FLAGS, "gather_chunks", chunks)
    flash.MASK_CACHE.clear()
    spec = StructuredMask(causal=True, doc_starts=torch.tensor(VIEW_STARTS, device=gpu))
    got = _module_step(gpu, impl, spec, EmulatedComm(N, rank=RANK), chunks, Rm=R)
    dense = spec.dense(1, R, N * R, RANK * R, gpu)
    assert dense[0, 0, :40].all() and not dense[0, 0, 40:97].any() and dense[0, 30, :126].all()
    ref = _module_step(gpu, impl, dense, EmulatedComm(N, rank=RANK), chunks, Rm=R)
    for a, b in zip(got, ref):
        _same(a, b)
    assert torch.isfinite(got[0].float()).all()


def test_seq_parallel_attention(gpu):
    from xdot import StructuredMask, seq_parallel_attention
    from xdot.ops import flash
    from xdot.utils.comm import LocalComm

    flash.MASK_CACHE.clear()
    B, T, H, D = 2, 130, 2, 96
    g = torch.Generator(device="cpu").manual_seed(2)
    q, k, v = (torch.randn(B, T, H * D, generator=g).to(gpu, torch.bfloat16) for _ in range(3))
    spec = StructuredMask(causal=True, doc_starts=torch.tensor([[20, 70], [64, 129]], device=gpu))
    got = seq_parallel_attention(q, k, v, spec, H, 0.1, comm=LocalComm())
    ref = seq_parallel_attention(q, k, v, spec.dense(B, T, T, 0, gpu), H, 0.1, comm=LocalComm())
    _same(got, ref)
    assert torch.isfinite(got.float()).all()


# ---------------------------------------------------------------------------------------------
def test_graph_replay_reads_the_tensor(gpu):
    """The generator captured in a graph with a device ``doc_starts``: after an in-place edit of the
    tensor a replay gives the NEW mask, so the kernel reads the tensor, not a host copy of it."""
    from xdot import StructuredMask, _ext
    from xdot.ops import flash

    B, Rg, T = 2, 70, 200
    starts = torch.tensor([[30, 100], [64, 65]], device=gpu)
    spec = StructuredMask(causal=True, doc_starts=starts)
    table = torch.tensor([[0, T, 0]], dtype=torch.int32, device=gpu)

    def gen():
        return _ext.ops().mask_gen(B, Rg, T, True, 0, 0, None, table, spec.device_doc_starts(gpu))

    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        gen()  # warm-up outside the capture
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        bits, flags, bits_t = gen()
    for new in ([[30, 100], [64, 65]], [[5, 150], [0, 199]]):
        starts.copy_(torch.tensor(new, device=gpu))
        graph.replay()
        torch.cuda.synchronize()
        got = flash.PackedMask(bits, flags, bits_t, (B, Rg, T))
        ref = StructuredMask(causal=True, doc_starts=new).dense(B, Rg, T, 0, gpu)
        _assert_packed_equal(got, flash.prepare_mask(ref, B, Rg, T))
