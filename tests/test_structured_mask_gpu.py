"""xdot.StructuredMask on the GPU: the generated packed mask (``mask_gen`` in
``csrc/mask_pack.hip``) is BITWISE what ``mask_pack`` makes of the equivalent dense tensor
(``StructuredMask.dense``, checked against an independent construction in
``tests/test_structured_mask.py``), for every column order the flash / ring paths present, and
every path fed a StructuredMask computes bit for bit what it computes from that dense tensor."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def _specs(B, T):
    from xdot import StructuredMask

    ln = [max(0, T - 13 - 40 * b) for b in range(B)]
    return {
        "causal": StructuredMask(causal=True),
        "causal_w5": StructuredMask(causal=True, window=5),
        "window70": StructuredMask(window=70),
        "lengths": StructuredMask(lengths=ln),
        "causal_lengths": StructuredMask(causal=True, lengths=ln),
    }


SPEC_NAMES = ["causal", "causal_w5", "window70", "lengths", "causal_lengths"]
# (B, R, T, row_offset): off the 64/128 grid with a partial last word; B = 2; T < 128 (slow path
# only); the exact grid; the middle rank of 3; T % 8 in {0, 4, odd}
SHAPES = [(1, 70, 200, 0), (2, 33, 130, 0), (1, 64, 100, 0), (1, 128, 256, 0), (1, 50, 150, 50),
          (1, 40, 264, 0), (1, 40, 260, 0), (1, 40, 257, 0)]


def _assert_packed_equal(got, ref):
    assert got.shape == ref.shape
    for name in ("bits", "flags", "bits_t"):
        a, b = getattr(got, name), getattr(ref, name)
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert torch.equal(a, b), name


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", SPEC_NAMES)
def test_generated_equals_packed_dense(gpu, name, shape):
    from xdot.ops import flash

    B, R, T, ro = shape
    spec = _specs(B, T)[name]
    got = flash.generate_mask(spec, B, R, T, ro, device=gpu)
    ref = flash.prepare_mask(spec.dense(B, R, T, ro, gpu), B, R, T)
    _assert_packed_equal(got, ref)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("lengths,T", [([0, 37], 130), ([130, 129], 130), ([200, 129], 200)])
def test_lengths_edges(gpu, lengths, T, causal):
    """A fully masked batch, a length crossing a word boundary, nothing masked (lengths = T);
    lengths as a device tensor."""
    from xdot import StructuredMask
    from xdot.ops import flash

    spec = StructuredMask(causal=causal, lengths=torch.tensor(lengths, device=gpu))
    got = flash.generate_mask(spec, 2, 33, T, 0)
    _assert_packed_equal(got, flash.prepare_mask(spec.dense(2, 33, T, 0, gpu), 2, 33, T))


# ---------------------------------------------------------------------------------------------
N, R, RANK, CHUNKS, H_RING = 3, 96, 1, [(0, 48), (48, 48)], 40


def _views():
    from xdot.parallel import attention as pa
    from xdot.parallel.ring import _block_mask

    B = 1

    def own_excluded(r0, rc):  # _own_excluded_mask's view of a user mask
        def view(m):
            m = pa._mask_cols(B, R, N, 0, N, r0, rc)(m).clone()
            m[..., RANK * rc:(RANK + 1) * rc] = True if m.dtype == torch.bool else -1
            return m
        return view

    def old_own_excluded(r0, rc):
        def view(m):
            m = m.reshape(B, R, N, R)[..., 0:N, r0:r0 + rc].reshape(B, R, N * rc).clone()
            m[..., RANK * rc:(RANK + 1) * rc] = True
            return m
        return view

    s0, s1 = 0, 2  # the two lanes' source ranks at some step of the bidirectional ring
    ring = lambda m: torch.cat([_block_mask(m, s0, R, 0, H_RING), _block_mask(m, s1, R, H_RING, R)], -1)  # noqa: E731
    # name -> (view as the package builds it, the pre-StructuredMask statement of it)
    return {
        "mask_cols_peer": (pa._mask_cols(B, R, N, 2, 3, 48, 48),
                           lambda m: m.reshape(B, R, N, R)[..., 2:3, 48:96].reshape(B, R, 48)),
        "mask_cols_chunk": (pa._mask_cols(B, R, N, 0, N, 0, 48),
                            lambda m: m.reshape(B, R, N, R)[..., 0:N, 0:48].reshape(B, R, N * 48)),
        "perm_cols": (pa._perm_cols(B, R, N, CHUNKS),
                      lambda m: torch.cat([m.reshape(B, R, N, R)[..., r0:r0 + rc].reshape(B, R, N * rc)
                                           for r0, rc in CHUNKS], dim=-1)),
        "own_excluded": (own_excluded(48, 48), old_own_excluded(48, 48)),
        "ring_merged": (ring, lambda m: torch.cat([m[..., s0 * R:s0 * R + H_RING], m[..., s1 * R + H_RING:(s1 + 1) * R]], -1)),
    }


VIEW_NAMES = ["mask_cols_peer", "mask_cols_chunk", "perm_cols", "own_excluded", "ring_merged"]


@pytest.mark.parametrize("vname", VIEW_NAMES)
def test_views_unchanged_for_bool_tensors(gpu, vname):
    view, old = _views()[vname]
    g = torch.Generator(device="cpu").manual_seed(3)
    m = (torch.rand(1, R, N * R, generator=g) < 0.4).to(gpu)
    a, b = view(m), old(m)
    assert a.dtype == torch.bool and a.shape == b.shape and torch.equal(a, b)


@pytest.mark.parametrize("vname", VIEW_NAMES)
@pytest.mark.parametrize("name", SPEC_NAMES)
def test_segment_tables(gpu, name, vname):
    from xdot.ops import flash
    from xdot.ops.mask import segments_of

    T = N * R
    spec = _specs(1, T)[name]
    view, _old = _views()[vname]
    dense = view(spec.dense(1, R, T, RANK * R, gpu))
    Tp = dense.shape[-1]
    segs = segments_of(view, T)
    assert 1 <= len(segs) <= 2 * N + 1
    got = flash.generate_mask(spec, 1, R, Tp, RANK * R, segments=segs, device=gpu)
    _assert_packed_equal(got, flash.prepare_mask(dense, 1, R, Tp))
    # and through the cache, as the attention paths ask for it
    flash.MASK_CACHE.clear()
    got = flash.prepare_mask_cached(spec.bind(RANK * R, T), 1, R, Tp, tag=("t", vname), view=view)
    _assert_packed_equal(got, flash.prepare_mask(dense, 1, R, Tp))


def test_own_excluded_without_user_mask(gpu):
    from xdot.ops import flash
    from xdot.parallel import attention as pa

    pa._OWN_EX.clear()
    got = pa._own_excluded_mask(None, 1, R, N, RANK, 48, 48, gpu)
    dense = torch.zeros(1, R, N * 48, dtype=torch.bool, device=gpu)
    dense[..., RANK * 48:(RANK + 1) * 48] = True
    _assert_packed_equal(got, flash.prepare_mask(dense, 1, R, N * 48))
    pa._OWN_EX.clear()


# ---------------------------------------------------------------------------------------------
def _peak_growth(gpu, fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(gpu)
    torch.cuda.reset_peak_memory_stats(gpu)
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(gpu) - base, out


def test_no_dense_allocation(gpu):
    """The packed outputs are ~R*T/4 bytes, a dense bool mask R*T: the peak stays below R*T/2."""
    from xdot import StructuredMask
    from xdot.ops import flash
    from xdot.parallel import attention as pa

    Rb = Tb = 4096
    spec = StructuredMask(causal=True)
    flash.generate_mask(spec, 1, 64, 128, 0, device=gpu)  # the extension, the allocator: warmed
    grown, out = _peak_growth(gpu, lambda: flash.generate_mask(spec, 1, Rb, Tb, 0, device=gpu))
    print(f"generate_mask R=T=4096: peak +{grown} B (dense bool {Rb * Tb} B)")
    assert grown < Rb * Tb // 2
    assert out.bits.numel() * 8 + out.bits_t.numel() * 8 + out.flags.numel() <= grown
    del out
    n, rank, rc = 3, 1, 2048
    pa._OWN_EX.clear()
    grown, out = _peak_growth(gpu, lambda: pa._own_excluded_mask(None, 1, Rb, n, rank, 0, rc, gpu))
    print(f"_own_excluded_mask R=4096 x {n * rc}: peak +{grown} B (dense bool {Rb * n * rc} B)")
    assert grown < Rb * n * rc // 2
    pa._OWN_EX.clear()


# ---------------------------------------------------------------------------------------------
def _same(a, b):
    torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_kernels_see_the_same_mask(gpu, dtype):
    from xdot import StructuredMask
    from xdot.ops import flash

    D, H, B, Rk, T, ro = 96, 2, 1, 96, 288, 96
    C = H * D
    scale = 1.0 / math.sqrt(D)
    g = torch.Generator(device="cpu").manual_seed(5)
    rows, kc, vc, do = (torch.randn(B, s, C, generator=g).to(gpu, dtype) for s in (Rk, T, T, Rk))
    spec = StructuredMask(causal=True)
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


@pytest.mark.parametrize("impl,fused", [("flash", True), ("flash", False), ("ring", True), ("materialized", True)])
def test_module_one_rank(gpu, impl, fused, monkeypatch):
    from xdot import StructuredMask
    from xdot.ops import flash
    from xdot.utils.env import FLAGS

    monkeypatch.setattr(FLAGS, "fused_module", fused)
    flash.MASK_CACHE.clear()
    spec = StructuredMask(causal=True, lengths=[150])
    got = _module_step(gpu, impl, spec)
    ref = _module_step(gpu, impl, spec.dense(1, 200, 200, 0, gpu))
    assert len(got) == len(ref) == 2 + 4
    for a, b in zip(got, ref):
        _same(a, b)
    assert torch.isfinite(got[0].float()).all()  # causal + lengths 150: every row keeps column 0


@pytest.mark.parametrize("impl,chunks,local_first", [("flash", 2, True), ("flash", 1, True), ("flash", 2, False),
                                                     ("ring", None, True)])
def test_module_emulated_middle_rank(gpu, impl, chunks, local_first, monkeypatch):
    """Rank 1 of 3 (EmulatedComm): the own-block-first segmented forward with the merged
    own-excluded chunk masks, gather chunks, the permuted backward; the merged ring.
    ``row_offset=None`` resolves to rank * R."""
    from xdot import StructuredMask
    from xdot.ops import flash
    from xdot.utils.comm import EmulatedComm
    from xdot.utils.env import FLAGS

    monkeypatch.setattr(FLAGS, "local_first", local_first)
    if chunks is not None:
        monkeypatch.setattr(FLAGS, "gather_chunks", chunks)
    flash.MASK_CACHE.clear()
    spec = StructuredMask(causal=True, window=130)
    got = _module_step(gpu, impl, spec, EmulatedComm(N, rank=RANK), chunks, Rm=R)
    dense = spec.dense(1, R, N * R, RANK * R, gpu)
    assert not dense[0, :, RANK * R].any() and dense[0, 0, RANK * R + 1:].all()  # causal from global row 96 on
    ref = _module_step(gpu, impl, dense, EmulatedComm(N, rank=RANK), chunks, Rm=R)
    for a, b in zip(got, ref):
        _same(a, b)
    assert torch.isfinite(got[0].float()).all()


def test_cache(gpu, monkeypatch):
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
    lengths = torch.tensor([150], device=gpu)
    spec = StructuredMask(causal=True, lengths=lengths)
    with torch.no_grad():
        y1 = m(x, x, x, spec)
        n1 = len(calls)
        y2 = m(x, x, x, spec)
        assert n1 == 1 and len(calls) == 1
        _same(y1, y2)
        lengths.add_(1)
        y3 = m(x, x, x, spec)
        assert len(calls) == 2
        ref = m(x, x, x, StructuredMask(causal=True, lengths=[151]).dense(1, 200, 200, 0, gpu))
        _same(y3, ref)
        assert not torch.equal(y3, y1)


def test_cache_keys_on_shape(gpu):
    """One description serves any batch size: a cached packed mask of another shape is not handed out."""
    from xdot import StructuredMask
    from xdot.ops import flash

    flash.MASK_CACHE.clear()
    bound = StructuredMask(causal=True).bind(0, 128)
    for B in (1, 2, 1):
        got = flash.prepare_mask_cached(bound, B, 64, 128)
        _assert_packed_equal(got, flash.prepare_mask(bound.dense(B, 64, 128, 0, gpu), B, 64, 128))
