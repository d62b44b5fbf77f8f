"""The fp8 cache on the MI355X (csrc/flash_decode8.hip): the quantising append bitwise against the torch
reference, the fp8 sweep against fp64 over the dequantised cache within the 16-bit kernel's bounds, and the
module's decode path over fp8 caches."""
import copy
import functools
import math

import pytest
import torch

from test_decode_gpu import FRO, SHAPES, _inputs, _ref
from test_flash_gpu import _close

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", [(1, 1, 1, 32), (2, 37, 2, 96), (1, 70, 4, 128), (1, 5, 3, 64)])
def test_cache_quant_kernel_bitwise(gpu, dt, shape):
    import xdot
    from xdot.parallel import _ref as ref

    (B, n, Hg, D), at = shape, 3
    g = torch.Generator().manual_seed(n + D)
    x = torch.randn(B, n, 2 * Hg, D, generator=g) * torch.exp2(torch.randint(-10, 11, (B, n, 2 * Hg, 1), generator=g).float())
    x[0, 0, 0] = 0
    x = x.reshape(B, n, 2 * Hg * D).to(gpu, dt)
    if D == 96:  # a strided view: the [q|v] columns of a wider buffer
        wide = torch.zeros(B, n, 2 * Hg * D + 64, device=gpu, dtype=dt)
        wide[..., 32:32 + 2 * Hg * D] = x
        x = wide[..., 32:32 + 2 * Hg * D]
    cache = xdot.AttnCache(B, n + 9, Hg, D, dt, device=gpu, cache_dtype="fp8")
    cache.fill = at
    cache.append(x, 100)
    b8, s = ref.cache_quant(x.cpu(), Hg)
    got8, gots = cache.qv.view(torch.uint8).cpu(), cache.scales.cpu()
    assert torch.equal(got8[:, at:at + n], b8.view(torch.uint8))
    assert torch.equal(gots[:, :, at:at + n], s.transpose(1, 2))
    for sl in (slice(0, at), slice(at + n, None)):
        assert got8[:, sl].eq(0).all() and gots[:, :, sl].eq(1).all() and cache.pos[:, sl].eq(-1).all()
    assert cache.pos[:, at:at + n].cpu().eq(torch.arange(100, 100 + n, dtype=torch.int32)).all() and cache.fill == at + n


@functools.lru_cache(maxsize=None)
def _fp8_inputs(gpu, dt, shape, fill):
    """``_inputs`` with every slot's q and v chunk scaled by an independent 2^k, k in [-3, 3], quantised by the
    torch reference on the CPU -> rows, bytes, scales (B, 2*Hg, Tcap), the dequantised [q|v] in fp64, col_pos,
    pos0.  Computed once per case and shared; nothing writes to them."""
    from xdot.parallel import _ref as ref

    B, Tcap, H, Hg, D, Rn = shape
    rows, qv, pos, pos0 = _inputs(gpu, dt, *shape, fill=fill)
    k = torch.randint(-3, 4, (B, Tcap, 2 * Hg, 1), generator=torch.Generator().manual_seed(Tcap))
    qv = (qv.cpu().view(B, Tcap, 2 * Hg, D).float() * torch.exp2(k.float())).to(dt).view(B, Tcap, 2 * Hg * D)
    b8, s = ref.cache_quant(qv, Hg)
    return (rows, b8.to(gpu), s.transpose(1, 2).contiguous().to(gpu), ref.cache_dequant(b8, s, Hg, torch.float64).to(gpu),
            pos, pos0)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nsplit", [0, 5])
@pytest.mark.parametrize("window", [0, 70])
@pytest.mark.parametrize("fill", ["order", "shuffled"])
def test_decode_fp8_kernel(gpu, dt, shape, nsplit, window, fill):
    from xdot.ops import flash

    B, Tcap, H, Hg, D, Rn = shape
    rows, b8, sc, deq, pos, pos0 = _fp8_inputs(gpu, dt, shape, fill)
    scale, w = 1.0 / math.sqrt(D), Hg * D
    assert flash.decode_eligible(dt, D, D, H // Hg, Rn, cache_dtype=F8)
    out, lse = flash.decode(rows, b8[..., :w], b8[..., w:], pos, pos0, H, scale, window=window, Hg=Hg, nsplit=nsplit,
                            qscale=sc[:, :Hg], vscale=sc[:, Hg:])
    ro, rl = _ref(rows, deq[..., :w], deq[..., w:], pos, pos0, window, H, Hg, scale)
    fro = ((out.double() - ro).norm() / ro.norm()).item()
    print(f"fp8 decode {dt} {shape} nsplit={nsplit} window={window} {fill}: fro {fro:.3e} lse {(lse - rl.float()).abs().max().item():.3e}")
    _close("decode fp8 out", out, ro.float(), FRO[dt])
    assert (lse - rl.float()).abs().max().item() < 1e-2, "lse"


def test_decode_fp8_strided_view_and_rerun_bitwise(gpu):
    from xdot.ops import flash

    B, Tcap, H, Hg, D, Rn = SHAPES[1]
    rows, b8, sc, _, pos, pos0 = _fp8_inputs(gpu, torch.bfloat16, SHAPES[1], "shuffled")
    qc, vc, kw = b8[..., :Hg * D], b8[..., Hg * D:], dict(window=70, Hg=Hg, qscale=sc[:, :Hg], vscale=sc[:, Hg:])
    a = flash.decode(rows, qc, vc, pos, pos0, H, 0.1, **kw)
    b = flash.decode(rows, qc, vc, pos, pos0, H, 0.1, **kw)
    c = flash.decode(rows, qc.contiguous(), vc.contiguous(), pos, pos0, H, 0.1, **kw)
    for x, y in zip(a + a, b + c):
        assert torch.equal(x, y)


def test_decode_fp8_ineligible_dequantises_and_takes_the_forward_route(gpu):
    from xdot.ops import flash

    dt, shape = torch.bfloat16, (1, 200, 5, 1, 32, 13)
    B, Tcap, H, Hg, D, Rn = shape
    assert not flash.decode_eligible(dt, D, D, H // Hg, Rn, cache_dtype=F8)
    assert all(flash.decode_eligible(dt, s[4], s[4], s[2] // s[3], s[5], cache_dtype=F8) for s in SHAPES)
    rows, b8, sc, deq, pos, pos0 = _fp8_inputs(gpu, dt, shape, "order")
    scale, w = 1.0 / math.sqrt(D), Hg * D
    out, lse = flash.decode(rows, b8[..., :w], b8[..., w:], pos, pos0, H, scale, window=70, Hg=Hg, qscale=sc[:, :Hg], vscale=sc[:, Hg:])
    ro, rl = _ref(rows, deq[..., :w], deq[..., w:], pos, pos0, 70, H, Hg, scale)
    _close("decode fp8 fallback out", out, ro.float(), FRO[dt])
    assert (lse - rl.float()).abs().max().item() < 1e-2, "lse"


@pytest.mark.parametrize("ws", [1, 3])
def test_module_prefill_then_decode_fp8(gpu, ws):
    """test_module_prefill_then_decode's module and steps over fp8 caches, against the fp64 torch module
    decoding over a cache whose bytes, scales and positions are copied from a one-rank GPU fp8 cache holding
    every position: the difference is compute only."""
    import xdot

    torch.manual_seed(0)
    kw = dict(num_heads=4, num_gathered_heads=2, rope=xdot.Rotary(), qk_norm=True, sinks=True, gate="headwise")
    m = xdot.DistributedDotProductAttn(256, distributed=ws > 1, **kw).to(gpu, torch.bfloat16)
    with torch.no_grad():
        m.sinks.copy_(torch.linspace(-1.0, 1.0, 4))
    ref = xdot.DistributedDotProductAttn(256, distributed=False, impl="materialized", backend="torch", **kw).to(gpu, torch.float64)
    ref.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    T0, steps = 96, [(96, 1), (97, 1), (98, 1), (99, 2)]
    x = torch.randn(1, T0 + 5, 256, generator=torch.Generator().manual_seed(1)).to(gpu, torch.bfloat16)
    m1 = copy.deepcopy(m)
    m1.distributed = False
    whole, rc, want = m1.new_cache(1, T0 + 5, cache_dtype="fp8"), ref.new_cache(1, T0 + 5, cache_dtype="fp8"), []
    m1.cache_append(whole, x[:, :T0], x[:, :T0], 0)
    for p, n in steps:
        m1.cache_append(whole, x[:, p:p + n], x[:, p:p + n], p)
        rc.qv.copy_(whole.qv), rc.scales.copy_(whole.scales), rc.pos.copy_(whole.pos)
        rc.fill = whole.fill
        want.append(ref.decode(x[:, p:p + n].double(), rc, p))

    def rank_fn(rank):
        mr, R = copy.deepcopy(m), T0 // ws
        cache = mr.new_cache(1, R + 5, cache_dtype="fp8")
        mr.cache_append(cache, x[:, rank * R:(rank + 1) * R], x[:, rank * R:(rank + 1) * R], rank * R)
        outs = []
        for step, (p, n) in enumerate(steps):
            if step % ws == rank:
                mr.cache_append(cache, x[:, p:p + n], x[:, p:p + n], p)
            outs.append(mr.decode(x[:, p:p + n], cache, p))
        return outs

    for outs in (xdot.ThreadGroup(ws).run(rank_fn) if ws > 1 else [rank_fn(0)]):
        for (p, n), out, w in zip(steps, outs, want):
            err = ((out.double() - w).norm() / w.norm()).item()
            assert err <= 2e-2, f"rows {p}..{p + n - 1}: {err:.3e}"
