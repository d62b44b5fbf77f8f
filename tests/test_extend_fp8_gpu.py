"""The chunked-prefill kernel over an fp8 cache (csrc/flash_extend8.hip) on the MI355X: more than 64 rows per
gathered head against e4m3 bytes and per-slot scales, within the 16-bit kernel's bounds of fp64 over the
dequantised cache, and the module's decode path above 64 rows over fp8 caches."""
import copy
import math

import pytest
import torch

from test_decode_fp8_gpu import _fp8_inputs
from test_decode_gpu import _check, _ref
from test_extend_gpu import SHAPES

pytestmark = pytest.mark.gpu


def _call(gpu, dt, shape, fill):
    """rows, q bytes, v bytes, the fp64 dequantised q and v, col_pos, pos0, scale, the scale keywords"""
    B, Tcap, H, Hg, D, Rn = shape
    rows, b8, sc, deq, pos, pos0 = _fp8_inputs(gpu, dt, shape, fill)
    w = Hg * D
    return (rows, b8[..., :w], b8[..., w:], deq[..., :w], deq[..., w:], pos, pos0, 1.0 / math.sqrt(D),
            dict(qscale=sc[:, :Hg], vscale=sc[:, Hg:]))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nsplit", [0, 1, 5])
@pytest.mark.parametrize("window", [0, 70])
@pytest.mark.parametrize("fill", ["order", "shuffled"])
def test_extend_fp8_kernel(gpu, dt, shape, nsplit, window, fill):
    from xdot.ops import flash

    B, Tcap, H, Hg, D, Rn = shape
    rows, qc, vc, dq, dv, pos, pos0, scale, sk = _call(gpu, dt, shape, fill)
    assert flash.extend_fp8_eligible(dt, D, D, H // Hg, Rn)
    out, lse = flash.extend(rows, qc, vc, pos, pos0, H, scale, window=window, Hg=Hg, nsplit=nsplit, **sk)
    _check(out, lse, _ref(rows, dq, dv, pos, pos0, window, H, Hg, scale), dt)


def test_extend_fp8_is_decodes_route_bitwise_rerun_and_strided_view(gpu):
    from xdot.ops import flash

    B, Tcap, H, Hg, D, Rn = SHAPES[1]
    rows, qc, vc, _, _, pos, pos0, scale, sk = _call(gpu, torch.bfloat16, SHAPES[1], "shuffled")
    kw = dict(window=70, Hg=Hg, **sk)
    a = flash.extend(rows, qc, vc, pos, pos0, H, scale, **kw)
    same = (flash.decode(rows, qc, vc, pos, pos0, H, scale, **kw) + flash.extend(rows, qc, vc, pos, pos0, H, scale, **kw)
            + flash.extend(rows, qc.contiguous(), vc.contiguous(), pos, pos0, H, scale, **kw))
    for x, y in zip(a + a + a, same):
        assert torch.equal(x, y)
    one, five = (flash.extend(rows, qc, vc, pos, pos0, H, scale, nsplit=ns, **kw) for ns in (1, 5))
    _check(one[0], one[1], (five[0].double(), five[1].double()), torch.bfloat16)


@pytest.mark.parametrize("nsplit", [1, 5])
def test_extend_fp8_rows_that_see_nothing(gpu, nsplit):
    """The cache holds positions 100 ..; the rows start at 95: rows 0 .. 4 precede every slot."""
    from xdot.ops import flash

    B, Tcap, H, Hg, D, Rn = SHAPES[2]
    rows, qc, vc, dq, dv, pos, _, scale, sk = _call(gpu, torch.bfloat16, SHAPES[2], "order")
    pos, pos0 = pos + 100, 95
    out, lse = flash.extend(rows, qc, vc, pos, pos0, H, scale, Hg=Hg, nsplit=nsplit, **sk)
    assert out[:, :5].isnan().all() and (lse[..., :5] == -float("inf")).all()
    ro, rl = _ref(rows, dq, dv, pos, pos0, 0, H, Hg, scale)
    _check(out[:, 5:], lse[..., 5:], (ro[:, 5:], rl[..., 5:]), torch.bfloat16)


@pytest.mark.parametrize("ws", [1, 3])
def test_module_chunked_prefill_fp8(gpu, ws):
    """test_module_chunked_prefill's module and steps over fp8 caches (G * Rn = 80 rows per gathered head),
    against the fp64 torch module decoding over a cache whose bytes, scales and positions are copied from a
    one-rank GPU fp8 cache holding every position: the difference is compute only."""
    import xdot

    torch.manual_seed(0)
    kw = dict(num_heads=4, num_gathered_heads=2, rope=xdot.Rotary(), qk_norm=True, sinks=True, gate="headwise")
    m = xdot.DistributedDotProductAttn(256, distributed=ws > 1, **kw).to(gpu, torch.bfloat16)
    with torch.no_grad():
        m.sinks.copy_(torch.linspace(-1.0, 1.0, 4))
    ref = xdot.DistributedDotProductAttn(256, distributed=False, impl="materialized", backend="torch", **kw).to(gpu, torch.float64)
    ref.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    T0, n = 96, 40
    x = torch.randn(1, T0 + n, 256, generator=torch.Generator().manual_seed(1)).to(gpu, torch.bfloat16)
    m1 = copy.deepcopy(m)
    m1.distributed = False
    whole, rc = m1.new_cache(1, T0 + n, cache_dtype="fp8"), ref.new_cache(1, T0 + n, cache_dtype="fp8")
    m1.cache_append(whole, x[:, :T0], x[:, :T0], 0)
    m1.cache_append(whole, x[:, T0:], x[:, T0:], T0)
    rc.qv.copy_(whole.qv), rc.scales.copy_(whole.scales), rc.pos.copy_(whole.pos)
    rc.fill = whole.fill
    want = ref.decode(x[:, T0:].double(), rc, T0)

    def rank_fn(rank):
        mr, R = copy.deepcopy(m), T0 // ws
        cache = mr.new_cache(1, R + n, cache_dtype="fp8")
        mr.cache_append(cache, x[:, rank * R:(rank + 1) * R], x[:, rank * R:(rank + 1) * R], rank * R)
        if rank == 0:
            mr.cache_append(cache, x[:, T0:], x[:, T0:], T0)
        return mr.decode(x[:, T0:], cache, T0)

    for out in (xdot.ThreadGroup(ws).run(rank_fn) if ws > 1 else [rank_fn(0)]):
        err = ((out.double() - want).norm() / want.norm()).item()
        assert err <= 2e-2, f"{err:.3e}"
