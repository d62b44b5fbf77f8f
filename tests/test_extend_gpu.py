"""The chunked-prefill kernel (csrc/flash_extend.hip) on the MI355X: more than 64 rows per gathered head
against a cache, within the decode kernel's bounds of the fp64 reference of test_decode_gpu.py."""
import copy
import math

import pytest
import torch

from test_decode_gpu import _check, _inputs, _ref

pytestmark = pytest.mark.gpu

# (B, Tcap, H, Hg, D, Rn): one row over the decode limit with G = 5; a partial second row block with grouped
# heads; several blocks with G = 1; D = 128 over a cache that is no tile multiple.  Every row of every case
# sees a slot (checked on the CPU when the shapes were chosen).
SHAPES = [(1, 200, 5, 1, 32, 13), (2, 1000, 8, 2, 96, 70), (1, 520, 4, 4, 64, 300), (1, 333, 8, 1, 128, 40)]


def _call(gpu, dt, shape, fill):
    B, Tcap, H, Hg, D, Rn = shape
    rows, qv, pos, pos0 = _inputs(gpu, dt, *shape, fill=fill)
    return rows, qv[..., :Hg * D], qv[..., Hg * D:], pos, pos0, 1.0 / math.sqrt(D)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nsplit", [0, 1, 5])
@pytest.mark.parametrize("window", [0, 70])
@pytest.mark.parametrize("fill", ["order", "shuffled"])
def test_extend_kernel(gpu, dt, shape, nsplit, window, fill):
    from xdot.ops import flash

    B, Tcap, H, Hg, D, Rn = shape
    rows, qc, vc, pos, pos0, scale = _call(gpu, dt, shape, fill)
    assert flash.extend_eligible(dt, D, D, H // Hg, Rn)
    out, lse = flash.extend(rows, qc, vc, pos, pos0, H, scale, window=window, Hg=Hg, nsplit=nsplit)
    _check(out, lse, _ref(rows, qc, vc, pos, pos0, window, H, Hg, scale), dt)


def test_extend_is_decodes_route_bitwise_rerun_and_strided_view(gpu):
    from xdot.ops import flash

    B, Tcap, H, Hg, D, Rn = SHAPES[1]
    rows, qc, vc, pos, pos0, scale = _call(gpu, torch.bfloat16, SHAPES[1], "shuffled")
    kw = dict(window=70, Hg=Hg)
    a = flash.extend(rows, qc, vc, pos, pos0, H, scale, **kw)
    same = (flash.decode(rows, qc, vc, pos, pos0, H, scale, **kw) + flash.extend(rows, qc, vc, pos, pos0, H, scale, **kw)
            + flash.extend(rows, qc.contiguous(), vc.contiguous(), pos, pos0, H, scale, **kw))
    for x, y in zip(a + a + a, same):
        assert torch.equal(x, y)
    one, five = (flash.extend(rows, qc, vc, pos, pos0, H, scale, nsplit=ns, **kw) for ns in (1, 5))
    _check(one[0], one[1], (five[0].double(), five[1].double()), torch.bfloat16)


@pytest.mark.parametrize("nsplit", [1, 5])
def test_extend_rows_that_see_nothing(gpu, nsplit):
    """The cache holds positions 100 ..; the rows start at 95: rows 0 .. 4 precede every slot."""
    from xdot.ops import flash

    B, Tcap, H, Hg, D, Rn = SHAPES[2]
    rows, qc, vc, pos, _, scale = _call(gpu, torch.bfloat16, SHAPES[2], "order")
    pos, pos0 = pos + 100, 95
    out, lse = flash.extend(rows, qc, vc, pos, pos0, H, scale, Hg=Hg, nsplit=nsplit)
    assert out[:, :5].isnan().all() and (lse[..., :5] == -float("inf")).all()
    ro, rl = _ref(rows, qc, vc, pos, pos0, 0, H, Hg, scale)
    _check(out[:, 5:], lse[..., 5:], (ro[:, 5:], rl[..., 5:]), torch.bfloat16)


@pytest.mark.parametrize("ws", [1, 3])
def test_module_chunked_prefill(gpu, ws):
    """Prefill 96 tokens into the ranks' caches, append a 40-token chunk (rank 0's cache; G * Rn = 80 rows per
    gathered head) and decode it: against the fp64 single-device module's causal forward."""
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
    with torch.no_grad():
        want = ref(x.double(), x.double(), x.double(), xdot.StructuredMask(causal=True, row_offset=0))[:, T0:]

    def rank_fn(rank):
        mr, R = copy.deepcopy(m), T0 // ws
        cache = mr.new_cache(1, R + n)
        mr.cache_append(cache, x[:, rank * R:(rank + 1) * R], x[:, rank * R:(rank + 1) * R], rank * R)
        if rank == 0:
            mr.cache_append(cache, x[:, T0:], x[:, T0:], T0)
        return mr.decode(x[:, T0:], cache, T0)

    for out in (xdot.ThreadGroup(ws).run(rank_fn) if ws > 1 else [rank_fn(0)]):
        err = ((out.double() - want).norm() / want.norm()).item()
        assert err <= 2e-2, f"{err:.3e}"
