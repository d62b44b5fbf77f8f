"""The decode kernel (csrc/flash_decode.hip) and the module's decode path on the MI355X against fp64
torch references, within the forward bounds of test_flash_gpu.py / test_module_gpu.py."""
import copy
import math

import pytest
import torch

from test_flash_gpu import _close

pytestmark = pytest.mark.gpu

FRO = {torch.bfloat16: 1e-2, torch.float16: 3e-3, torch.float32: 3e-3}


def _ref(rows, qc, vc, col_pos, pos0, window, H, Hg, scale):
    """fp64: dense scores, the visibility rule from ``col_pos``, softmax, ``@ v``."""
    (B, Rn, C), D = rows.shape, rows.shape[-1] // H
    k = rows.double().view(B, Rn, H, D).transpose(1, 2)
    q, v = (t.double().reshape(B, -1, Hg, D).transpose(1, 2).repeat_interleave(H // Hg, dim=1) for t in (qc, vc))
    p = pos0 + torch.arange(Rn, device=rows.device).view(1, Rn, 1)
    c = col_pos.long().unsqueeze(1)
    vis = (c >= 0) & (c <= p) & ((c > p - window) if window else (c >= 0))
    s = (k @ q.transpose(-1, -2) * scale).masked_fill(~vis.unsqueeze(1), -float("inf"))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, Rn, C), torch.logsumexp(s, -1)


def _inputs(gpu, dt, B, Tcap, H, Hg, D, Rn, fill="order"):
    """rows, one [q|v] buffer, col_pos, pos0.  ``order``: batch b holds positions 0 .. Tcap - 37 b - 1 in
    order; ``shuffled``: a permutation of positions with a fifth of the slots and the whole second of five
    spans empty.  Position pos0 is always present."""
    g = torch.Generator().manual_seed(B * Tcap + H * D + Rn)
    rows = torch.randn(B, Rn, H * D, generator=g).to(gpu, dt)
    qv = torch.randn(B, Tcap, 2 * Hg * D, generator=g).to(gpu, dt)
    if fill == "order":
        pos = torch.arange(Tcap).repeat(B, 1)
        for b in range(B):
            pos[b, Tcap - 37 * b:] = -1
        pos0 = Tcap - 37 * (B - 1) - Rn
    else:
        pos0, span = Tcap // 2, 32 * math.ceil(math.ceil(Tcap / 32) / 5)
        pos = torch.stack([torch.randperm(Tcap, generator=g) for _ in range(B)])
        pos[torch.rand(B, Tcap, generator=g) < 0.2] = -1
        pos[:, span:2 * span] = -1
        pos[pos == pos0] = -1
        pos[:, 0] = pos0
    return rows, qv, pos.to(gpu, torch.int32), pos0


def _check(out, lse, ref, dt):
    _close("decode out", out, ref[0].float(), FRO[dt])
    assert (lse - ref[1].float()).abs().max().item() < 1e-2, "lse"


SHAPES = [(1, 200, 4, 4, 64, 1), (2, 1000, 8, 2, 96, 4), (1, 333, 8, 1, 128, 2), (1, 777, 8, 1, 32, 3), (1, 520, 4, 2, 96, 8)]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nsplit", [0, 1, 5])
@pytest.mark.parametrize("window", [0, 70])
@pytest.mark.parametrize("fill", ["order", "shuffled"])
def test_decode_kernel(gpu, dt, shape, nsplit, window, fill):
    from xdot.ops import flash

    B, Tcap, H, Hg, D, Rn = shape
    rows, qv, pos, pos0 = _inputs(gpu, dt, *shape, fill=fill)
    qc, vc, scale = qv[..., :Hg * D], qv[..., Hg * D:], 1.0 / math.sqrt(D)
    assert flash.decode_eligible(dt, D, D, H // Hg, Rn)
    out, lse = flash.decode(rows, qc, vc, pos, pos0, H, scale, window=window, Hg=Hg, nsplit=nsplit)
    _check(out, lse, _ref(rows, qc, vc, pos, pos0, window, H, Hg, scale), dt)


def test_decode_strided_view_and_rerun_bitwise(gpu):
    from xdot.ops import flash

    B, Tcap, H, Hg, D, Rn = SHAPES[1]
    rows, qv, pos, pos0 = _inputs(gpu, torch.bfloat16, *SHAPES[1], fill="shuffled")
    qc, vc = qv[..., :Hg * D], qv[..., Hg * D:]
    a = flash.decode(rows, qc, vc, pos, pos0, H, 0.1, window=70, Hg=Hg)
    b = flash.decode(rows, qc, vc, pos, pos0, H, 0.1, window=70, Hg=Hg)
    c = flash.decode(rows, qc.contiguous(), vc.contiguous(), pos, pos0, H, 0.1, window=70, Hg=Hg)
    for x, y in zip(a + a, b + c):
        assert torch.equal(x, y)


@pytest.mark.parametrize("dt,shape", [(torch.float32, (1, 200, 4, 4, 64, 1)), (torch.bfloat16, (1, 200, 5, 1, 32, 13))])
def test_decode_ineligible_takes_the_forward_route(gpu, dt, shape):
    from xdot.ops import flash

    B, Tcap, H, Hg, D, Rn = shape
    rows, qv, pos, pos0 = _inputs(gpu, dt, *shape)
    qc, vc, scale = qv[..., :Hg * D], qv[..., Hg * D:], 1.0 / math.sqrt(D)
    assert not flash.decode_eligible(dt, D, D, H // Hg, Rn)
    out, lse = flash.decode(rows, qc, vc, pos, pos0, H, scale, window=70, Hg=Hg)
    _check(out, lse, _ref(rows, qc, vc, pos, pos0, 70, H, Hg, scale), dt)


def test_decode_wrong_col_pos_raises(gpu):
    from xdot.ops import flash

    B, Tcap, H, Hg, D, Rn = SHAPES[0]
    rows, qv, pos, pos0 = _inputs(gpu, torch.bfloat16, *SHAPES[0])
    with pytest.raises(RuntimeError, match="col_pos must be a contiguous int32"):
        flash.decode(rows, qv[..., :Hg * D], qv[..., Hg * D:], pos[:, :-1], pos0, H, 0.125, Hg=Hg)


@pytest.mark.parametrize("ws", [1, 3])
def test_module_prefill_then_decode(gpu, ws):
    """Prefill 96 tokens into the ranks' caches, decode 3 tokens one at a time (token ``step`` owned by rank
    ``step % ws``) and 2 rows at once: each output against the fp64 single-device module's causal forward."""
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
    with torch.no_grad():
        full = ref(x.double(), x.double(), x.double(), xdot.StructuredMask(causal=True, row_offset=0))

    def rank_fn(rank):
        mr, R = copy.deepcopy(m), T0 // ws
        cache = mr.new_cache(1, R + 5)
        mr.cache_append(cache, x[:, rank * R:(rank + 1) * R], x[:, rank * R:(rank + 1) * R], rank * R)
        outs = []
        for step, (p, n) in enumerate(steps):
            if step % ws == rank:
                mr.cache_append(cache, x[:, p:p + n], x[:, p:p + n], p)
            outs.append(mr.decode(x[:, p:p + n], cache, p))
        return outs

    for outs in (xdot.ThreadGroup(ws).run(rank_fn) if ws > 1 else [rank_fn(0)]):
        for (p, n), out in zip(steps, outs):
            want = full[:, p:p + n]
            err = ((out.double() - want).norm() / want.norm()).item()
            assert err <= 2e-2, f"rows {p}..{p + n - 1}: {err:.3e}"
