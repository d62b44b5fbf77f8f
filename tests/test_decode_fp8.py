"""The fp8 cache on the CPU (the torch path): the quantiser ``_ref.cache_quant`` against its format, and the
module decoding over an fp8 cache against the same module over that cache's dequantised values."""
import copy

import pytest
import torch

import xdot
from xdot.parallel import _ref


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_ref_cache_quant_round_trip(dt):
    """Chunks at scales over about +-10 binades, one all zero, one holding the dtype's largest finite value:
    every element is RNE to e4m3 (3 mantissa bits, subnormal spacing 2^-9) of x / s, and s = amax / 448."""
    Hg, D, n = 2, 32, 24
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, 2 * Hg, D, generator=g) * torch.exp2(torch.randint(-10, 11, (n, 2 * Hg, 1), generator=g).float())
    x[1, 2] = 0
    x = x.to(dt)
    x[2, 1, 5] = torch.finfo(dt).max
    b8, s = _ref.cache_quant(x.reshape(n, 2 * Hg * D), Hg)
    assert b8.dtype == torch.float8_e4m3fn and b8.shape == (n, 2 * Hg * D) and s.shape == (n, 2 * Hg) and s.dtype == torch.float32
    amax = x.float().abs().amax(-1)
    want_s = amax * (torch.tensor(1.0) / 448)
    want_s[1, 2] = 1.0
    assert torch.equal(s, want_s)
    assert b8.view(torch.uint8).reshape(n, 2 * Hg, D)[1, 2].eq(0).all()
    r = x.double() / s.double().unsqueeze(-1)
    q8 = b8.double().reshape(n, 2 * Hg, D)
    bound = torch.maximum(r.abs() * 2.0 ** -4, torch.full_like(r, 2.0 ** -10)) * (1 + 2.0 ** -20)
    assert ((r - q8).abs() <= bound).all(), ((r - q8).abs() / bound).max().item()
    assert q8.abs().max().item() == 448.0


@pytest.mark.parametrize("ws", [1, 3])
def test_module_decode_over_fp8_cache_equals_dequantised_cache(ws):
    """The same code after dequantisation: catches swapped q / v halves, per-head scale indexing and append
    offsets."""
    torch.manual_seed(0)
    m0 = xdot.DistributedDotProductAttn(64, num_heads=4, num_gathered_heads=2, distributed=ws > 1, rope=xdot.Rotary(),
                                        qk_norm=True, sinks=True)
    with torch.no_grad():
        m0.sinks.copy_(torch.linspace(-1.0, 1.0, 4))
    T0, steps = 24, [(24, 1), (25, 1), (26, 2)]
    x = torch.randn(2, T0 + 4, 64, generator=torch.Generator().manual_seed(1))

    def rank_fn(rank):
        m, R = copy.deepcopy(m0), T0 // ws
        c8 = m.new_cache(2, R + 5, cache_dtype="fp8")
        assert c8.qv.dtype == torch.float8_e4m3fn and c8.scales.shape == (2, 4, R + 5) and c8.dtype == torch.float32
        assert c8.scales.eq(1).all() and c8.qv.view(torch.uint8).eq(0).all()
        errs = []
        m.cache_append(c8, x[:, rank * R:(rank + 1) * R], x[:, rank * R:(rank + 1) * R], rank * R)
        for step, (p, n) in enumerate(steps):
            if step % ws == rank:
                m.cache_append(c8, x[:, p:p + n], x[:, p:p + n], p)
            plain = m.new_cache(2, R + 5)
            plain.append(torch.cat(c8.dequant(), dim=-1)[:, :c8.fill], c8.pos[0, :c8.fill])
            a, b = m.decode(x[:, p:p + n], c8, p), m.decode(x[:, p:p + n], plain, p)
            errs.append(((a - b).norm() / b.norm()).item())
        return errs

    for errs in (xdot.ThreadGroup(ws).run(rank_fn) if ws > 1 else [rank_fn(0)]):
        assert max(errs) <= 1e-6, errs
