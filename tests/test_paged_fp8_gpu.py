"""The fp8 paged pool on the MI355X (csrc/flash_paged8.hip): the quantising scatter append bitwise against the
torch reference, the block-table fp8 sweep against fp64 over the dequantised pool within the 16-bit paged
kernel's bounds, its gather route, and the module's paged decode path over fp8 pools."""
import copy
import functools
import math

import pytest
import torch

from test_flash_gpu import _close
from test_paged_gpu import FRO, SHAPES, _inputs, _ref

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn


@functools.lru_cache(maxsize=None)
def _fp8_inputs(gpu, dt, shape, perm=0):
    """``test_paged_gpu._inputs`` with every slot's q and v chunk of every gathered head scaled by its own 2^k, k
    in [-3, 3] (drawn from the chunk's first value, so that it belongs to the logical content whatever the
    placement), quantised by the torch reference on the CPU -> (rows, bytes (P, S, C), scales (P, 2*Hg, S), pool_pos,
    table, npages, pos0) and the dequantised pool in fp64.  Computed once per case; tests that write clone."""
    from xdot.parallel import _ref as ref

    B, S, H, Hg, D, Rn = shape
    rows, pool, ppos, table, npages, pos0 = _inputs(gpu, dt, *shape, perm=perm)
    ch = pool.cpu().float().view(*pool.shape[:2], 2 * Hg, D)
    k = (ch[..., :1].abs() * 1000).floor() % 7 - 3
    b8, s = ref.cache_quant((ch * torch.exp2(k)).to(dt).view(pool.shape), Hg)
    return ((rows, b8.to(gpu), s.transpose(1, 2).contiguous().to(gpu), ppos, table, npages, pos0),
            ref.cache_dequant(b8, s, Hg, torch.float64).to(gpu))


def _run(flash, x, H, Hg, scale, **kw):
    rows, b8, sc, ppos, table, npages, pos0 = x
    w = b8.shape[-1] // 2
    return flash.decode_paged(rows, b8[..., :w], b8[..., w:], ppos, table, npages, pos0, H, scale, Hg=Hg,
                              qscale=sc[:, :Hg], vscale=sc[:, Hg:], **kw)


def _check(got, x, deq, window, H, Hg, scale, dt, keep=slice(None), what="paged fp8"):
    (out, lse), (ro, rl) = got, _ref(x[0], deq, *x[3:], window, H, Hg, scale)
    fro = ((out[keep].double() - ro[keep]).norm() / ro[keep].norm()).item()
    print(f"{what} {dt} window={window}: fro {fro:.3e} lse {(lse[keep] - rl[keep].float()).abs().max().item():.3e}")
    _close(what + " out", out[keep], ro[keep].float(), FRO[dt])
    assert (lse[keep] - rl[keep].float()).abs().max().item() < 1e-2, "lse"


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nsplit", [0, 1, 5])
@pytest.mark.parametrize("window", [0, 70])
def test_paged_fp8_kernel(gpu, dt, shape, nsplit, window):
    from xdot.ops import flash

    B, S, H, Hg, D, Rn = shape
    (x, deq), scale = _fp8_inputs(gpu, dt, shape), 1.0 / math.sqrt(D)
    assert flash.decode_paged_eligible(dt, D, D, H // Hg, Rn, S, cache_dtype=F8)
    _check(_run(flash, x, H, Hg, scale, window=window, nsplit=nsplit), x, deq, window, H, Hg, scale, dt)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Hg,D", [(1, 32), (2, 64), (2, 96), (1, 128)])
def test_paged_fp8_scatter_append_bitwise(gpu, dt, Hg, D):
    """Two sequences interleaved: a ragged prefill each (one crosses a page boundary, one from a strided view),
    then a one-token step of both."""
    import xdot
    from xdot.parallel import _ref as ref

    S, C, g = 32, 2 * Hg * D, torch.Generator().manual_seed(D)
    cache = xdot.PagedAttnCache(2, 5, S, Hg, D, dt, device=gpu, cache_dtype="fp8")

    def rows(n):
        x = torch.randn(1, n, 2 * Hg, D, generator=g) * torch.exp2(torch.randint(-10, 11, (1, n, 2 * Hg, 1), generator=g).float())
        x[0, 0, 0] = 0
        wide = torch.zeros(1, n, C + 64, device=gpu, dtype=dt)
        wide[..., 32:32 + C] = x.reshape(1, n, C).to(gpu, dt)
        return wide[..., 32:32 + C]

    xa, xb, xc = rows(37), rows(5), rows(2).transpose(0, 1)
    cache.append_seq(0, xa, 100)
    cache.append_seq(1, xb.contiguous(), torch.tensor([7, 3, 9, 1, 4]))
    cache.append_seq(0, xa[:, :30], 137)
    cache.append(xc, [167, 20])
    want = {0: (torch.cat([xa[0], xa[0, :30], xc[0]]), list(range(100, 168))), 1: (torch.cat([xb[0], xc[1]]), [7, 3, 9, 1, 4, 20])}
    got8, gots, gotp = cache.qv.view(torch.uint8).cpu().clone(), cache.scales.cpu().clone(), cache.pos.cpu().clone()
    for b, (x, p) in want.items():
        b8, s = ref.cache_quant(x.cpu(), Hg)
        i = torch.arange(len(p))
        pg, sl = torch.tensor(cache.pages[b])[i // S], i % S
        assert torch.equal(got8[pg, sl], b8.view(torch.uint8)) and torch.equal(gots[pg, :, sl], s)
        assert gotp[pg, sl].tolist() == p
        got8[pg, sl], gots[pg, :, sl], gotp[pg, sl] = 0, 1, -1
    assert cache.pages == [[0, 1, 3], [2]] and got8.eq(0).all() and gots.eq(1).all() and gotp.eq(-1).all()


@pytest.mark.parametrize("how", ["npages", "pos0"])
def test_paged_fp8_inactive_sequence_sees_nothing(gpu, how):
    from xdot.ops import flash

    B, S, H, Hg, D, Rn = SHAPES[1]
    x, deq = _fp8_inputs(gpu, torch.bfloat16, SHAPES[1])
    x = tuple(t.clone() for t in x)
    if how == "npages":
        x[5][1] = 0
    else:
        x[6][1] = -1
    out, lse = _run(flash, x, H, Hg, 0.1, window=70)
    assert torch.isnan(out[1]).all() and (lse[1] == -float("inf")).all()
    _check((out, lse), x, deq, 70, H, Hg, 0.1, torch.bfloat16, keep=[0, 2])


def test_paged_fp8_placement_does_not_matter_and_rerun_bitwise(gpu):
    from xdot.ops import flash

    B, S, H, Hg, D, Rn = SHAPES[3]
    xa, xb = (_fp8_inputs(gpu, torch.float16, SHAPES[3], perm=p)[0] for p in (0, 1))
    assert not torch.equal(xa[4], xb[4])
    a, b, c = _run(flash, xa, H, Hg, 0.2, window=70), _run(flash, xb, H, Hg, 0.2, window=70), _run(flash, xa, H, Hg, 0.2, window=70)
    for u, v in zip(a + a, b + c):
        assert torch.equal(u, v)


def test_paged_fp8_reads_positions_on_the_device(gpu):
    """The same tensor objects after in-place updates: a generation step changes no argument."""
    from xdot.ops import flash

    B, S, H, Hg, D, Rn = SHAPES[2]
    x, deq = _fp8_inputs(gpu, torch.bfloat16, SHAPES[2])
    x = tuple(t.clone() for t in x)
    rows, b8, sc, ppos, table, npages, pos0 = x
    _check(_run(flash, x, H, Hg, 0.1), x, deq, 0, H, Hg, 0.1, torch.bfloat16)
    pos0 += 5
    npages[1] -= 3
    table[0, 1] = table[1, 38]                    # sequence 0 now reads a page sequence 1 gave up
    _check(_run(flash, x, H, Hg, 0.1), x, deq, 0, H, Hg, 0.1, torch.bfloat16)


@pytest.mark.parametrize("dt,shape", [(torch.float32, (3, 32, 8, 2, 96, 4)), (torch.bfloat16, (2, 128, 5, 1, 32, 13))])
def test_paged_fp8_ineligible_gathers_bytes_and_scales(gpu, dt, shape):
    """fp32 rows (the dense call's dequantising route), and 65 rows per gathered head (csrc/flash_extend8.hip)."""
    from xdot.ops import flash

    B, S, H, Hg, D, Rn = shape
    (x, deq), scale = _fp8_inputs(gpu, dt, shape), 1.0 / math.sqrt(D)
    assert not flash.decode_paged_eligible(dt, D, D, H // Hg, Rn, S, cache_dtype=F8)
    _check(_run(flash, x, H, Hg, scale, window=70), x, deq, 70, H, Hg, scale, dt, what="paged fp8 gathered")


@pytest.mark.parametrize("ws", [1, 3])
def test_module_paged_fp8_prefill_decode_free(gpu, ws):
    """test_module_paged_prefill_decode_free's scenario over fp8 pools, against the fp64 torch module decoding over
    a dense fp8 cache whose bytes, scales and positions are copied from a one-rank GPU fp8 cache holding every
    position of that sequence: the difference is compute only."""
    import xdot

    torch.manual_seed(0)
    kw = dict(num_heads=4, num_gathered_heads=2, rope=xdot.Rotary(), qk_norm=True, sinks=True, gate="headwise")
    m = xdot.DistributedDotProductAttn(256, distributed=ws > 1, **kw).to(gpu, torch.bfloat16)
    with torch.no_grad():
        m.sinks.copy_(torch.linspace(-1.0, 1.0, 4))
    ref = xdot.DistributedDotProductAttn(256, distributed=False, impl="materialized", backend="torch", **kw).to(gpu, torch.float64)
    ref.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    g = torch.Generator().manual_seed(1)
    T = [96, 40, 49]   # sequence 0, sequence 1, and the prompt that replaces sequence 0
    xs = [torch.randn(1, t + 4, 256, generator=g).to(gpu, torch.bfloat16) for t in T]
    m1, want = copy.deepcopy(m), {}
    m1.distributed = False
    for s, x in enumerate(xs):
        whole, rc = m1.new_cache(1, T[s] + 4, cache_dtype="fp8"), ref.new_cache(1, T[s] + 4, cache_dtype="fp8")
        m1.cache_append(whole, x[:, :T[s]], x[:, :T[s]], 0)
        for p in range(T[s], T[s] + 4):
            m1.cache_append(whole, x[:, p:p + 1], x[:, p:p + 1], p)
            rc.qv.copy_(whole.qv), rc.scales.copy_(whole.scales), rc.pos.copy_(whole.pos)
            rc.fill = whole.fill
            want[s, p] = ref.decode(x[:, p:p + 1].double(), rc, p)

    def rank_fn(rank):
        mr = copy.deepcopy(m)
        cache = mr.new_paged_cache(2, {1: 6, 3: 3}[ws], page_size=32, cache_dtype="fp8")   # every page is taken before the free
        assert cache.fp8 and cache.qv.dtype == F8

        def prefill(b, s):
            lo, hi = rank * T[s] // ws, (rank + 1) * T[s] // ws
            mr.cache_append(cache, xs[s][:, lo:hi], xs[s][:, lo:hi], lo, seq=b)

        def step(seqs, pos, owner):
            x = torch.cat([xs[s][:, p:p + 1] for s, p in zip(seqs, pos)])
            if owner == rank:
                mr.cache_append(cache, x, x, pos)
            return seqs, pos, mr.decode(x, cache, pos)

        prefill(0, 0)
        prefill(1, 1)
        outs = [step((0, 1), [T[0] + k, T[1] + k], k % ws) for k in range(3)]
        cache.free(0)
        prefill(0, 2)
        return outs + [step((2, 1), [T[2], T[1] + 3], 0)]

    for outs in (xdot.ThreadGroup(ws).run(rank_fn) if ws > 1 else [rank_fn(0)]):
        for seqs, pos, out in outs:
            for b, (s, p) in enumerate(zip(seqs, pos)):
                err = ((out[b:b + 1].double() - want[s, p]).norm() / want[s, p].norm()).item()
                assert err <= 2e-2, f"sequence {s}, token {p}: {err:.3e}"
