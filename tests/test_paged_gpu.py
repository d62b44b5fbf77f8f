"""The paged decode kernel (csrc/flash_paged.hip), its fallback and the module's paged decode path on the
MI355X against fp64 torch references, within the dense decode kernel's bounds (test_decode_gpu.py: the
arithmetic per tile is the same)."""
import copy
import math

import pytest
import torch

from test_flash_gpu import _close

pytestmark = pytest.mark.gpu

FRO = {torch.bfloat16: 1e-2, torch.float16: 3e-3, torch.float32: 3e-3}
PAGES = {1: [9], 2: [9, 40], 3: [1, 9, 40]}   # pages of each sequence: under 8 tiles, a few spans, many


def _ref(rows, pool, ppos, table, npages, pos0, window, H, Hg, scale):
    """fp64 per sequence: its pages gathered by the table, dense scores, the visibility rule, softmax, ``@ v``."""
    (B, Rn, C), D, outs, lses = rows.shape, rows.shape[-1] // H, [], []
    for b in range(B):
        pg = table[b, :int(npages[b])].long()
        pg = pg[pg >= 0]
        qv = torch.cat([pool[pg].double().reshape(-1, 2 * Hg * D), pool.new_zeros(1, 2 * Hg * D).double()])  # + one empty slot
        c = torch.cat([ppos[pg].reshape(-1).long(), ppos.new_full((1,), -1).long()]).view(1, -1)
        q, v = (t.reshape(-1, Hg, D).transpose(0, 1).repeat_interleave(H // Hg, dim=0) for t in (qv[:, :Hg * D], qv[:, Hg * D:]))
        p = int(pos0[b]) + torch.arange(Rn, device=rows.device).view(Rn, 1)
        vis = (c >= 0) & (c <= p) & ((c > p - window) if window else (c >= 0)) & (int(pos0[b]) >= 0)
        s = (rows[b].double().view(Rn, H, D).transpose(0, 1) @ q.transpose(-1, -2) * scale).masked_fill(~vis, -float("inf"))
        outs.append((torch.softmax(s, -1) @ v).transpose(0, 1).reshape(Rn, C))
        lses.append(torch.logsumexp(s, -1))
    return torch.stack(outs), torch.stack(lses)


def _inputs(gpu, dt, B, S, H, Hg, D, Rn, perm=0):
    """rows, pool, pool_pos, table, npages, pos0.  The logical content depends on the shape alone, the physical
    pages are permutation ``perm`` of the pool.  Per sequence: a permutation of positions, a fifth of the slots
    empty, the last page filled to a third, one hole in the table of a sequence of 9 pages or more, and its own
    ``pos0``, which is present in logical slot 0."""
    g = torch.Generator().manual_seed(B * S + H * D + Rn)
    npg, C = PAGES[B], 2 * Hg * D
    P, maxp = sum(npg) + 3, max(npg) + 2
    rows = torch.randn(B, Rn, H * D, generator=g)
    phys = torch.randperm(P, generator=torch.Generator().manual_seed(perm)).tolist()
    pool, ppos, table, pos0 = torch.zeros(P, S, C), torch.full((P, S), -1), torch.full((B, maxp), -1), []
    for b, n in enumerate(npg):
        T = n * S
        qv, pos = torch.randn(n, S, C, generator=g), torch.randperm(T, generator=g)
        pos[torch.rand(T, generator=g) < 0.2] = -1
        pos[T - S + S // 3:] = -1
        pos0.append(T // 2 + 11 * b)
        pos[pos == pos0[b]] = -1
        pos[0] = pos0[b]
        pages = [phys.pop() for _ in range(n)]
        pool[pages], ppos[pages], table[b, :n] = qv, pos.view(n, S), torch.tensor(pages)
        if n >= 9:
            table[b, n // 2] = -1
        assert table[b, 0] >= 0 and ppos[table[b, 0], 0] == pos0[b]   # every row sees something: no NaN in the reference
    i32 = dict(device=gpu, dtype=torch.int32)
    return (rows.to(gpu, dt), pool.to(gpu, dt), ppos.to(**i32), table.to(**i32), torch.tensor(npg, **i32), torch.tensor(pos0, **i32))


def _run(flash, x, H, Hg, scale, **kw):
    rows, pool, ppos, table, npages, pos0 = x
    return flash.decode_paged(rows, pool[..., :pool.shape[-1] // 2], pool[..., pool.shape[-1] // 2:], ppos, table, npages, pos0,
                              H, scale, Hg=Hg, **kw)


def _check(out, lse, ref, dt, keep=slice(None)):
    _close("paged out", out[keep], ref[0][keep].float(), FRO[dt])
    assert (lse[keep] - ref[1][keep].float()).abs().max().item() < 1e-2, "lse"


SHAPES = [(1, 32, 4, 4, 64, 1), (3, 32, 8, 2, 96, 4), (2, 128, 8, 1, 128, 2), (3, 64, 8, 1, 32, 3), (2, 256, 4, 2, 96, 8)]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nsplit", [0, 1, 5])
@pytest.mark.parametrize("window", [0, 70])
def test_paged_kernel(gpu, dt, shape, nsplit, window):
    from xdot.ops import flash

    B, S, H, Hg, D, Rn = shape
    x, scale = _inputs(gpu, dt, *shape), 1.0 / math.sqrt(D)
    assert flash.decode_paged_eligible(dt, D, D, H // Hg, Rn, S)
    out, lse = _run(flash, x, H, Hg, scale, window=window, nsplit=nsplit)
    _check(out, lse, _ref(*x, window, H, Hg, scale), dt)


@pytest.mark.parametrize("how", ["npages", "pos0"])
def test_paged_inactive_sequence_sees_nothing(gpu, how):
    from xdot.ops import flash

    B, S, H, Hg, D, Rn = SHAPES[1]
    x = _inputs(gpu, torch.bfloat16, *SHAPES[1])
    if how == "npages":
        x[4][1] = 0
    else:
        x[5][1] = -1
    out, lse = _run(flash, x, H, Hg, 0.1, window=70)
    assert torch.isnan(out[1]).all() and (lse[1] == -float("inf")).all()
    _check(out, lse, _ref(*x, 70, H, Hg, 0.1), torch.bfloat16, keep=[0, 2])


def test_paged_placement_does_not_matter_and_rerun_bitwise(gpu):
    from xdot.ops import flash

    B, S, H, Hg, D, Rn = SHAPES[3]
    xa, xb = (_inputs(gpu, torch.float16, *SHAPES[3], perm=p) for p in (0, 1))
    assert not torch.equal(xa[3], xb[3])
    a, b, c = _run(flash, xa, H, Hg, 0.2, window=70), _run(flash, xb, H, Hg, 0.2, window=70), _run(flash, xa, H, Hg, 0.2, window=70)
    for u, v in zip(a + a, b + c):
        assert torch.equal(u, v)


def test_paged_reads_positions_on_the_device(gpu):
    """The same tensor objects after in-place updates: a generation step changes no argument."""
    from xdot.ops import flash

    B, S, H, Hg, D, Rn = SHAPES[2]
    x = _inputs(gpu, torch.bfloat16, *SHAPES[2])
    rows, pool, ppos, table, npages, pos0 = x
    _check(*_run(flash, x, H, Hg, 0.1), _ref(*x, 0, H, Hg, 0.1), torch.bfloat16)
    pos0 += 5
    npages[1] -= 3
    table[0, 1] = table[1, 38]                    # sequence 0 now reads a page sequence 1 gave up
    pool[table[0, 0].item(), 0] = 0.5             # the slot at the old pos0
    _check(*_run(flash, x, H, Hg, 0.1), _ref(*x, 0, H, Hg, 0.1), torch.bfloat16)


@pytest.mark.parametrize("dt,shape", [(torch.float32, (3, 32, 8, 2, 96, 4)), (torch.bfloat16, (2, 128, 5, 1, 32, 13))])
def test_paged_ineligible_gathers_and_shifts(gpu, dt, shape):
    from xdot.ops import flash

    B, S, H, Hg, D, Rn = shape
    x, scale = _inputs(gpu, dt, *shape), 1.0 / math.sqrt(D)
    assert not flash.decode_paged_eligible(dt, D, D, H // Hg, Rn, S)
    _check(*_run(flash, x, H, Hg, scale, window=70), _ref(*x, 70, H, Hg, scale), dt)


def test_paged_bad_arguments_raise(gpu):
    from xdot import _ext

    B, S, H, Hg, D, Rn = SHAPES[0]
    rows, pool, ppos, table, npages, pos0 = _inputs(gpu, torch.bfloat16, *SHAPES[0])
    q, v, op = pool[..., :Hg * D], pool[..., Hg * D:], _ext.ops().flash_decode_paged
    with pytest.raises(RuntimeError, match="table must be a contiguous int32"):
        op(rows, q, v, ppos, table.long(), npages, pos0, 0, H, 0.125, Hg, 0, False, 0)
    pool48 = torch.zeros(pool.shape[0], 48, pool.shape[2], device=gpu, dtype=pool.dtype)
    with pytest.raises(RuntimeError, match="page size must be 32, 64, 128 or 256"):
        op(rows, pool48[..., :Hg * D], pool48[..., Hg * D:], ppos.new_full((pool.shape[0], 48), -1), table, npages, pos0,
           0, H, 0.125, Hg, 0, False, 0)


@pytest.mark.parametrize("ws", [1, 3])
def test_module_paged_prefill_decode_free(gpu, ws):
    """Prompts of 96 and 40 tokens prefilled into the ranks' paged caches, three tokens decoded for both at once
    (token ``step`` owned by rank ``step % ws``), then sequence 0 freed, a prompt of 49 tokens put into its pages and one more token decoded:
    each output against the fp64 single-device module's causal forward of that sequence alone."""
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
    with torch.no_grad():
        full = [ref(x.double(), x.double(), x.double(), xdot.StructuredMask(causal=True, row_offset=0)) for x in xs]

    def rank_fn(rank):
        mr = copy.deepcopy(m)
        cache = mr.new_paged_cache(2, {1: 6, 3: 3}[ws], page_size=32)   # every page is taken before the free

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
                want = full[s][:, p:p + 1]
                err = ((out[b:b + 1].double() - want).norm() / want.norm()).item()
                assert err <= 2e-2, f"sequence {s}, token {p}: {err:.3e}"
