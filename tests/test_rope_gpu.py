"""Rotary position embedding on the MI355X: the table and apply kernels (``csrc/rope.hip``)
against fp64, strided views and in-place calls, and the module with ``rope`` set on the flash /
ring paths against the dense fp64 reference of ``tests/_rope_ref.py``."""
import math

import pytest
import torch

from _rope_ref import dense_run

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()


# ---------------------------------------------------------------------------------- table
@pytest.mark.parametrize("R,D,offset", [(1, 2, 0), (33, 96, 0), (257, 40, 199_743), (64, 384, 2_147_483_583)])
def test_table(gpu, R, D, offset):
    """``rope_table`` against the CPU fp64 table: both multiply the same doubles, so the angle is
    identical and what remains is the final rounding: <= 2^-24 (one fp32 ulp in [0.5, 1))."""
    import xdot

    c, s = xdot.Rotary().table(R, D, offset, gpu)
    assert c.dtype == s.dtype == torch.float32 and tuple(c.shape) == tuple(s.shape) == (R, D // 2)
    c64, s64 = xdot.Rotary().table(R, D, offset, "cpu", torch.float64)
    ec, es = (c.cpu().double() - c64).abs().max().item(), (s.cpu().double() - s64).abs().max().item()
    print(f"rope_table R={R} D={D} offset={offset}: max |cos err| {ec:.3e} |sin err| {es:.3e}")
    cc, sc = xdot.Rotary().table(R, D, offset, "cpu")
    assert (c.cpu() - cc).abs().max().item() <= 2.0 ** -24 and (s.cpu() - sc).abs().max().item() <= 2.0 ** -24
    assert ec <= 2.0 ** -24 and es <= 2.0 ** -24


# ---------------------------------------------------------------------------------- apply
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10, torch.float32: 2.0 ** -21}
SHAPES = [(1, 1, 1, 2), (2, 33, 8, 96), (1, 257, 1, 40), (1, 65, 2, 384), (2, 31, 4, 20)]


def _ref64(x, H, c64, s64, inverse, alpha):
    """fp64 rotation of the dtype-rounded input with the fp64 table, and the pair norms."""
    B, R, C = x.shape
    h = C // H // 2
    xv = x.double().cpu().view(B, R, H, 2 * h)
    x1, x2 = xv[..., :h], xv[..., h:]
    c, s = c64.view(1, R, 1, h), (-s64 if inverse else s64).view(1, R, 1, h)
    ref = alpha * torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    hyp = torch.hypot(x1, x2)
    return ref.reshape(B, R, C), torch.cat([hyp, hyp], -1).reshape(B, R, C)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_apply(gpu, dtype, shape):
    """Per element ``|out - ref| <= eps * |alpha| * hypot(x[i], x[i + D/2])``: relative to the
    pair's norm because ``x1 c - x2 s`` can cancel.  eps = 2^-8 bf16 / 2^-10 fp16 (the output's
    final rounding is half of it), 2^-21 fp32 (three roundings plus two table errors of 2^-24)."""
    import xdot

    B, R, H, D = shape
    off = 1000
    rot = xdot.Rotary()
    g = torch.Generator().manual_seed(B * 1000 + R)
    x = torch.randn(B, R, H * D, generator=g).to(gpu, dtype)
    c64, s64 = rot.table(R, D, off, "cpu", torch.float64)
    for inverse in (False, True):
        for alpha in (1.0, 0.1803):
            out = xdot.rope(x, H, rot, offset=off, inverse=inverse, alpha=alpha)
            assert out.dtype == dtype and out.is_contiguous()
            ref, hyp = _ref64(x, H, c64, s64, inverse, alpha)
            err = (out.double().cpu() - ref).abs()
            ratio = (err / (abs(alpha) * hyp).clamp_min(1e-300)).max().item()
            print(f"rope_apply {dtype} {shape} inverse={inverse} alpha={alpha}: max err / (alpha*hypot) {ratio:.3e}")
            assert (err <= EPS[dtype] * abs(alpha) * hyp).all(), ratio
            assert torch.equal(out, xdot.rope(x, H, rot, offset=off, inverse=inverse, alpha=alpha))  # deterministic


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_views(gpu, dtype):
    """Strided views give bitwise the contiguous call's values and touch nothing else."""
    import xdot

    B, R, H, D = 2, 37, 4, 48
    C = H * D
    rot = xdot.Rotary()
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, R, C, generator=g).to(gpu, dtype)
    v = torch.randn(B, R, C, generator=g).to(gpu, dtype)
    want = xdot.rope(x, H, rot, offset=70, alpha=0.25)
    # the q half of a packed [q | v] buffer, in place
    buf = torch.cat([x, v], dim=-1)
    half = buf[..., :C]
    assert xdot.rope(half, H, rot, offset=70, alpha=0.25, out=half) is half
    assert torch.equal(buf[..., :C], want) and torch.equal(buf[..., C:], v)
    # rank slot 1 of a (3, B, R, 2C) gather buffer, in place
    gb = torch.cat([x, v], dim=-1).unsqueeze(0).repeat(3, 1, 1, 1)
    keep = gb.clone()
    slot = gb[1][..., :C]
    xdot.rope(slot, H, rot, offset=70, alpha=0.25, out=slot)
    assert torch.equal(gb[1][..., :C], want) and torch.equal(gb[1][..., C:], v)
    assert torch.equal(gb[0], keep[0]) and torch.equal(gb[2], keep[2])
    # B = 2 with a padded batch stride, out of place and into a strided out
    pad = torch.zeros(B, R + 3, C, device=gpu, dtype=dtype)
    pad[:, :R] = x
    assert torch.equal(xdot.rope(pad[:, :R], H, rot, offset=70, alpha=0.25), want)
    dst = torch.full((B, R + 3, C), 7.0, device=gpu, dtype=dtype)
    xdot.rope(pad[:, :R], H, rot, offset=70, alpha=0.25, out=dst[:, :R])
    assert torch.equal(dst[:, :R], want) and bool((dst[:, R:] == 7).all())
    # a base pointer off the 16-byte grid (scalar path), and in place there
    odd = torch.zeros(B, R, C + 8, device=gpu, dtype=dtype)
    odd[..., 1:1 + C] = x
    assert torch.equal(xdot.rope(odd[..., 1:1 + C], H, rot, offset=70, alpha=0.25), want)
    ov = odd[..., 1:1 + C]
    xdot.rope(ov, H, rot, offset=70, alpha=0.25, out=ov)
    assert torch.equal(odd[..., 1:1 + C], want) and bool((odd[..., 0] == 0).all()) and bool((odd[..., 1 + C:] == 0).all())
    # a row stride off the 16-byte grid: C = 20 in bf16 is 40 bytes a row
    xs = torch.randn(1, 19, 20, generator=g).to(gpu, dtype)
    a = xdot.rope(xs, 1, rot, offset=5)
    b = xdot.rope(torch.cat([xs, xs], -1)[..., :20], 1, rot, offset=5)
    assert torch.equal(a, b)
    # overlapping but different views are refused
    with pytest.raises(RuntimeError):
        xdot.rope(buf[..., :C], H, rot, offset=70, out=buf[..., 8:C + 8])


def test_backward_is_inverse_rotation(gpu):
    import xdot

    rot = xdot.Rotary()
    x = torch.randn(2, 33, 192, device=gpu, dtype=torch.bfloat16).requires_grad_(True)
    gy = torch.randn(2, 33, 192, device=gpu, dtype=torch.bfloat16)
    xdot.rope(x, 2, rot, offset=9, alpha=0.5).backward(gy)
    assert torch.equal(x.grad, xdot.rope(gy, 2, rot, offset=9, alpha=0.5, inverse=True))


# ---------------------------------------------------------------------------------- module
def _step(m, x, mask):
    x = x.detach().clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    out = m(x, x, x, mask)
    out.float().pow(2).mean().backward()
    torch.cuda.synchronize()
    return out.detach(), x.grad, {n: p.grad for n, p in m.named_parameters()}


def _errors(got, ref):
    """Relative Frobenius error per tensor; ``queries.bias`` (zero up to rounding without rope)
    against the keys bias gradient's norm, as ``tests/test_module_gpu.py`` treats it."""
    (o, dx, gp), (ro, rdx, rgp) = got, ref
    e = {"out": _rel(o, ro), "dx": _rel(dx, rdx)}
    for n, gr in gp.items():
        if n == "queries.bias":
            e[n] = ((gr.double() - rgp[n]).norm() / rgp["keys.bias"].norm()).item()
        else:
            e[n] = _rel(gr, rgp[n])
    return e


def test_module_exact_fp32(gpu):
    """Exact fp32 family (``XDOT_FP32_MODE`` default), D = 96, R = T = 160, causal: forward and all
    gradients within the 2e-6 relative Frobenius error ``tests/test_flash_f32_gpu.py`` allows the
    exact kernels (the rotation's own error is 2^-21)."""
    import xdot

    torch.manual_seed(0)
    m = xdot.DistributedDotProductAttn(192, num_heads=2, impl="flash", rope=xdot.Rotary()).to(gpu)
    x = torch.randn(1, 160, 192, generator=torch.Generator().manual_seed(1)).to(gpu)
    spec = xdot.StructuredMask(causal=True)
    e = _errors(_step(m, x, spec), dense_run(m, x, spec.dense(1, 160, 160, 0, gpu)))
    print("rope exact fp32 module errors:", {k: f"{v:.2e}" for k, v in e.items()})
    for k, v in e.items():
        assert v <= 2e-6, (k, v)


BF16_CASES = {
    "fused": dict(key_dim=768, H=8, impl="flash", fused=True, bias=False),
    "per_op": dict(key_dim=768, H=8, impl="flash", fused=False, bias=False),
    "bias": dict(key_dim=768, H=8, impl="flash", fused=True, bias=True),
    "padded": dict(key_dim=80, H=2, impl="flash", fused=True, bias=False),
    "ring": dict(key_dim=768, H=8, impl="ring", fused=True, bias=False),
}


def _bf16_pair(gpu, key_dim, H, impl, bias, T=320, comm=None, rows=None, chunks=None):
    """(errors with rope, errors without) of the bf16 module against the dense fp64 reference of
    each, same weights and inputs.  ``rows`` / ``comm``: an emulated rank's rows of the sequence."""
    import xdot

    res = []
    spec = xdot.StructuredMask(causal=True)
    for rope in (xdot.Rotary(), None):
        kw = {} if comm is None else {"comm": comm(rope)}  # (draws from the global generator: before the seed)
        torch.manual_seed(0)
        m = xdot.DistributedDotProductAttn(key_dim, num_heads=H, impl=impl, add_bias=bias, rope=rope, chunk_plan=chunks,
                                           **kw).to(gpu, torch.bfloat16)
        x = torch.randn(1, T, key_dim, generator=torch.Generator().manual_seed(1)).to(gpu, torch.bfloat16)
        ref = dense_run(m, x, spec.dense(1, T, T, 0, gpu), rope=rope is not None)
        if rows is None:
            res.append(_errors(_step(m, x, spec), ref))
        else:
            with torch.no_grad():
                out = m(x[:, rows], x[:, rows], x[:, rows], spec)
            res.append({"out": _rel(out, ref[0][:, rows])})
    return res


@pytest.mark.parametrize("case", list(BF16_CASES))
def test_module_bf16(gpu, case, monkeypatch):
    """Yardstick: the same module with ``rope=None`` on the same inputs (the behaviour before
    rope existed) against ITS fp64 dense reference.  With rope every tensor's error against its
    reference may be at most 1.5x that: the rotation adds one more bf16 rounding to k and to q
    (about sqrt 2 on the score error) plus margin.  ``queries.bias``: without rope its gradient is
    zero up to rounding, so a ratio says nothing; both runs get the absolute bound
    ``tests/test_module_gpu.py`` gives it (3e-2 of the keys bias gradient's norm)."""
    from xdot.utils.env import FLAGS

    c = BF16_CASES[case]
    monkeypatch.setattr(FLAGS, "fused_module", c["fused"])
    with_rope, without = _bf16_pair(gpu, c["key_dim"], c["H"], c["impl"], c["bias"])
    for k in with_rope:
        print(f"rope bf16 [{case}] {k}: rope {with_rope[k]:.3e}  none {without[k]:.3e}  "
              f"ratio {with_rope[k] / max(without[k], 1e-30):.2f}")
    for k in with_rope:
        if k == "queries.bias":
            assert with_rope[k] <= 3e-2 and without[k] <= 3e-2, (k, with_rope[k], without[k])
        else:
            assert with_rope[k] <= 1.5 * without[k], (k, with_rope[k], without[k])


def _replay_comm(N, RANK, R, peers_of):
    """EmulatedComm whose all-gather hands out the REAL peers' blocks (``peers_of(rope)``: the
    whole sequence's gathered side (1, N*R, 2C), q rotated at its global positions), so that the
    emulated rank's forward is rank ``RANK`` of a true N-rank job.  (The stock EmulatedComm
    replicates the own block, which no N = 1 run equals.)"""
    from xdot.utils.comm import EmulatedComm

    class Replay(EmulatedComm):
        def __init__(self, peers):
            super().__init__(N, rank=RANK)
            self.peers, self.row = peers, 0

        def all_gather_into(self, out, inp, async_op=False):
            rc = inp.shape[1]
            r0 = self.row % R
            self.row += rc
            h = super().all_gather_into(out, inp, async_op=async_op)
            if h is not None:
                h.wait()
            ov = out.view(N, 1, rc, -1)
            for j in range(N):
                if j != RANK:
                    ov[j].copy_(self.peers[:, j * R + r0:j * R + r0 + rc])
            return h

    return lambda rope: Replay(peers_of(rope))


def test_emulated_middle_rank(gpu, monkeypatch):
    """Rank 1 of N = 4 (R = 96, bf16, two gather chunks, own block first) against rows [96, 192)
    of the whole sequence's dense fp64 reference, within the bf16 bound above (1.5x the same
    rank's error with ``rope=None``); and bitwise equal, forward and every gradient, between
    ``StructuredMask(causal=True)`` and its ``dense()`` tensor."""
    import xdot
    from xdot.ops import flash
    from xdot.utils.comm import EmulatedComm
    from xdot.utils.env import FLAGS

    N, RANK, R, dim, H = 4, 1, 96, 192, 2
    monkeypatch.setattr(FLAGS, "gather_chunks", 2)
    monkeypatch.setattr(FLAGS, "fused_module", True)
    flash.MASK_CACHE.clear()

    def peers_of(rope):  # the gathered side of the whole sequence, from the module's own pieces
        torch.manual_seed(0)
        m = xdot.DistributedDotProductAttn(dim, num_heads=H, impl="flash", rope=rope).to(gpu, torch.bfloat16)
        x = torch.randn(1, N * R, dim, generator=torch.Generator().manual_seed(1)).to(gpu, torch.bfloat16)
        with torch.no_grad():
            qv = m._project_qv(x, x)
            if rope is not None:
                q = qv[..., :dim]
                xdot.rope(q, H, rope, offset=0, out=q)
        return qv

    rows = slice(RANK * R, (RANK + 1) * R)
    with_rope, without = _bf16_pair(gpu, dim, H, "flash", False, T=N * R, comm=_replay_comm(N, RANK, R, peers_of),
                                    rows=rows, chunks=2)
    print(f"rope bf16 emulated rank 1/4 out: rope {with_rope['out']:.3e}  none {without['out']:.3e}")
    assert without["out"] <= 2e-2  # the replayed job IS rank 1 of the whole sequence (tests/test_module_gpu.py's bf16 bound)
    assert with_rope["out"] <= 1.5 * without["out"]

    spec = xdot.StructuredMask(causal=True)
    res = []
    for mask in (spec, spec.dense(1, R, N * R, RANK * R, gpu)):
        torch.manual_seed(0)
        m = xdot.DistributedDotProductAttn(dim, num_heads=H, impl="flash", rope=xdot.Rotary(), chunk_plan=2,
                                           comm=EmulatedComm(N, rank=RANK)).to(gpu, torch.bfloat16)
        x = torch.randn(1, R, dim, generator=torch.Generator().manual_seed(1)).to(gpu, torch.bfloat16)
        o, dx, gp = _step(m, x, mask)
        res.append([o, dx] + list(gp.values()))
    for a, b in zip(*res):
        torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)
    assert torch.isfinite(res[0][0].float()).all()


def test_table_cache(gpu):
    """A second forward, and one under ``no_grad``, reuse the cached table: no ``rope_table`` launch."""
    import xdot

    rot = xdot.Rotary()
    torch.manual_seed(0)
    m = xdot.DistributedDotProductAttn(192, num_heads=2, impl="flash", rope=rot).to(gpu, torch.bfloat16)
    x = torch.randn(1, 200, 192, device=gpu, dtype=torch.bfloat16)
    y1 = m(x, x, x, None)
    assert len(rot._tables) == 1
    tabs = {k: (c.data_ptr(), s.data_ptr(), c, s) for k, (c, s) in rot._tables.items()}
    y2 = m(x, x, x, None)
    with torch.no_grad():
        y3 = m(x, x, x, None)
    assert {k: (c.data_ptr(), s.data_ptr(), c, s) for k, (c, s) in rot._tables.items()} == tabs
    assert all(c is rot._tables[k][0] for k, (_, _, c, _) in tabs.items())
    assert torch.equal(y1, y2) and torch.equal(y1, y3)
    m(x[:, :100], x[:, :100], x[:, :100], None)  # another shape: another table
    assert len(rot._tables) == 2


def test_graph_capture(gpu):
    """A ``GraphedStep`` capture of a training step with ``rope`` set replays to the eager result.
    The table is built BEFORE the capture, by GraphedStep's eager warm-up steps (building it needs
    a host-to-device copy of ``inv_freq``, which a capture cannot hold); the captured step finds it
    in the cache and holds the rotation launches only."""
    import xdot
    from xdot.utils.graphs import GraphedStep

    def train(graphed, steps=4, warmup=2):
        torch.manual_seed(0)
        rot = xdot.Rotary()
        m = xdot.DistributedDotProductAttn(256, num_heads=4, impl="flash", rope=rot).to(gpu, torch.bfloat16)
        opt = xdot.FusedAdamW(m.parameters(), lr=1e-3, capturable=graphed)
        crit = xdot.MSELoss()
        g = torch.Generator(device=gpu).manual_seed(1)
        x = torch.rand(1, 256, 256, device=gpu, dtype=torch.bfloat16, generator=g)
        y = torch.rand(1, 256, 256, device=gpu, dtype=torch.bfloat16, generator=g)
        spec = xdot.StructuredMask(causal=True)

        def body():
            loss = crit(m(x, x, x, spec), y)
            loss.backward()
            opt.step()
            return loss

        losses = []
        if graphed:
            st = GraphedStep(body, zero_grad=opt.zero_grad, warmup=warmup)
            for _ in range(steps - warmup):
                losses.append(st().float().item())
            assert len(rot._tables) == 1
        else:
            for i in range(steps):
                opt.zero_grad(set_to_none=True)
                l = body().float().item()
                if i >= warmup:
                    losses.append(l)
        torch.cuda.synchronize()
        return losses, [p.detach().float().clone() for p in m.parameters()]

    le, pe = train(False)
    lg, pg = train(True)
    assert len(le) == len(lg) == 2
    for a, b in zip(le, lg):  # the tolerances of tests/test_graphs_gpu.py
        assert abs(a - b) <= 2e-2 * abs(a) + 1e-6, (le, lg)
    for a, b in zip(pe, pg):
        assert ((a - b).norm() / a.norm()).item() < 1e-2
    assert math.isfinite(lg[-1])
