"""Gated attention on the GPU: the two kernels of ``csrc/gate.hip`` alone against fp64 under the
rounding model of ``tests/_gate_ref.py``, strided views, in-place ``do`` and determinism bitwise, the
module with a gate in exact fp32 and in bf16 against the fp64 definition, an emulated middle rank, a
HIP-graph captured step and the launch accounting."""
import math

import pytest
import torch

import _gate_ref as ref
from _gate_ref import BF16, DT_IDS, F32, FP16

pytestmark = pytest.mark.gpu

KINDS = ["elementwise", "headwise"]
# (B, R, H, dv): a single row and head; batch and head count not powers of two; 12 chunks (60 of 64
# lanes, a ragged last wave); a full 16-chunk head row; more than 64 chunks in 16 bits; more than 64
# chunks in fp32; dv no multiple of the vector width (the unaligned mode); a two-feature head; many
# workgroups and a ragged last one
SHAPES = [(1, 1, 1, 8), (2, 5, 3, 96), (1, 67, 8, 96), (1, 130, 2, 128), (1, 9, 1, 1024), (1, 9, 1, 260),
          (1, 33, 4, 20), (2, 3, 5, 2), (1, 4099, 8, 96)]


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---------------------------------------------------------------------------------- kernels alone
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [F32, BF16, FP16], ids=DT_IDS.get)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels(gpu, shape, dtype, kind):
    """``gate_apply`` and ``gate_backward`` against fp64 within F = 2 times the unit bounds: normal
    draws with planted g in {0, +-30, +-100, +-inf}, zeros and 1e4 in o and one NaN row, which stays
    NaN (and only it); g = +inf gives o bit for bit."""
    from xdot.ops.gate import gate_apply, gate_backward

    B, R, H, D = shape
    o, g, dy = ref.gate_inputs(B, R, H, D, dtype, kind == "headwise", seed=R + D)
    y64, by = ref.ref_apply(o, g, H, dtype)
    do64, dg64, bdo, bdg = ref.ref_backward(dy, o, g, H, dtype)
    og, gg, dyg = o.to(gpu), g.to(gpu), dy.to(gpu)
    y = gate_apply(og, gg, H)
    do, dg = gate_backward(dyg, og, gg, H)
    torch.cuda.synchronize()
    assert y.dtype == dtype and do.dtype == dtype and dg.dtype == dtype and dg.shape == g.shape
    assert torch.equal(_bits(og.cpu()), _bits(o)) and torch.equal(_bits(dyg.cpu()), _bits(dy))  # out of place
    tag = f"{DT_IDS[dtype]} {shape} {kind}"
    ref.check(f"gate_apply o' {tag}", y, y64, by)
    ref.check(f"gate_backward do {tag}", do, do64, bdo)
    ref.check(f"gate_backward dg {tag}", dg, dg64, bdg)
    assert torch.equal(torch.isnan(y.cpu()), torch.isnan(y64)) and not bool(torch.isnan(do).any())
    pick = lambda m: m.unsqueeze(-1).expand(B, R, H, D) if kind == "headwise" else m.view(B, R, H, D)
    sel = pick(g == float("inf"))
    assert torch.equal(_bits(y.cpu().view(B, R, H, D)[sel]), _bits(o.view(B, R, H, D)[sel]))
    off = pick(g == -float("inf")) & ~torch.isnan(o.view(B, R, H, D))  # g = -inf: +-0 with o's sign
    yo, oo = y.cpu().view(B, R, H, D)[off].float(), o.view(B, R, H, D)[off].float()
    assert bool((yo == 0).all()) and torch.equal(torch.signbit(yo), torch.signbit(oo))
    do_off = do.cpu().view(B, R, H, D)[off].float()
    assert bool((do_off == 0).all()) and torch.equal(torch.signbit(do_off), torch.signbit(dy.view(B, R, H, D)[off].float()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [BF16, FP16, F32], ids=DT_IDS.get)
def test_views_in_place_and_determinism(gpu, dtype, kind):
    """``o``, ``o'``, ``do'`` and ``do`` inside wider buffers and ``g`` a column slice give bitwise
    what contiguous copies give and leave the rest of the buffers alone; ``do`` written over ``do'`` is
    bitwise ``do`` out of place; two runs agree bitwise.  A view off 16-byte alignment runs with one
    element per lane step: everything but the headwise ``dg`` is bitwise the aligned result, and the
    headwise ``dg`` -- whose order of summation is that of the lane step -- is bitwise the contiguous
    call at the same lane step (``vec=False``) and inside the model's bounds."""
    from xdot.ops.gate import gate_apply, gate_backward

    B, R, H, D = 2, 37, 3, 96
    C, pad = H * D, 64
    o, g, dy = (t.to(gpu) for t in ref.gate_inputs(B, R, H, D, dtype, kind == "headwise", seed=3))
    y = gate_apply(o, g, H)
    do, dg = gate_backward(dy, o, g, H)
    y2 = gate_apply(o, g, H)
    do2, dg2 = gate_backward(dy, o, g, H)
    for a, b in ((y, y2), (do, do2), (dg, dg2)):
        assert torch.equal(_bits(a), _bits(b))

    def wide(t, fill=7.0):
        w = torch.full((B, R, t.shape[-1] + 2 * pad), fill, dtype=dtype, device=gpu)
        v = w[..., pad:pad + t.shape[-1]]
        v.copy_(t)
        return w, v

    (wo, vo), (wg, vg), (wd, vd) = wide(o), wide(g), wide(dy)
    wy, vy = wide(torch.zeros_like(o))
    wx, vx = wide(torch.zeros_like(o))
    assert not vo.is_contiguous() and not vg.is_contiguous()
    ry = gate_apply(vo, vg, H, out=vy)
    assert ry is vy and torch.equal(_bits(vy), _bits(y))
    rdo, rdg = gate_backward(vd, vo, vg, H, out=vx)
    assert rdo is vx and torch.equal(_bits(vx), _bits(do)) and torch.equal(_bits(rdg), _bits(dg))
    for w in (wo, wg, wd, wy, wx):
        assert bool((w[..., :pad] == 7).all()) and bool((w[..., -pad:] == 7).all())
    # do in place over do', contiguous and in the view
    d1 = dy.clone()
    r1, g1 = gate_backward(d1, o, g, H, out=d1)
    assert r1 is d1 and torch.equal(_bits(d1), _bits(do)) and torch.equal(_bits(g1), _bits(dg))
    r2, g2 = gate_backward(vd, vo, vg, H, out=vd)
    assert torch.equal(_bits(vd), _bits(do)) and torch.equal(_bits(g2), _bits(dg))
    # a view off 16-byte alignment
    w = torch.zeros(B, R, C + 8, dtype=dtype, device=gpu)
    v = w[..., 3:3 + C]
    v.copy_(o)
    assert torch.equal(_bits(gate_apply(v, g, H)), _bits(y))
    r3, g3 = gate_backward(dy, v, g, H)
    assert torch.equal(_bits(r3), _bits(do))
    rs, gs = gate_backward(dy, o, g, H, vec=False)
    assert torch.equal(_bits(rs), _bits(do)) and torch.equal(_bits(g3), _bits(gs))
    assert torch.equal(_bits(gate_apply(o, g, H, vec=False)), _bits(y))
    if kind == "elementwise":
        assert torch.equal(_bits(g3), _bits(dg))
    else:  # (K = D covers the one-element order: D / 64 steps per lane and the tree are shorter)
        _, dg64, _, bdg = ref.ref_backward(dy.cpu(), o.cpu(), g.cpu(), H, dtype, K=D)
        ref.check(f"gate_backward dg headwise, unaligned view {DT_IDS[dtype]}", g3, dg64, bdg)


def test_argument_checks_and_empty(gpu):
    """Bad arguments raise -- the binding's checks, the launcher's own error code turned into an
    exception, outputs that share memory with inputs -- and an empty B or R returns without a launch."""
    from xdot import _ext
    from xdot.ops.gate import gate_apply, gate_backward

    ops = _ext.ops()
    o = torch.zeros(1, 4, 2 * 64, dtype=BF16, device=gpu)
    g = torch.zeros(1, 4, 2, dtype=BF16, device=gpu)
    out = torch.empty_like(o)
    with pytest.raises(RuntimeError, match="g must be"):
        ops.gate_apply(o, torch.zeros(1, 4, 3, dtype=BF16, device=gpu), 2, out)
    with pytest.raises(RuntimeError, match="g must be"):
        ops.gate_apply(o, torch.zeros(1, 5, 2, dtype=BF16, device=gpu), 2, out)
    with pytest.raises(RuntimeError, match="dtype"):
        ops.gate_apply(o, g.float(), 2, out)
    with pytest.raises(RuntimeError, match="H\\*D"):
        ops.gate_apply(o, g, 3, out)
    with pytest.raises(RuntimeError, match="bf16/fp16/fp32"):
        ops.gate_apply(o.double(), g.double(), 2, out.double())
    with pytest.raises(RuntimeError, match="stride 1"):
        ops.gate_apply(torch.zeros(1, 4, 256, dtype=BF16, device=gpu)[..., ::2], g, 2, out)
    with pytest.raises(RuntimeError, match="overlap"):
        ops.gate_apply(o, g, 2, out[:, :1].expand(1, 4, 128))
    with pytest.raises(RuntimeError, match="out must be"):
        ops.gate_apply(o, g, 2, torch.empty(1, 4, 64, dtype=BF16, device=gpu))
    with pytest.raises(RuntimeError, match="dy must be"):
        ops.gate_backward(torch.zeros(1, 3, 128, dtype=BF16, device=gpu), o, g, 2, out)
    # the launcher's own error code (D = 20 is no multiple of the 8-element vector asked for) -> an exception
    o20, g20 = torch.zeros(1, 4, 2 * 20, dtype=BF16, device=gpu), torch.zeros(1, 4, 2, dtype=BF16, device=gpu)
    with pytest.raises(RuntimeError, match="gate_apply: shape"):
        gate_apply(o20, g20, 2, vec=True)
    with pytest.raises(RuntimeError, match="gate_backward: shape"):
        gate_backward(o20, o20, g20, 2, vec=True)
    with pytest.raises(RuntimeError, match="mode"):
        ops.gate_apply(o, g, 2, out, 2)
    with pytest.raises(RuntimeError, match="aligned"):
        gate_apply(torch.zeros(1, 4, 2 * 64 + 8, dtype=BF16, device=gpu)[..., 3:131], g, 2, vec=True)
    # shared memory: out over o or g; dout over part of dy, or over dy with other strides
    with pytest.raises(RuntimeError, match="share memory"):
        ops.gate_apply(o, g, 2, o)
    ge = torch.zeros(1, 4, 128, dtype=BF16, device=gpu)
    with pytest.raises(RuntimeError, match="share memory"):
        ops.gate_apply(o, ge, 2, ge)
    big = torch.zeros(1, 9, 128, dtype=BF16, device=gpu)
    with pytest.raises(RuntimeError, match="dy itself"):
        ops.gate_backward(big[:, 0:4], o, g, 2, big[:, 2:6])
    with pytest.raises(RuntimeError, match="dy itself"):
        ops.gate_backward(big[:, 0:8:2], o, g, 2, big[:, 0:4])
    with pytest.raises(RuntimeError, match="share memory"):
        ops.gate_backward(big[:, 0:4], o, g, 2, o)
    ops.gate_backward(big[:, 0:8:2], o, g, 2, big[:, 0:8:2])  # dy itself, strided: in place
    with pytest.raises(ValueError):
        gate_apply(o, g, 2, out=torch.empty(1, 4, 64, dtype=BF16, device=gpu))
    with pytest.raises(ValueError):
        gate_backward(o[:, :3], o, g, 2)
    for B, R in ((0, 4), (2, 0)):
        e = torch.zeros(B, R, 128, dtype=BF16, device=gpu)
        eg = torch.zeros(B, R, 2, dtype=BF16, device=gpu)
        assert tuple(gate_apply(e, eg, 2).shape) == (B, R, 128)
        do, dg = gate_backward(e, e, eg, 2)
        assert tuple(do.shape) == (B, R, 128) and tuple(dg.shape) == (B, R, 2)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------- module
def _step(m, x, mask):
    x = x.detach().clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    out = m(x, x, x, mask)
    out.float().pow(2).mean().backward()
    torch.cuda.synchronize()
    return out.detach(), x.grad, {n: p.grad for n, p in m.named_parameters()}


def _errors(got, want):
    """As ``tests/test_sinks_gpu.py``: relative Frobenius error per tensor, the gathered side's bias
    against the keys bias gradient's norm."""
    (o, dx, gp), (ro, rdx, rgp) = got, want
    e = {"out": _rel(o, ro), "dx": _rel(dx, rdx)}
    for n, gr in gp.items():
        if n == "queries.bias":
            e[n] = ((gr.double() - rgp[n]).norm() / rgp["keys.bias"].norm()).item()
        else:
            e[n] = _rel(gr, rgp[n])
    return e


def _module(gpu, dtype, key_dim, H, impl, bias, gate, rope=False, Hg=None, sinks=False, qk_norm=False, **kw):
    """The gate projection (the last submodule drawn: the other parameters are the same draws with
    and without a gate) scaled to 4x ``nn.Linear``'s own initialisation, so that the gate is far from
    1/2 and a missing or misplaced gate shows."""
    import xdot

    torch.manual_seed(0)
    m = xdot.DistributedDotProductAttn(key_dim, num_heads=H, impl=impl, add_bias=bias, sinks=sinks, qk_norm=qk_norm,
                                       rope=xdot.Rotary() if rope else None, num_gathered_heads=Hg, gate=gate, **kw)
    with torch.no_grad():
        if sinks:
            m.sinks.copy_(torch.rand(H, generator=torch.Generator().manual_seed(5)) * 2 - 1)
        if gate is not None:
            m.gate.weight.mul_(4.0)
    return m.to(gpu, dtype)


@pytest.mark.parametrize("kind", KINDS)
def test_module_exact_fp32(gpu, kind):
    """Exact fp32 family, D = 96, R = T = 160, causal, rope, sinks: forward and all gradients, the gate
    projection's included, within the 2e-6 relative Frobenius error
    ``tests/test_sinks_gpu.py::test_module_exact_fp32`` holds the same configuration to."""
    import xdot

    m = _module(gpu, F32, 192, 2, "flash", False, kind, rope=True, sinks=True)
    x = torch.randn(1, 160, 192, generator=torch.Generator().manual_seed(1)).to(gpu)
    spec = xdot.StructuredMask(causal=True)
    e = _errors(_step(m, x, spec), ref.dense_run(m, x, spec.dense(1, 160, 160, 0, gpu), rope=True))
    print(f"gate {kind} exact fp32 module errors:", {k: f"{v:.2e}" for k, v in e.items()})
    assert "gate.weight" in e
    for k, v in e.items():
        assert v <= 2e-6, (k, v)


BF16_CASES = {
    "fused": dict(key_dim=768, H=8, impl="flash", fused=True, bias=False),
    "per_op": dict(key_dim=768, H=8, impl="flash", fused=False, bias=False),
    "bias": dict(key_dim=768, H=8, impl="flash", fused=True, bias=True),
    "padded": dict(key_dim=80, H=2, impl="flash", fused=True, bias=False),
    "wide": dict(key_dim=320, H=2, impl="flash", fused=True, bias=False),
    "ring": dict(key_dim=768, H=8, impl="ring", fused=True, bias=False),
    "gqa": dict(key_dim=768, H=8, impl="flash", fused=True, bias=False, Hg=2),
    "sinks_norm_rope": dict(key_dim=768, H=8, impl="flash", fused=True, bias=False, sinks=True, qk_norm=True, rope=True),
}


def _gate_terms(m, x, kind):
    """The gate's own first-order relative (Frobenius) error on ``o'``, and so on everything
    downstream, in fp64 from the module's weights: ``o'`` is rounded once more, 2^-9 per element, and
    ``g`` rounded to bf16 moves ``sigma`` by ``(1 - sigma) |g| 2^-9`` relative -- over the tensor the
    root mean square of that factor weighted by ``sigma^2`` (``o' = sigma o``; the elements where
    ``sigma`` is small carry little of the norm).  The two terms are added, not summed in squares."""
    g = torch.nn.functional.linear(x.double(), m.gate.weight.double(), None if m.gate.bias is None else m.gate.bias.double())
    s = torch.sigmoid(g)
    rms = ((s * (1 - s) * g.abs()).pow(2).sum() / s.pow(2).sum()).sqrt().item()
    return 2.0 ** -9 + rms * 2.0 ** -9


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", list(BF16_CASES))
def test_module_bf16(gpu, case, kind, monkeypatch):
    """T = 320, bf16, a causal window of 96: every tensor's error against its fp64 reference at most
    1.5x that of the same module with ``gate=None`` on the same inputs against ITS reference, plus the
    gate's own first-order terms (:func:`_gate_terms`); ``queries.bias``: the absolute 3e-2 of the keys
    bias gradient's norm, as ``tests/test_sinks_gpu.py::test_module_bf16``.  The gate projection's
    own gradients have no counterpart without a gate: they are held to 1.5x the LARGEST error among the
    yardstick's weight gradients plus the same terms."""
    import xdot
    from xdot.utils.env import FLAGS

    c = BF16_CASES[case]
    monkeypatch.setattr(FLAGS, "fused_module", c["fused"])
    T = 320
    spec = xdot.StructuredMask(causal=True, window=96)
    dense = spec.dense(1, T, T, 0, gpu)
    x = torch.randn(1, T, c["key_dim"], generator=torch.Generator().manual_seed(1)).to(gpu, BF16)
    res = {}
    for gate in (kind, None):
        m = _module(gpu, BF16, c["key_dim"], c["H"], c["impl"], c["bias"], gate, Hg=c.get("Hg"), sinks=c.get("sinks", False),
                    qk_norm=c.get("qk_norm", False), rope=c.get("rope", False))
        got, want = _step(m, x, spec), ref.dense_run(m, x, dense, rope=c.get("rope", False))
        res[gate] = _errors(got, want)
        if gate is not None:
            assert all(bool(torch.isfinite(t).all()) for t in (got[0], got[1], *got[2].values()))
            own = _gate_terms(m, x, kind)
    gated, plain = res[kind], res[None]
    worst_w = max(v for k, v in plain.items() if k.endswith(".weight"))
    for k in gated:
        yard = plain.get(k, worst_w)
        print(f"gate bf16 [{case}] {kind} {k}: gated {gated[k]:.3e}  none {yard:.3e}  ratio {gated[k] / yard:.2f}"
              f"  own terms {own:.2e}")
    assert "gate.weight" in gated
    for k in gated:
        if k == "queries.bias":
            assert gated[k] <= 3e-2, (k, gated[k])
        else:
            assert gated[k] <= 1.5 * plain.get(k, worst_w) + own, (k, gated[k], plain.get(k, worst_w), own)


_RANK_CACHE = {}


@pytest.mark.parametrize("kind", KINDS)
def test_emulated_middle_rank(gpu, kind, monkeypatch):
    """Rank 3 of N = 8 at the benchmark's rank shape (R = 3125, T = 25000, C = 768, H = 8, bf16, causal)
    with a communicator that replays the real peers' ``[q|v]`` blocks, through the fused node and
    through the per-op graph: output, ``dx`` and EVERY parameter gradient of each run against the fp64
    definition of this rank's step (``tests/_gate_ref.py::rank_run``: the rank's rows against the whole
    gathered side, the gathered side's gradient being the rank's own block, as the emulated
    reduce-scatter hands it back).  The bound is the one of ``test_module_bf16``: 1.5x the error of the
    same run with ``gate=None`` against ITS reference, plus the gate's own first-order terms; the gate
    projection's gradients against the largest error among the yardstick's weight gradients; the
    yardstick itself within the 2e-2 the emulated ranks of ``tests/test_sinks_gpu.py`` hold ``out`` to
    and the 3e-2 that ``smoke()`` holds the bf16 module's gradients to.
    Where the two paths are bitwise equal without a gate they must be with one."""
    import xdot
    from xdot.ops import flash
    from xdot.utils.comm import EmulatedComm
    from xdot.utils.env import FLAGS

    N, R, dim, H, rank = 8, 3125, 768, 8, 3
    flash.MASK_CACHE.clear()
    spec = xdot.StructuredMask(causal=True)
    xs = torch.randn(1, N * R, dim, generator=torch.Generator().manual_seed(1)).to(gpu, BF16)
    rows = slice(rank * R, (rank + 1) * R)
    x = xs[:, rows].contiguous()

    class Replay(EmulatedComm):
        def __init__(self, peers):
            super().__init__(N, rank=rank)
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
                if j != rank:
                    ov[j].copy_(self.peers[:, j * R + r0:j * R + r0 + rc])
            return h

    errs, runs = {}, {}
    for gate in (kind, None):
        whole = _module(gpu, BF16, dim, H, "flash", False, gate)
        with torch.no_grad():
            qv = whole._project_qv(xs, xs)
        if gate is None and "none" in _RANK_CACHE:  # (the yardstick's reference: the same for both kinds)
            want = _RANK_CACHE["none"]
        else:
            want = ref.rank_run(whole, x, qv, rank, spec.dense(1, R, N * R, rank * R, gpu))
            want = tuple(t.cpu() if torch.is_tensor(t) else {n: g.cpu() for n, g in t.items()} for t in want)
            if gate is None:
                _RANK_CACHE["none"] = want
            else:
                own = _gate_terms(whole, x, kind)
        for fused in (True, False):
            monkeypatch.setattr(FLAGS, "fused_module", fused)
            m = _module(gpu, BF16, dim, H, "flash", False, gate, comm=Replay(qv))
            got = _step(m, x, spec)
            got = (got[0].cpu(), got[1].cpu(), {n: g.cpu() for n, g in got[2].items()})
            assert all(bool(torch.isfinite(t).all()) for t in (got[0], got[1], *got[2].values()))
            runs[gate, fused], errs[gate, fused] = got, _errors(got, want)
    torch.cuda.empty_cache()
    same = lambda a, b: torch.equal(a[0], b[0]) and all(torch.equal(a[2][n], b[2][n]) for n in a[2])
    held = same(runs[None, True], runs[None, False])
    print(f"gate {kind} emulated rank 3/8: fused == per-op bitwise (out, parameter gradients) without a gate: {held}; "
          f"with: {same(runs[kind, True], runs[kind, False])}")
    if held:
        assert same(runs[kind, True], runs[kind, False])
    for fused in (True, False):
        gated, plain = errs[kind, fused], errs[None, fused]
        worst_w = max(v for k, v in plain.items() if k.endswith(".weight"))
        assert "gate.weight" in gated
        for k in gated:
            yard = plain.get(k, worst_w)
            print(f"gate bf16 emulated rank 3/8 [{'fused' if fused else 'per_op'}] {kind} {k}: gated {gated[k]:.3e}  "
                  f"none {yard:.3e}  ratio {gated[k] / yard:.2f}  own terms {own:.2e}")
        for k, v in plain.items():  # the yardstick itself: out as the emulated ranks, gradients as smoke()
            assert v <= (2e-2 if k == "out" else 3e-2), (k, v)
        for k in gated:
            assert gated[k] <= 1.5 * plain.get(k, worst_w) + own, (fused, k, gated[k], plain.get(k, worst_w), own)


@pytest.mark.parametrize("kind", KINDS)
def test_graph_capture(gpu, kind, monkeypatch):
    """A ``GraphedStep`` capture of a training step with a gate: 2 eager warm-up steps and 2 replays
    equal 4 eager steps bitwise, and the gate projection moves.  Both runs take the configuration a
    capture runs in, as ``tests/test_sinks_gpu.py::test_graph_capture``."""
    import xdot
    from xdot.utils.env import FLAGS
    from xdot.utils.graphs import GraphedStep

    monkeypatch.setattr(FLAGS, "wgrad_side", False)

    def train(graphed, steps=4, warmup=2):
        torch.manual_seed(0)
        m = xdot.DistributedDotProductAttn(256, num_heads=4, impl="flash", gate=kind).to(gpu, BF16)
        w0 = m.gate.weight.detach().clone()
        opt = xdot.FusedAdamW(m.parameters(), lr=1e-2, capturable=True)
        crit = xdot.MSELoss()
        gen = torch.Generator(device=gpu).manual_seed(1)
        x = torch.rand(1, 256, 256, device=gpu, dtype=BF16, generator=gen)
        y = torch.rand(1, 256, 256, device=gpu, dtype=BF16, generator=gen)
        spec = xdot.StructuredMask(causal=True, window=64)

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
        else:
            for i in range(steps):
                opt.zero_grad(set_to_none=True)
                l = body().float().item()
                if i >= warmup:
                    losses.append(l)
        torch.cuda.synchronize()
        return losses, {n: p.detach().clone() for n, p in m.named_parameters()}, w0

    le, pe, w0 = train(False)
    lg, pg, _ = train(True)
    assert len(le) == len(lg) == 2 and math.isfinite(lg[-1])
    assert le == lg, (le, lg)
    for n in pe:
        assert torch.equal(pe[n], pg[n]), n
    assert not torch.equal(pg["gate.weight"], w0)


class _Counting:
    """``torch.ops.xdot`` with every op call counted by name."""

    def __init__(self, ops):
        self._ops, self.calls = ops, {}

    def __getattr__(self, name):
        op = getattr(self._ops, name)

        def call(*a, **k):
            self.calls[name] = self.calls.get(name, 0) + 1
            return op(*a, **k)

        return call


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per_op"])
@pytest.mark.parametrize("impl", ["flash", "ring"])
def test_launch_accounting(gpu, impl, fused, monkeypatch):
    """One step of the one-node module, counted as calls of the ``torch.ops.xdot`` ops as
    ``tests/test_sinks_gpu.py::test_launch_accounting`` does: ``gate=None`` is the list of a module
    built without the keyword; with a gate exactly one ``gate_apply`` in the forward and one
    ``gate_backward`` in the backward, plus EXACTLY the ops of one more projection -- those that
    ``xdot.linear`` on the same input and the gate's weight calls, forward and backward, counted here
    the same way -- and nothing else.  (The add of the gate projection's input gradient into ``dx_k``
    is a torch ``add_``, no ``torch.ops.xdot`` op: this count does not see it; the fused node's one
    ``add_`` is in the code and in ``profiles/gate.md``.)"""
    import xdot
    from xdot import _ext
    from xdot.utils.env import FLAGS

    monkeypatch.setattr(FLAGS, "fused_module", fused)
    x = torch.randn(1, 200, 256, device=gpu).to(BF16).requires_grad_(True)
    counts = {}
    for key, kw in (("elementwise", dict(gate="elementwise")), ("headwise", dict(gate="headwise")), ("off", dict(gate=None)),
                    ("absent", {})):
        torch.manual_seed(0)
        m = xdot.DistributedDotProductAttn(256, num_heads=2, impl=impl, **kw).to(gpu, BF16)
        m(x, x, x, None).float().sum().backward()  # (packed weights built outside the count)
        c = _Counting(_ext.ops())
        with monkeypatch.context() as mp:
            mp.setattr(_ext, "ops", lambda c=c: c)
            out = m(x, x, x, None)
            fwd = dict(c.calls)
            out.float().sum().backward()
            torch.cuda.synchronize()
        counts[key] = (fwd, dict(c.calls))
    assert counts["off"] == counts["absent"]
    fwd0, both0 = counts["absent"]
    assert "gate_apply" not in both0 and "gate_backward" not in both0
    plus = lambda a, b: {k: a.get(k, 0) + b.get(k, 0) for k in set(a) | set(b)}
    for key in ("elementwise", "headwise"):
        fwd, both = counts[key]
        # one more projection of the same shape, on its own
        torch.manual_seed(0)
        w = xdot.DistributedDotProductAttn(256, num_heads=2, impl=impl, gate=key).to(gpu, BF16).gate.weight
        c = _Counting(_ext.ops())
        with monkeypatch.context() as mp:
            mp.setattr(_ext, "ops", lambda c=c: c)
            y = xdot.linear(x, w)
            lin_fwd = dict(c.calls)
            y.float().sum().backward()
            torch.cuda.synchronize()
        lin_both = dict(c.calls)
        print(f"gate launch accounting [{impl} fused={fused}] {key}: one projection = {lin_fwd} forward, {lin_both} in all")
        assert fwd == plus(plus(fwd0, lin_fwd), {"gate_apply": 1}), (fwd, fwd0, lin_fwd)
        assert both == plus(plus(both0, lin_both), {"gate_apply": 1, "gate_backward": 1}), (both, both0, lin_both)
