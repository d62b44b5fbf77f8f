"""Attention sinks on the GPU: the two kernels of ``csrc/sink.hip`` alone against fp64 under the
rounding model of ``tests/_sink_ref.py``, the attention functions and the module with sinks against
the fp64 definition, the fp32 score-buffer and split families, an emulated middle rank, a HIP-graph
captured step and the launch accounting."""
import math

import pytest
import torch

import _sink_ref as ref
from _sink_ref import BF16, DT_IDS, F32, FP16, NINF

pytestmark = pytest.mark.gpu

FOLD_SHAPES = [(1, 1, 1, 32), (2, 37, 3, 96), (1, 130, 8, 96), (1, 65, 2, 160), (1, 33, 1, 384)]


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---------------------------------------------------------------------------------- kernels alone
@pytest.mark.parametrize("sink16", [False, True], ids=["sinks_fp32", "sinks_16bit"])
@pytest.mark.parametrize("dtype", [F32, BF16, FP16], ids=DT_IDS.get)
@pytest.mark.parametrize("shape", FOLD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fold_kernel(gpu, shape, dtype, sink16):
    """``sink_fold`` against fp64 within F = 2 times the unit bounds, |lse - s| up to 6 and up to 200
    in both signs: rows with lse = -inf and NaN in out give exact 0 and lse' == s_h, a head whose
    sink is -inf is left bit for bit (NaN rows included)."""
    from xdot.ops import flash

    B, R, H, D = shape
    sdt = (BF16 if dtype == F32 else dtype) if sink16 else F32
    for gap in (6.0, 200.0):
        out, lse, sinks = ref.fold_inputs(B, R, H, D, dtype, seed=R + int(gap), gap=gap, sink_dtype=sdt)
        o64, l64, g, x = ref.ref_fold(out, lse, sinks, H)
        bo, bl = ref.fold_bounds(o64, l64, g, x, dtype)
        og, lg, sg = out.to(gpu), lse.to(gpu), sinks.to(gpu)
        ro, rl = flash.sink_fold(og, lg, sg, H)
        assert ro is og and rl is lg  # in place
        tag = f"{DT_IDS[dtype]} {shape} gap={gap:g} sinks={DT_IDS[sdt]}"
        ref.check(f"sink_fold o' {tag}", og, o64, bo)
        ref.check(f"sink_fold lse' {tag}", lg, l64, bl)
        ov, lc = og.cpu().view(B, R, H, D), lg.cpu()
        s32 = sinks.float()
        for h in range(H):
            if s32[h] == NINF:  # no sink on this head: nothing was written
                assert torch.equal(_bits(ov[:, :, h]), _bits(out.view(B, R, H, D)[:, :, h]))
                assert torch.equal(lc[:, h], lse[:, h])
                continue
            dead = lse[:, h] == NINF
            assert not bool(torch.isnan(ov[:, :, h]).any())
            if bool(dead.any()):
                assert bool((ov[:, :, h][dead] == 0).all()) and bool((lc[:, h][dead] == s32[h]).all())


def test_fold_minus_inf_is_the_identity_and_views(gpu):
    """All sinks -inf: out and lse bitwise unchanged.  A row-strided view of a wider buffer gives
    bitwise what the contiguous call gives and leaves the rest of the buffer alone."""
    from xdot.ops import flash

    B, R, H, D = 2, 37, 3, 96
    out, lse, sinks = ref.fold_inputs(B, R, H, D, BF16, seed=3)
    og, lg = out.to(gpu), lse.to(gpu)
    flash.sink_fold(og, lg, torch.full((H,), NINF, device=gpu), H)
    assert torch.equal(_bits(og.cpu()), _bits(out)) and torch.equal(lg.cpu(), lse)
    sinks[-1] = 4.0
    oc, lc = out.to(gpu), lse.to(gpu)
    flash.sink_fold(oc, lc, sinks.to(gpu), H)
    wide = torch.full((B, R, H * D + 64), 7.0, dtype=BF16, device=gpu)
    view = wide[..., 32:32 + H * D]
    view.copy_(out.to(gpu))
    lv = lse.to(gpu)
    flash.sink_fold(view, lv, sinks.to(gpu), H)
    assert torch.equal(_bits(view), _bits(oc)) and torch.equal(lv, lc)
    assert bool((wide[..., :32] == 7).all()) and bool((wide[..., 32 + H * D:] == 7).all())


def test_fold_argument_checks(gpu):
    from xdot.ops import flash

    out = torch.zeros(1, 4, 2 * 64, dtype=BF16, device=gpu)
    lse = torch.zeros(1, 2, 4, device=gpu)
    s = torch.zeros(2, device=gpu)
    with pytest.raises(RuntimeError, match="head dim"):
        flash.sink_fold(torch.zeros(1, 4, 2 * 20, dtype=BF16, device=gpu), lse, s, 2)
    with pytest.raises(RuntimeError, match="head dim"):
        flash.sink_fold(torch.zeros(1, 4, 2 * 392, dtype=BF16, device=gpu), lse, s, 2)
    with pytest.raises(RuntimeError, match="sinks"):
        flash.sink_fold(out, lse, torch.zeros(3, device=gpu), 2)
    with pytest.raises(RuntimeError, match="lse"):
        flash.sink_fold(out, torch.zeros(1, 2, 5, device=gpu), s, 2)
    with pytest.raises(RuntimeError, match="aligned"):
        flash.sink_fold(torch.zeros(1, 4, 2 * 64 + 4, dtype=BF16, device=gpu)[..., 4:], lse, s, 2)
    with pytest.raises(RuntimeError, match="bf16/fp16/fp32"):
        flash.sink_fold(out.double(), lse, s, 2)
    with pytest.raises(RuntimeError, match="lse"):
        flash.sink_grad(torch.zeros(1, 2, 4, device=gpu), torch.zeros(1, 2, 5, device=gpu), s)
    assert torch.equal(flash.sink_grad(torch.zeros(0, 2, 4, device=gpu), torch.zeros(0, 2, 4, device=gpu), s),
                       torch.zeros(2, device=gpu))


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 37, 3), (1, 2100, 8), (2, 140000, 2)], ids=lambda s: "x".join(map(str, s)))
def test_grad_kernel(gpu, shape):
    """``sink_grad`` against fp64 within F = 2 times the ordered-sum bound -- one element, ragged
    chunks over two batches, several workgroups per head, more partials than the second stage has
    threads -- with fp32 and bf16 sinks, a head whose sink is -inf (0, whatever delta holds) and
    bitwise equal results of two calls.  (A permutation of the rows changes the order of the sum:
    the model promises no bitwise equality there, determinism is what is tested.)"""
    from xdot.ops import flash

    B, R, H = shape
    gen = torch.Generator().manual_seed(B + R + H)
    lse = 5.0 + torch.randn(B, H, R, generator=gen)
    delta = torch.randn(B, H, R, generator=gen)
    for sdt in (F32, BF16):
        sinks = (5.0 + 6.0 * (2 * torch.rand(H, generator=gen) - 1)).to(sdt)
        l2 = torch.logaddexp(lse, sinks.float().view(1, H, 1))  # a folded lse: >= s
        d = delta.clone()
        if H > 1:
            sinks[-1] = NINF
            d[:, -1, 0] = float("nan")
            l2[:, -1] = lse[:, -1]
        want, term, gapv = ref.ref_grad(torch.where(torch.isnan(d), torch.zeros_like(d), d), l2, sinks)
        a = flash.sink_grad(d.to(gpu), l2.to(gpu), sinks.to(gpu))
        b = flash.sink_grad(d.to(gpu), l2.to(gpu), sinks.to(gpu))
        assert a.dtype == F32 and tuple(a.shape) == (H,) and torch.equal(a, b)
        ref.check(f"sink_grad {shape} sinks={DT_IDS[sdt]}", a, want, ref.grad_bound(term, gapv, B, R))
        if H > 1:
            assert a[-1].item() == 0.0


# ---------------------------------------------------------------------------------- the attention functions
def _fn_inputs(gpu, dt, Hg, kind, seed=0):
    B, R, T, H, D = 1, 160, 160, 4, 64
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(B, R, H * D, generator=g).to(gpu, dt)
    q = torch.randn(B, T, (Hg or H) * D, generator=g).to(gpu, dt)
    v = torch.randn(B, T, (Hg or H) * D, generator=g).to(gpu, dt)
    do = torch.randn(B, R, H * D, generator=g).to(gpu, dt)
    s = (torch.rand(H, generator=g) * 2 - 1).to(gpu)
    if kind == "none":
        mask = dense = None
    elif kind == "window":
        import xdot

        mask = xdot.StructuredMask(causal=True, window=40)
        dense = mask.dense(B, R, T, 0, gpu)
    else:  # random, rows 3 and 130..139 fully masked
        dense = torch.rand(B, R, T, generator=g) < 0.4
        dense[:, 3] = True
        dense[:, 130:140] = True
        mask = dense = dense.to(gpu)
    return k, q, v, do, s, mask, dense, H, D


def _fn_run(f, k, q, v, do, s, mask, H, scale, Hg, with_arg=True):
    from xdot.utils.comm import LocalComm

    kk, qq, vv = (t.detach().clone().requires_grad_(True) for t in (k, q, v))
    ss = None if s is None else s.detach().clone().requires_grad_(True)
    kw = {"sinks": ss} if with_arg else {}
    out = f(kk, qq, vv, mask, H, scale, comm=LocalComm(), gathered_heads=Hg, **kw)
    out.backward(do)
    torch.cuda.synchronize()
    return [out.detach(), kk.grad, qq.grad, vv.grad] + ([ss.grad] if ss is not None else [])


def _fn_check(got, k, q, v, do, s, dense, H, scale, Hg, dt, tag, fro32=2e-6):
    """out / dk / dq / dv: relative Frobenius error (fp32: ``fro32``; 16-bit: the 1e-2 / 3e-3 forward
    and 1.5e-2 / 4e-3 backward of tests/test_flash_gpu.py).  ds: F = 2 times 4 eps E_h in 16 bits (the
    module's bound), ``fro32`` E_h in fp32 (the families' relative error on every term of the sum)."""
    k64, q64, v64, s64 = (t.detach().double().clone().requires_grad_(True) for t in (k, q, v, s))
    want = ref.definition(k64, q64, v64, dense, H, scale, s64, Hg)
    want.backward(do.double())
    E = ref.sink_scale(k, q, v, dense, H, scale, s, do, Hg)
    tol = {F32: (fro32, fro32), BF16: (1e-2, 1.5e-2), FP16: (3e-3, 4e-3)}[dt]
    for name, a, b, t in zip(("out", "dk", "dq", "dv"), got, (want.detach(), k64.grad, q64.grad, v64.grad),
                             (tol[0], tol[1], tol[1], tol[1])):
        assert bool(torch.isfinite(a).all()), f"{tag} {name}: non-finite"
        e = _rel(a, b)
        print(f"sinks fn {tag} {name}: {e:.3e} (allowed {t:.1e})")
        assert e <= t, (tag, name, e)
    unit = (4 * ref.EPS_OUT[dt] if dt != F32 else fro32 / ref.F) * E
    ref.check(f"sinks fn {tag} ds", got[4], s64.grad.cpu(), unit.cpu() + 1e-300)


# (fp32 rows are never pre-scaled: one case)
FN_DTYPES = [(BF16, True), (BF16, False), (FP16, True), (FP16, False), (F32, False)]


@pytest.mark.parametrize("Hg", [None, 2], ids=["mha", "gqa"])
@pytest.mark.parametrize("kind", ["none", "window", "dead_rows"])
@pytest.mark.parametrize("dt,prescale", FN_DTYPES, ids=lambda v: DT_IDS.get(v, "prescaled" if v else "scaled_in_kernel"))
@pytest.mark.parametrize("path", ["flash", "ring"])
def test_functions_with_sinks(gpu, path, dt, kind, Hg, prescale, monkeypatch):
    """``seq_parallel_attention`` / ``ring_attention`` with ``sinks`` on 16-bit and exact-fp32 tensors:
    forward and all four gradients against the fp64 definition, and ``sinks=None`` bitwise equal to
    the call without the argument."""
    from xdot.ops import flash
    from xdot.parallel.attention import seq_parallel_attention
    from xdot.parallel.ring import ring_attention
    from xdot.utils.env import FLAGS

    monkeypatch.setattr(FLAGS, "prescale", prescale)
    flash.MASK_CACHE.clear()
    f = seq_parallel_attention if path == "flash" else ring_attention
    k, q, v, do, s, mask, dense, H, D = _fn_inputs(gpu, dt, Hg, kind)
    scale = 1.0 / math.sqrt(D)
    got = _fn_run(f, k, q, v, do, s, mask, H, scale, Hg)
    _fn_check(got, k, q, v, do, s, dense, H, scale, Hg, dt, f"{path} {DT_IDS[dt]} {kind} Hg={Hg} pre={prescale}")
    if kind != "dead_rows":
        a = _fn_run(f, k, q, v, do, None, mask, H, scale, Hg)
        b = _fn_run(f, k, q, v, do, None, mask, H, scale, Hg, with_arg=False)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


@pytest.mark.parametrize("mode", ["exact_scores", "exact_recompute", "split", "split_scores_off"])
def test_fp32_families(gpu, mode, monkeypatch):
    """The exact family in score-buffer mode (``XDOT_FP32_SCORES=1``: the backward reads the stored S
    with the folded lse') and recomputing, and the split-bf16 family, under their existing bounds
    (2e-6 exact, 2e-5 split: tests/test_flash_f32_gpu.py)."""
    from xdot.ops import flash
    from xdot.parallel.attention import seq_parallel_attention
    from xdot.utils.env import FLAGS

    monkeypatch.setattr(FLAGS, "fp32_scores", mode in ("exact_scores", "split"))
    monkeypatch.setattr(FLAGS, "fp32_mode", "split" if mode.startswith("split") else "exact")
    flash.MASK_CACHE.clear()
    k, q, v, do, s, mask, dense, H, D = _fn_inputs(gpu, F32, None, "dead_rows", seed=2)
    scale = 1.0 / math.sqrt(D)
    got = _fn_run(seq_parallel_attention, k, q, v, do, s, mask, H, scale, None)
    _fn_check(got, k, q, v, do, s, dense, H, scale, None, F32, f"fp32 {mode}", fro32=2e-5 if mode.startswith("split") else 2e-6)


# ---------------------------------------------------------------------------------- module
def _step(m, x, mask):
    x = x.detach().clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    out = m(x, x, x, mask)
    out.float().pow(2).mean().backward()
    torch.cuda.synchronize()
    return out.detach(), x.grad, {n: p.grad for n, p in m.named_parameters()}


def _errors(got, want):
    """As ``tests/test_rope_gpu.py``: relative Frobenius error per tensor, ``queries.bias`` against
    the keys bias gradient's norm."""
    (o, dx, gp), (ro, rdx, rgp) = got, want
    e = {"out": _rel(o, ro), "dx": _rel(dx, rdx)}
    for n, gr in gp.items():
        if n == "queries.bias":
            e[n] = ((gr.double() - rgp[n]).norm() / rgp["keys.bias"].norm()).item()
        else:
            e[n] = _rel(gr, rgp[n])
    return e


def _module(gpu, dtype, key_dim, H, impl, bias, sinks, rope=False, Hg=None, **kw):
    """Sinks drawn uniform in [-1, 1], so that a missing or misplaced sink shows (zeros would hide a
    sign error in all but the few-key rows)."""
    import xdot

    torch.manual_seed(0)
    m = xdot.DistributedDotProductAttn(key_dim, num_heads=H, impl=impl, add_bias=bias, sinks=sinks,
                                       rope=xdot.Rotary() if rope else None, num_gathered_heads=Hg, **kw).to(gpu, dtype)
    if sinks:
        with torch.no_grad():
            m.sinks.copy_((torch.rand(H, generator=torch.Generator().manual_seed(5)) * 2 - 1).to(m.sinks))
    return m


def test_module_exact_fp32(gpu):
    """Exact fp32 family, D = 96, R = T = 160, causal, rope: forward and all gradients, the sinks'
    included, within the 2e-6 relative Frobenius error ``tests/test_rope_gpu.py`` holds the same
    configuration to."""
    import xdot

    m = _module(gpu, F32, 192, 2, "flash", False, True, rope=True)
    x = torch.randn(1, 160, 192, generator=torch.Generator().manual_seed(1)).to(gpu)
    spec = xdot.StructuredMask(causal=True)
    e = _errors(_step(m, x, spec), ref.dense_run(m, x, spec.dense(1, 160, 160, 0, gpu), rope=True))
    print("sinks exact fp32 module errors:", {k: f"{v:.2e}" for k, v in e.items()})
    assert "sinks" in e
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
}


@pytest.mark.parametrize("case", list(BF16_CASES))
def test_module_bf16(gpu, case, monkeypatch):
    """T = 320, bf16, a causal window of 96: every tensor's error against its fp64 reference at most
    1.5x that of the same module without sinks on the same inputs against ITS reference
    (``queries.bias``: the absolute 3e-2 of the keys bias gradient's norm), and ``sinks.grad`` within
    F = 2 times the unit bound 4 * 2^-9 * E_h of tests/_sink_ref.py."""
    import xdot
    from xdot.utils.env import FLAGS

    c = BF16_CASES[case]
    monkeypatch.setattr(FLAGS, "fused_module", c["fused"])
    T = 320
    spec = xdot.StructuredMask(causal=True, window=96)
    dense = spec.dense(1, T, T, 0, gpu)
    x = torch.randn(1, T, c["key_dim"], generator=torch.Generator().manual_seed(1)).to(gpu, BF16)
    res = {}
    for sinks in (True, False):
        m = _module(gpu, BF16, c["key_dim"], c["H"], c["impl"], c["bias"], sinks, Hg=c.get("Hg"))
        got, want = _step(m, x, spec), ref.dense_run(m, x, dense)
        res[sinks] = _errors(got, want)
        if sinks:
            assert all(bool(torch.isfinite(t).all()) for t in (got[0], got[1], *got[2].values()))
            E = ref.sink_grad_scale(m, x, dense)
            ds, ds64 = got[2]["sinks"], want[2]["sinks"]
    with_s, plain = res[True], res[False]
    for k in with_s:
        print(f"sinks bf16 [{case}] {k}: sinks {with_s[k]:.3e}  none {plain.get(k, float('nan')):.3e}")
    ref.check(f"sinks bf16 [{case}] sinks.grad", ds, ds64.cpu(), (4 * ref.EPS_OUT[BF16] * E).cpu())
    for k in with_s:
        if k == "queries.bias":
            assert with_s[k] <= 3e-2, (k, with_s[k])
        elif k in plain:
            assert with_s[k] <= 1.5 * plain[k], (k, with_s[k], plain[k])


@pytest.mark.parametrize("rank", [1, 0])
def test_emulated_rank(gpu, rank, monkeypatch):
    """Rank 1 (a middle rank: own-block-excluded masks) and rank 0 (every peer chunk fully masked for
    all its rows under the causal mask) of N = 4, R = 96, bf16, two gather chunks, with a
    communicator replaying the real peers' blocks, against their rows of the whole sequence's dense
    fp64 reference: finite, and within 1.5x the same rank's error without sinks."""
    import xdot
    from xdot.ops import flash
    from xdot.utils.comm import EmulatedComm
    from xdot.utils.env import FLAGS

    N, R, dim, H = 4, 96, 192, 2
    monkeypatch.setattr(FLAGS, "gather_chunks", 2)
    monkeypatch.setattr(FLAGS, "fused_module", True)
    flash.MASK_CACHE.clear()
    spec = xdot.StructuredMask(causal=True)
    x = torch.randn(1, N * R, dim, generator=torch.Generator().manual_seed(1)).to(gpu, BF16)
    rows = slice(rank * R, (rank + 1) * R)

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

    errs = []
    for sinks in (True, False):
        whole = _module(gpu, BF16, dim, H, "flash", False, sinks)
        with torch.no_grad():
            qv = whole._project_qv(x, x)
        m = _module(gpu, BF16, dim, H, "flash", False, sinks, chunk_plan=2, comm=Replay(qv))
        want = ref.dense_run(whole, x, spec.dense(1, N * R, N * R, 0, gpu))
        with torch.no_grad():
            out = m(x[:, rows], x[:, rows], x[:, rows], spec)
        assert bool(torch.isfinite(out).all())
        errs.append(_rel(out, want[0][:, rows]))
    print(f"sinks bf16 emulated rank {rank}/4 out: sinks {errs[0]:.3e}  none {errs[1]:.3e}")
    assert errs[1] <= 2e-2
    assert errs[0] <= 1.5 * errs[1]


def test_emulated_rank_with_fully_masked_rows(gpu, monkeypatch):
    """A middle rank under a dense mask that masks whole rows everywhere (and so in every chunk): the
    segmented forward's partials are all -inf there, the fold gives exact zeros and finite gradients."""
    from xdot.ops import flash
    from xdot.parallel.attention import seq_parallel_attention
    from xdot.utils.comm import EmulatedComm
    from xdot.utils.env import FLAGS

    N, R, H, D = 4, 96, 2, 64
    monkeypatch.setattr(FLAGS, "gather_chunks", 2)
    flash.MASK_CACHE.clear()
    g = torch.Generator().manual_seed(4)
    k = torch.randn(1, R, H * D, generator=g).to(gpu, BF16).requires_grad_(True)
    q = torch.randn(1, R, H * D, generator=g).to(gpu, BF16).requires_grad_(True)
    v = torch.randn(1, R, H * D, generator=g).to(gpu, BF16).requires_grad_(True)
    s = (torch.rand(H, generator=g) * 2 - 1).to(gpu).requires_grad_(True)
    mask = (torch.rand(1, R, N * R, generator=g) < 0.3).to(gpu)
    mask[:, 5] = True
    mask[:, 40:44] = True
    out = seq_parallel_attention(k, q, v, mask, H, 0.125, comm=EmulatedComm(N, rank=1), sinks=s)
    out.float().sum().backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool((out[:, 5] == 0).all()) and bool((out[:, 40:44] == 0).all())
    for t in (k, q, v, s):
        assert bool(torch.isfinite(t.grad).all())
    plain = seq_parallel_attention(k.detach(), q.detach(), v.detach(), mask, H, 0.125, comm=EmulatedComm(N, rank=1))
    assert bool(torch.isnan(plain[:, 5]).all())


def test_graph_capture(gpu, monkeypatch):
    """A ``GraphedStep`` capture of a training step with sinks: 2 eager warm-up steps and 2 replays
    equal 4 eager steps bitwise, and the sinks move (``sinks.grad`` is refreshed by the replays): the
    fold and the ordered sum are capturable and deterministic.  Both runs take the configuration a
    capture runs in, as ``tests/test_headnorm_gpu.py::test_graph_capture``."""
    import xdot
    from xdot.utils.env import FLAGS
    from xdot.utils.graphs import GraphedStep

    monkeypatch.setattr(FLAGS, "wgrad_side", False)

    def train(graphed, steps=4, warmup=2):
        torch.manual_seed(0)
        m = xdot.DistributedDotProductAttn(256, num_heads=4, impl="flash", sinks=True).to(gpu, BF16)
        opt = xdot.FusedAdamW(m.parameters(), lr=1e-2, capturable=True)
        crit = xdot.MSELoss()
        gen = torch.Generator(device=gpu).manual_seed(1)
        x = torch.rand(1, 256, 256, device=gpu, dtype=BF16, generator=gen)
        y = torch.rand(1, 256, 256, device=gpu, dtype=BF16, generator=gen)
        spec = xdot.StructuredMask(causal=True, window=64)
        seen = []

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
                seen.append(m.sinks.detach().clone())
        else:
            for i in range(steps):
                opt.zero_grad(set_to_none=True)
                l = body().float().item()
                if i >= warmup:
                    losses.append(l)
                    seen.append(m.sinks.detach().clone())
        torch.cuda.synchronize()
        return losses, {n: p.detach().clone() for n, p in m.named_parameters()}, seen

    le, pe, se = train(False)
    lg, pg, sg = train(True)
    assert len(le) == len(lg) == 2 and math.isfinite(lg[-1])
    assert le == lg, (le, lg)
    for n in pe:
        assert torch.equal(pe[n], pg[n]), n
    assert not torch.equal(pg["sinks"], torch.zeros_like(pg["sinks"]))
    assert not torch.equal(sg[0], sg[1]) and all(torch.equal(a, b) for a, b in zip(se, sg))  # updated on every replay


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


@pytest.mark.parametrize("impl", ["flash", "ring"])
def test_launch_accounting(gpu, impl, monkeypatch):
    """One step of the one-node module, counted as calls of the ``torch.ops.xdot`` ops as
    ``tests/test_headnorm_gpu.py::test_launch_accounting`` does: with sinks exactly one more op in the
    forward (``sink_fold``: one launch) and one more in the backward (``sink_grad``: its two
    launches, the partials and their ordered sum); without sinks the list is the one of a module
    built without the argument."""
    import xdot
    from xdot import _ext
    from xdot.utils.env import FLAGS

    monkeypatch.setattr(FLAGS, "fused_module", True)
    x = torch.randn(1, 200, 192, device=gpu).to(BF16).requires_grad_(True)
    counts = {}
    for key, kw in (("sinks", dict(sinks=True)), ("off", dict(sinks=False)), ("absent", {})):
        torch.manual_seed(0)
        m = xdot.DistributedDotProductAttn(192, num_heads=2, impl=impl, **kw).to(gpu, BF16)
        m(x, x, x, None).float().sum().backward()  # (packed weights built outside the count)
        c = _Counting(_ext.ops())
        with monkeypatch.context() as mp:
            mp.setattr(_ext, "ops", lambda c=c: c)
            out = m(x, x, x, None)
            fwd = dict(c.calls)
            out.float().sum().backward()
            torch.cuda.synchronize()
        counts[key] = (fwd, dict(c.calls))
    fwd, both = counts["sinks"]
    assert fwd.get("sink_fold") == 1 and "sink_grad" not in fwd and both.get("sink_grad") == 1 and both["sink_fold"] == 1
    assert counts["off"] == counts["absent"]
    fwd0, both0 = counts["absent"]
    assert "sink_fold" not in both0 and "sink_grad" not in both0
    strip = lambda d: {k: v for k, v in d.items() if k not in ("sink_fold", "sink_grad")}
    assert strip(fwd) == fwd0 and strip(both) == both0, (both, both0)
