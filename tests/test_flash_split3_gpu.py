"""fp32 mode ``split3`` (csrc/flash_x6.hip, ``fp32_mode=2``: three bf16 parts per operand, six bf16 MFMAs
per product) against fp64 torch.

The yardstick, per tensor: errors are the largest deviation from the fp64 reference over the reference's
largest magnitude, and ``err(split3) <= 2 err(exact) + 2^-23`` with the exact family (``fp32_mode=0``) run
on the same inputs.  The factor 2 covers the other accumulation order (six partial products per step,
32-row tiles) over an algorithm whose dropped terms are <= 2^-25 per product; the floor keeps a case
where exact happens to be nearly perfect from failing.  Where it says so, also
``err(split3) <= err(split) / 3``: the two-way arithmetic, or a dropped mid term, fails that.
"""
import functools
import math

import pytest
import torch

import _module_ref as ref

gpu_test = pytest.mark.gpu
B, H, R, T = 2, 2, 161, 203  # ragged 32-row block, two 128-row workgroups; ragged 32-column tile, 4 mask words
BAD_ROW = 100                # the fully masked row


def _err(x, want, ok=None, scale=None):
    d = (x.double() - want).abs()
    scale = (want if ok is None else want[ok]).abs().max() if scale is None else scale
    return ((d if ok is None else d[ok]).max() / scale).item()


def _yardstick(name, got, exact, want, ok=None, split=None, scale=None):
    e3, e0 = _err(got, want, ok, scale), _err(exact, want, ok, scale)
    msg = f"{name}: split3 {e3:.2e} exact {e0:.2e} ratio {e3 / max(e0, 1e-30):.2f}"
    if split is not None:
        es = _err(split, want, ok)
        msg += f" split {es:.2e} split/split3 {es / max(e3, 1e-30):.1f}"
    print(msg)
    assert e3 <= 2 * e0 + 2.0 ** -23, msg
    assert split is None or e3 <= es / 3, msg


@functools.lru_cache(maxsize=None)
def _setup(D, masked, big):
    """Inputs, the fp64 reference and the exact family's results of one case (computed once)."""
    from xdot.ops import flash

    dev, C, scale = torch.device("cuda", 0), H * D, 1.0 / math.sqrt(D)
    g = torch.Generator().manual_seed(D + 2 * masked + big)
    rows, kc, vc, do = (torch.randn(B, n, C, generator=g).to(dev) for n in (R, T, T, R))
    if big:
        rows *= 30.0  # scores span about +-100
    mask = rmask = None
    rok = torch.ones(R, dtype=torch.bool, device=dev)
    if masked:
        mask = torch.rand(B, R, T, generator=g) < 0.3
        mask[:, 32:64, 64:128] = True  # one fully masked 32x64 tile
        mask[:, BAD_ROW] = True        # one fully masked row: NaN in o, -inf in lse
        mask = mask.to(dev)
        # its fp64 row: unmasked and without a gradient (the kernels' masked entries contribute nothing
        # to dq / dv either); the row itself is compared by its NaN / -inf positions, its dk not at all
        rmask = mask.clone()
        rmask[:, BAD_ROW] = False
        rok[BAD_ROW] = False
    k, q, v = (t.double().view(B, -1, H, D).transpose(1, 2).clone().requires_grad_(True) for t in (rows, kc, vc))
    s = (k @ q.transpose(-1, -2)) * scale
    if rmask is not None:
        s = s.masked_fill(rmask.unsqueeze(1), -float("inf"))
    o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, R, C)
    o.backward(do.double() * rok[None, :, None])
    want = dict(o=o.detach(), lse=torch.logsumexp(s, -1).detach(),
                **{n: t.grad.transpose(1, 2).reshape(B, -1, C) for n, t in (("dk", k), ("dq", q), ("dv", v))})
    mk = flash.prepare_mask(mask, B, R, T)
    args = (rows, kc, vc, do, mk, scale)
    return args, want, rok, {fm: _run(args, fm) for fm in (0, 1)}


def _run(args, fm, nsplit=1, dsbuf=None):
    from xdot.ops import flash

    rows, kc, vc, do, mk, scale = args
    o, lse = flash.fwd(rows, kc, vc, mk, H, scale, nsplit=nsplit, fp32_mode=fm)
    dkv, delta = flash.bwd_cols(do, rows, kc, vc, o, lse, mk, H, scale, fp32_mode=fm, dsbuf=dsbuf)
    dk = flash.bwd_rows(do, rows, kc, vc, lse, delta, mk, H, scale, nsplit=nsplit, fp32_mode=fm, dsbuf=dsbuf)
    C = rows.shape[-1]
    return dict(o=o, lse=lse, dk=dk, dq=dkv[..., :C], dv=dkv[..., C:])


@gpu_test
@pytest.mark.parametrize("big", [False, True], ids=["unit", "big"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("D", [32, 64, 96, 128])
def test_kernels(gpu, monkeypatch, D, masked, big):
    """The three kernels directly: forward column splits 1 and 3 (partials + combine), column-kernel row
    splits 1 and 2, the recompute and the dS-only backward (bitwise equal dq / dv), twice for bitwise
    determinism."""
    from xdot.ops import flash

    args, want, rok, base = _setup(D, masked, big)
    exact, split = base[0], (base[1] if not masked and not big else None)
    for csplit, nsplit in (("1", 1), ("2", 3)):
        monkeypatch.setenv("XDOT_CSPLIT", csplit)
        got = _run(args, 2, nsplit)
        dsb = torch.full((flash.score_buffer_numel(B, H, R, T),), float("nan"), device=gpu)  # no stale zeros
        ds = _run(args, 2, nsplit, dsbuf=dsb)
        assert torch.equal(got["dq"], ds["dq"]) and torch.equal(got["dv"], ds["dv"]), "dS-only != recompute"
        again = _run(args, 2, nsplit)
        assert all(torch.equal(again[n].nan_to_num(7.0), got[n].nan_to_num(7.0)) for n in got), "not deterministic"
        for n in ("o", "lse"):  # the fully masked row: NaN / -inf where the exact family has them
            assert torch.equal(got[n].isnan(), exact[n].isnan()) and torch.equal(got[n].isinf(), exact[n].isinf()), n
        tag = f"D={D} {'mask' if masked else 'nomask'} {'big' if big else 'unit'} nsplit={nsplit} csplit={csplit}"
        _yardstick(f"{tag} o", got["o"], exact["o"], want["o"], rok[None, :, None].expand_as(got["o"]), split and split["o"])
        _yardstick(f"{tag} lse", got["lse"], exact["lse"], want["lse"], rok[None, None, :].expand_as(got["lse"]))
        _yardstick(f"{tag} dq", got["dq"], exact["dq"], want["dq"], None, split and split["dq"])
        _yardstick(f"{tag} dv", got["dv"], exact["dv"], want["dv"])
        okk = rok[None, :, None].expand_as(got["dk"])
        _yardstick(f"{tag} dk", got["dk"], exact["dk"], want["dk"], okk)
        _yardstick(f"{tag} dk (dS)", ds["dk"], exact["dk"], want["dk"], okk)


@gpu_test
def test_partial_slots(gpu):
    """``fwd_partial`` over two column segments into slots + combine against the one-launch forward."""
    from xdot.ops import flash

    (rows, kc, vc, do, mk, scale), want, rok, base = _setup(96, False, False)
    C, cut = rows.shape[-1], 128
    opart = torch.empty(3, B, R, C, device=gpu)
    lpart = torch.empty(3, B, H, R, device=gpu)
    flash.fwd_partial(rows, kc[:, :cut], vc[:, :cut], None, H, scale, opart, lpart, 0, 2, fp32_mode=2)
    flash.fwd_partial(rows, kc[:, cut:], vc[:, cut:], None, H, scale, opart, lpart, 2, 1, fp32_mode=2)
    o, lse = flash.fwd_combine(opart, lpart, H, rows)
    _yardstick("partial o", o, base[0]["o"], want["o"], None, base[1]["o"])
    _yardstick("partial lse", lse, base[0]["lse"], want["lse"])


@gpu_test
@pytest.mark.parametrize("causal", [False, True], ids=["nomask", "causal"])
@pytest.mark.parametrize("kind", ["flash", "gqa", "ring"])
def test_module(gpu, monkeypatch, kind, causal):
    """``DistributedDotProductAttn(192, num_heads=2, distributed=False)`` in fp32 under ``split3``: output,
    input gradient and every parameter gradient under the yardstick of the same module under ``exact``."""
    import xdot
    from xdot.utils.env import FLAGS

    torch.manual_seed(0)
    m = xdot.DistributedDotProductAttn(192, num_heads=2, distributed=False, impl="ring" if kind == "ring" else "flash",
                                       num_gathered_heads=1 if kind == "gqa" else None).to(gpu)
    x = torch.randn(1, 160, 192, generator=torch.Generator().manual_seed(1)).to(gpu)
    spec = xdot.StructuredMask(causal=True) if causal else None

    def step(mode):
        monkeypatch.setattr(FLAGS, "fp32_mode", mode)
        xr = x.clone().requires_grad_(True)
        m.zero_grad(set_to_none=True)
        out = m(xr, xr, xr, spec)
        out.pow(2).mean().backward()
        return dict(out=out.detach(), dx=xr.grad, **{n: p.grad for n, p in m.named_parameters()})

    got, exact = step("split3"), step("exact")
    wo, wdx, wp = ref.dense_run(m, x, spec.dense(1, 160, 160, 0, gpu) if causal else None)
    want = dict(out=wo, dx=wdx, **wp)
    for n in got:
        # queries.bias: exactly zero in exact arithmetic (softmax shift invariance), held against the keys bias
        _yardstick(f"module {kind} {n}", got[n], exact[n], want[n],
                   scale=want["keys.bias"].abs().max() if n == "queries.bias" else None)


@gpu_test
def test_refusals(gpu):
    from xdot.ops import flash

    rows, kc = torch.randn(1, 64, 128, device=gpu), torch.randn(1, 96, 128, device=gpu)
    with pytest.raises(ValueError, match="exact.*split.*split3"):
        flash.fp32_code(torch.float32, "split4")
    with pytest.raises(RuntimeError, match="fp32_mode"):
        flash.fwd(rows, kc, kc, None, 2, 0.1, fp32_mode=3)
    with pytest.raises(RuntimeError, match="no S buffer"):
        flash.fwd(rows, kc, kc, None, 2, 0.1, fp32_mode=2, sbuf=torch.empty(flash.score_buffer_numel(1, 2, 64, 96), device=gpu))


def test_three_way_split_identity():
    """The scheme in torch, on the CPU: three bf16 parts sum to x within 2^-24 |x| (random, huge and tiny
    normal inputs), and the six-term product beats the plain fp32 matmul against fp64."""
    def parts(x):
        h = x.bfloat16().float()
        m = (x - h).bfloat16().float()
        return h, m, (x - h - m).bfloat16().float()

    g = torch.Generator().manual_seed(0)
    for s in (1.0, 1e30, 1e-30):
        x = torch.randn(4096, generator=g) * s
        assert ((sum(p.double() for p in parts(x)) - x.double()).abs() <= 2.0 ** -24 * x.double().abs()).all(), s
    a, b = torch.randn(64, 96, generator=g), torch.randn(96, 64, generator=g)
    (ah, am, al), (bh, bm, bl) = parts(a), parts(b)
    six = sum(x.double() @ y.double() for x, y in ((al, bh), (ah, bl), (am, bm), (am, bh), (ah, bm), (ah, bh)))
    want = a.double() @ b.double()
    assert (six - want).abs().max() < ((a @ b).double() - want).abs().max()
