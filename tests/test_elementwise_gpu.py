"""The softmax, AdamW, partial-sum, prescale and MSE kernels (csrc/softmax.hip, csrc/optim.hip,
csrc/reduce.hip) against fp64 references under the rounding models of tests/_elementwise.py (GPU only).

Softmax: every edge of the seven dispatch branches (the parametrize id names the branch and whether
the case takes the vector or the scalar loads), two batches so that the mask row map's batch term
counts, every mask form, misaligned views, dead rows, -inf inputs, a negative scale and element
offsets past 2^31.  AdamW: one step from a hand-set state (so that an update of lr cannot hide under
a tolerance), sizes around the 1024-element block, 40 tensors (two launches), misaligned views, fp32
gradients, the capturable path, and a three-step run that a kernel writing nothing fails.  The sums
and the prescale are compared bitwise.  Every case prints its ratios to the unit bounds (``-s``)."""
import pytest
import torch

import _elementwise as ew
from _elementwise import BF16, F32, FP16

pytestmark = pytest.mark.gpu

DT_PARAMS = pytest.mark.parametrize("dtype", ew.DTYPES, ids=ew.DT_IDS.values())
DT16_PARAMS = pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
EDGE_PARAMS = pytest.mark.parametrize("T", ew.EDGE_CASES, ids=ew.case_id)


def _report(kernel, case, dtype, ratios):
    print(f"\nRATIO kernel={kernel} case={case} dtype={ew.DT_IDS[dtype]} " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))


def _worse(worst, r, prefix=""):
    for k, v in r.items():
        worst[prefix + k] = max(v, worst.get(prefix + k, 0.0))


# ---- softmax -------------------------------------------------------------------------------------------
def _softmax(what, x, mask, scale, backward=True):
    """Forward (elements, row sums, exact zeros / NaN rows) and backward on the kernel's own y."""
    from xdot.ops.softmax import scale_mask_softmax_bwd, scale_mask_softmax_fwd

    y = scale_mask_softmax_fwd(x, mask, scale)
    assert y.dtype == x.dtype and y.shape == x.shape
    r = ew.assert_ratios(f"{what} forward", ew.softmax_fwd_ratios(y, x, mask, scale))
    if backward:
        dy = ew.make_dy(x).to(x.device)
        dx = scale_mask_softmax_bwd(y, dy, scale)
        assert dx.dtype == x.dtype and dx.shape == x.shape
        r.update(ew.assert_ratios(f"{what} backward", ew.softmax_bwd_ratios(dx, y, dy, scale)))
    return y, r


def _scores(gpu, T, dtype, **kw):
    x, mask = ew.make_scores(T, dtype, **kw)
    return x.to(gpu), mask.to(gpu)


@DT_PARAMS
@pytest.mark.parametrize("T", ew.ALL_T, ids=ew.case_id)
def test_softmax_fwd_bwd(gpu, T, dtype):
    """No mask and the (B, R, T) mask with 30 % hidden, randn * 3 scores, scale 0.37."""
    x, mask = _scores(gpu, T, dtype)
    worst = {}
    _worse(worst, _softmax("no mask", x, None, ew.SCALE)[1])
    _worse(worst, _softmax("(B, R, T) mask", x, mask, ew.SCALE)[1], "masked_")
    _report("softmax", ew.case_id(T), dtype, worst)


@DT_PARAMS
@pytest.mark.parametrize("branch", ew.BRANCHES)
def test_softmax_amplitude_60(gpu, branch, dtype):
    """Scores of +-80 nats, the hidden entries another 370 nats above them (a max taken before the mask
    leaves no live probability), at the largest T of the branch."""
    T = ew.BRANCH_T[branch][-1]
    x, mask = _scores(gpu, T, dtype, amp=60.0, hidden_lift=1000.0)
    _report("softmax-amp60", ew.case_id(T), dtype, _softmax("amplitude 60", x, mask, ew.SCALE)[1])


@DT_PARAMS
@EDGE_PARAMS
def test_softmax_mask_forms(gpu, T, dtype):
    """(B, 1, R, T) gives bitwise what (B, R, T) gives; a mask of the scores' shape differs per head;
    2-D scores with a 2-D mask."""
    x, mask = _scores(gpu, T, dtype)
    worst = {}
    y3, _ = _softmax("(B, R, T)", x, mask, ew.SCALE, backward=False)
    y4, r = _softmax("(B, 1, R, T)", x, mask.unsqueeze(1), ew.SCALE, backward=False)
    assert torch.equal(y3, y4)
    _worse(worst, r)
    g = torch.Generator(device="cpu").manual_seed(T)
    full = (torch.rand(x.shape, generator=g) < 0.3).to(gpu)
    full[..., 0] = False
    _worse(worst, _softmax("same shape", x, full, ew.SCALE, backward=False)[1], "same_")
    _worse(worst, _softmax("2-D", x[1, 1], full[1, 1], ew.SCALE, backward=False)[1], "2d_")
    _report("softmax-mask-forms", ew.case_id(T), dtype, worst)


def _offset_copy(t, elems=1):
    """A contiguous copy of ``t`` that starts ``elems`` elements into its storage."""
    buf = torch.empty(t.numel() + elems, dtype=t.dtype, device=t.device)
    view = buf[elems:].view(t.shape)
    view.copy_(t)
    return view


@DT_PARAMS
@EDGE_PARAMS
def test_softmax_misaligned_views(gpu, T, dtype):
    """x one element, then the mask one byte, into their storage: the scalar loads and stores also
    where T % 8 == 0; the backward with dy offset.  (Not bitwise the aligned run: in fp16 the two
    instantiations round the product with 1 / sum differently, once or twice, on a few elements.)"""
    from xdot.ops.softmax import scale_mask_softmax_bwd

    x, mask = _scores(gpu, T, dtype)
    xo, mo = _offset_copy(x), _offset_copy(mask)
    assert xo.data_ptr() % 16 and mo.data_ptr() % 8 and xo.is_contiguous() and mo.is_contiguous()
    worst = {}
    for what, xs, ms in (("x offset", xo, mask), ("mask offset", x, mo)):
        y, r = _softmax(what, xs, ms, ew.SCALE, backward=False)
        _worse(worst, r)
    dy = _offset_copy(ew.make_dy(x).to(gpu))
    dx = scale_mask_softmax_bwd(y, dy, ew.SCALE)
    _worse(worst, ew.assert_ratios("dy offset", ew.softmax_bwd_ratios(dx, y, dy, ew.SCALE)))
    _report("softmax-misaligned", ew.case_id(T), dtype, worst)


@DT_PARAMS
@EDGE_PARAMS
def test_softmax_special_rows(gpu, T, dtype):
    """A fully masked row (NaN on that row of every head only), a row whose only live column is T - 1,
    and a row whose maximum sits in the last 8-group of the row (ragged when T is odd)."""
    x, mask = _scores(gpu, T, dtype)
    mask[0, 0] = True
    mask[0, 1] = True
    mask[0, 1, T - 1] = False
    mask[1, 2, T - 1] = False
    x[1, :, 2, T - 1] = 40.0
    y, r = _softmax("special rows", x, mask, ew.SCALE, backward=False)
    assert torch.isnan(y[0, :, 0]).all() and int(torch.isnan(y).sum()) == x.shape[1] * T
    assert (y[0, :, 1, T - 1] == 1).all() and (y[0, :, 1, :T - 1] == 0).all()
    assert (y[1, :, 2].argmax(-1) == T - 1).all()
    _report("softmax-special-rows", ew.case_id(T), dtype, r)


@DT_PARAMS
@EDGE_PARAMS
def test_softmax_inf_inputs(gpu, T, dtype):
    """-inf entries in x itself, one row of nothing else, no mask: torch.softmax in fp64, NaN pattern
    included."""
    x, mask = _scores(gpu, T, dtype)
    x = x.masked_fill(mask.unsqueeze(1), -float("inf"))
    x[1, 0, 1] = -float("inf")
    y, r = _softmax("-inf inputs", x, None, ew.SCALE, backward=False)
    assert torch.isnan(y[1, 0, 1]).all() and int(torch.isnan(y).sum()) == T
    _report("softmax-inf-inputs", ew.case_id(T), dtype, r)


@DT_PARAMS
@pytest.mark.parametrize("T", [2049, 65537], ids=ew.case_id)
def test_softmax_negative_scale(gpu, T, dtype):
    """scale = -0.5: the padding of the ragged tail must stay -inf, not become +inf."""
    x, mask = _scores(gpu, T, dtype)
    _report("softmax-negative-scale", ew.case_id(T), dtype, _softmax("scale -0.5", x, mask, -0.5)[1])


def test_softmax_64bit_offsets(gpu):
    """bf16, T = 131080, 16500 rows: 2.16e9 elements.  Forward and backward on the first and last row
    and the rows on both sides of element 2^30 (byte 2^31) and element 2^31 (byte 2^32)."""
    from xdot.ops.softmax import scale_mask_softmax_bwd, scale_mask_softmax_fwd

    free = torch.cuda.mem_get_info(gpu)[0]
    if free < 24 * 2 ** 30:
        pytest.skip(f"needs 24 GB of free device memory, {free / 2 ** 30:.1f} GB are free")
    T, rows = 131080, 16500
    assert rows * T > 2 ** 31
    pick = torch.tensor([0, 2 ** 30 // T, 2 ** 30 // T + 1, 2 ** 31 // T, 2 ** 31 // T + 1, rows - 1], device=gpu)
    x = torch.randn(rows, T, device=gpu, dtype=BF16).mul_(3.0)
    y = scale_mask_softmax_fwd(x, None, ew.SCALE)
    xs, ys = x[pick], y[pick]
    del x
    r = ew.assert_ratios("forward", ew.softmax_fwd_ratios(ys, xs, None, ew.SCALE))
    dy = torch.randn(rows, T, device=gpu, dtype=BF16)
    dx = scale_mask_softmax_bwd(y, dy, ew.SCALE)
    r.update(ew.assert_ratios("backward", ew.softmax_bwd_ratios(dx[pick], ys, dy[pick], ew.SCALE)))
    del y, dy, dx
    torch.cuda.empty_cache()
    _report("softmax-64bit", "stream-T131080-vec", BF16, r)


# ---- AdamW -----------------------------------------------------------------------------------------------
def _adam_setup(gpu, numels, dtype, t, seed, g32=False, capturable=False, offset=None):
    """FusedAdamW over parameters of ``numels`` with the hand-set state of step t - 1.  ``offset``: 'p',
    'grad' or 'grad_out': that tensor of every parameter starts one element into its storage."""
    from xdot.ops.optim import FusedAdamW

    states = [ew.make_adam_state(n, dtype, seed=1000 * seed + i, g32=g32) for i, n in enumerate(numels)]
    params = []
    for s in states:
        p = s.p.to(gpu)
        params.append((_offset_copy(p) if offset == "p" else p).detach().requires_grad_(True))
    opt = FusedAdamW(params, lr=ew.ADAM_LR, capturable=capturable)
    g32s = []
    for p, s in zip(params, states):
        opt.state[p] = {"step": t - 1, "exp_avg": s.m.to(gpu), "exp_avg_sq": s.v.to(gpu)}
        g = s.g.to(gpu)
        if g32:
            g32s.append(g)
            p.grad = _offset_copy(torch.zeros_like(p)) if offset == "grad_out" else None
        else:
            p.grad = _offset_copy(g) if offset == "grad" else g
    return opt, params, states, g32s


def _adam_check(what, opt, params, states, t, dtype, g32s=(), device_state=False):
    worst = {}
    for i, (p, s) in enumerate(zip(params, states)):
        st = opt.state[p]
        ref = ew.adamw_ref(s.p, s.g, s.m, s.v, t, device_state=device_state)
        _worse(worst, ew.assert_adamw(f"{what}: parameter {i} ({s.p.numel()} elements)", p.detach().cpu(),
                                      st["exp_avg"].cpu(), st["exp_avg_sq"].cpu(), ref))
        if g32s:   # the written-back gradient: the fp32 gradient rounded once
            assert p.grad.dtype == dtype and torch.equal(p.grad, g32s[i].to(dtype)), f"{what}: grad_out of parameter {i}"
    return worst


# fp32 gradient overrides (step(params=, grads=)) are for 16-bit parameters only
GRAD_KINDS = [(dt, "own") for dt in ew.DTYPES] + [(BF16, "fp32"), (FP16, "fp32")]
GRAD_PARAMS = pytest.mark.parametrize("dtype,grads", GRAD_KINDS, ids=[f"{ew.DT_IDS[d]}-{g}" for d, g in GRAD_KINDS])


@pytest.mark.parametrize("t", [1, 2, 1000])
@GRAD_PARAMS
def test_adamw_one_step(gpu, dtype, t, grads):
    """Sizes around the 1024-element block and the module's 768 x 768, one empty parameter among them;
    ``grads='fp32'``: step(params=, grads=) with fp32 gradients of 16-bit parameters."""
    numels = ew.ADAM_NUMELS[:4] + (0,) + ew.ADAM_NUMELS[4:]
    opt, params, states, g32s = _adam_setup(gpu, numels, dtype, t, seed=t, g32=grads == "fp32")
    if g32s:
        opt.step(params=params, grads=g32s)
    else:
        opt.step()
    assert all(opt.state[p]["step"] == t for p in params)
    _report(f"adamw-{grads}", f"t{t}", dtype, _adam_check("one step", opt, params, states, t, dtype, g32s))


@DT_PARAMS
def test_adamw_forty_parameters(gpu, dtype):
    """40 tensors in one group: two launches (32 + 8); the prefix search of a block's tensor crosses
    one-block and 576-block tensors."""
    numels = [ew.ADAM_NUMELS[(2 * i + 1) % 9] for i in range(40)]
    assert numels.count(768 * 768) >= 4 and 768 * 768 in numels[32:]
    opt, params, states, _ = _adam_setup(gpu, numels, dtype, 2, seed=40)
    opt.step()
    _report("adamw-40-tensors", "t2", dtype, _adam_check("40 tensors", opt, params, states, 2, dtype))


OFFSET_KINDS = [(dt, o) for dt in ew.DTYPES for o in ("p", "grad")] + [(BF16, "grad_out"), (FP16, "grad_out")]


@pytest.mark.parametrize("dtype,offset", OFFSET_KINDS, ids=[f"{ew.DT_IDS[d]}-{o}" for d, o in OFFSET_KINDS])
def test_adamw_misaligned_views(gpu, dtype, offset):
    """One operand of every parameter one element into its storage: the scalar path, full blocks too."""
    opt, params, states, g32s = _adam_setup(gpu, (4, 1025, 4098), dtype, 2, seed=7, g32=offset == "grad_out",
                                            offset=offset)
    probe = {"p": params[1], "grad": params[1].grad, "grad_out": params[1].grad}[offset]
    assert probe.data_ptr() % (4 * probe.element_size()) != 0
    if g32s:
        outs = [p.grad for p in params]
        opt.step(params=params, grads=g32s)
        assert all(p.grad is o for p, o in zip(params, outs))
    else:
        opt.step()
    _report(f"adamw-offset-{offset}", "t2", dtype, _adam_check(offset, opt, params, states, 2, dtype, g32s))


@pytest.mark.parametrize("start", [0, 1000], ids=["fresh", "resumed"])
@DT_PARAMS
def test_adamw_capturable(gpu, dtype, start):
    """capturable=True run eagerly: the step count and lr are read on the device and the bias
    corrections computed in the kernel.  Steps start + 1 .. start + 3, each against the fp64 step from
    the state before it; ``resumed``: the state of step 1000 through state_dict / load_state_dict."""
    from xdot.ops.optim import FusedAdamW

    numels = (5, 1025, 4098)
    o1, params, states, _ = _adam_setup(gpu, numels, dtype, start + 1, seed=9)
    opt = FusedAdamW(params, lr=ew.ADAM_LR, capturable=True)
    if start:
        opt.load_state_dict(o1.state_dict())
    else:
        for s in states:
            s.m.zero_()
            s.v.zero_()
    worst = {}
    for k in range(1, 4):
        gen = torch.Generator(device="cpu").manual_seed(100 * k + start)
        for p, s in zip(params, states):
            s.g = torch.randn(s.p.shape, generator=gen).to(dtype)
            p.grad = s.g.to(gpu)
        opt.step()
        _worse(worst, _adam_check(f"step {start + k}", opt, params, states, start + k, dtype, device_state=True))
        for p, s in zip(params, states):   # the next step starts from what the kernel wrote
            st = opt.state[p]
            s.p, s.m, s.v = p.detach().cpu(), st["exp_avg"].cpu(), st["exp_avg_sq"].cpu()
    for p in params:
        step = opt.state[p]["step"]
        assert step.is_cuda and step.dtype == torch.float32 and step.item() == start + 3.0
    _report("adamw-capturable", f"t{start + 1}-{start + 3}", dtype, worst)


@DT_PARAMS
def test_adamw_three_step_run(gpu, dtype):
    """Three steps from zero moments against fp64 AdamW that rounds the parameter to the dtype after
    each step.  The reference moves at least 99 % of the elements by more than the bound, so a kernel
    that writes nothing (or a fraction of the update) cannot pass."""
    from xdot.ops.optim import FusedAdamW

    worst = {}
    for numel in (768 * 768, 4098):
        p0, grads, want, bound = ew.make_adam_run(dtype, numel)
        start = p0.to(dtype)
        moved = ((want - start.double()).abs() > bound).double().mean().item()
        assert moved >= 0.99, f"the reference moves only {moved:.2%} of the elements by more than the bound"
        p = start.to(gpu).requires_grad_(True)
        opt = FusedAdamW([p], lr=ew.ADAM_LR)
        for g in grads:
            p.grad = g.to(gpu)
            opt.step()
        ratio = ((p.detach().cpu().double() - want).abs() / (bound / ew.F)).max().item()
        _worse(worst, ew.assert_ratios(f"{numel} elements", {"run": ratio}))
    _report("adamw-three-steps", "t1-3", dtype, worst)


# ---- partial sums, prescale, MSE ---------------------------------------------------------------------------
def _partials(gpu, S, n):
    g = torch.Generator(device="cpu").manual_seed(S * 100003 + n)
    # magnitudes spread over 2^+-8: the fp32 sum depends on the order of the slots
    return (torch.randn(S, n, generator=g) * torch.exp2(8 * torch.randn(S, n, generator=g))).to(gpu)


@DT_PARAMS
@pytest.mark.parametrize("n", [4, 1024, 1028, 768 * 768])
@pytest.mark.parametrize("S", [1, 2, 7])
def test_sum_partials(gpu, S, n, dtype):
    """Bitwise the fp32 sum in slot order, rounded once to the output dtype."""
    import xdot._ext as ext

    part = _partials(gpu, S, n)
    keep = part.clone()
    out = ext.ops().sum_partials(part, dtype)
    assert out.dtype == dtype and out.shape == (n,)
    assert torch.equal(out, ew.sum_partials_ref(part, dtype)) and torch.equal(part, keep)


@pytest.mark.parametrize("n", [4, 1028, 768 * 768])
@pytest.mark.parametrize("S", [1, 2, 7])
def test_sum_partials_into_first_slot(gpu, S, n):
    """``out`` aliases ``part[0]`` (the running sums of xdot/parallel/ring.py): the other slots stay."""
    import xdot._ext as ext

    part = _partials(gpu, S, n)
    keep = part.clone()
    ext.ops().sum_partials_into(part, part[0])
    assert torch.equal(part[0], ew.sum_partials_ref(keep, F32)) and torch.equal(part[1:], keep[1:])


def test_sum_partials_rejects_odd_sizes(gpu):
    import xdot._ext as ext

    part = torch.zeros(2, 6, device=gpu)
    with pytest.raises(RuntimeError):
        ext.ops().sum_partials(part, F32)
    with pytest.raises(RuntimeError):
        ext.ops().sum_partials_into(part, part[0])


@DT16_PARAMS
@pytest.mark.parametrize("scale", [96 ** -0.5, 1.0, 0.37])
def test_flash_prescale_bitwise(gpu, dtype, scale):
    """flash.prescale: x * (float32(scale) * float32(log2 e)) in fp32, rounded once.  (The profile tests
    hand its output to kernel and reference alike: a wrong constant cancels there.)"""
    from xdot.ops import flash

    g = torch.Generator(device="cpu").manual_seed(5)
    for shape in ((1, 1, 8), (2, 37, 96), (1, 1000, 768)):
        x = (torch.randn(shape, generator=g) * 4).to(gpu, dtype)
        out = flash.prescale(x, scale)
        assert out.dtype == dtype and torch.equal(out, ew.prescale_ref(x, scale)), shape


@DT_PARAMS
def test_mse_partial_vector_block(gpu, dtype):
    """(3, 1000, 8): 3000 (fp32: 6000) 16-byte vectors, not a multiple of the 256 of a workgroup."""
    import xdot._ext as ext

    g = torch.Generator(device="cpu").manual_seed(8)
    y = torch.randn(3, 1000, 8, generator=g).to(gpu, dtype)
    t = torch.randn(3, 1000, 8, generator=g).to(gpu, dtype)
    assert (y.numel() // (16 // y.element_size())) % 256
    loss, dy = ext.ops().mse_fwd(y, t)
    want, dy_ref, bound = ew.mse_ref(y, t)
    ratio = abs(loss.double().item() - want) / (bound * want)
    _report("mse", "3x1000x8", dtype, {"loss": ratio})
    assert loss.dtype == dtype and ratio <= 1.0, f"loss {loss.item()} vs {want}: {ratio:.2f} of the bound"
    assert dy.dtype == dtype and torch.equal(dy, dy_ref)
