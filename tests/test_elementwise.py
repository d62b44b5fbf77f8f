"""The bounds of tests/_elementwise.py against a torch emulation of the softmax and AdamW kernels'
algorithms (CPU only): the correct algorithm stays within the unit bounds at every (T, block) of the
softmax dispatch table, and eight wrong algorithms exceed the asserted bounds on cases of the GPU
list (tests/test_elementwise_gpu.py).  Also the mask row map of xdot/ops/softmax.py against torch
broadcasting, and the Python side of FusedAdamW on the CPU against the fp64 step."""
import pytest
import torch

import _elementwise as ew
from _elementwise import BF16, F32, FP16

DT_PARAMS = pytest.mark.parametrize("dtype", ew.DTYPES, ids=ew.DT_IDS.values())


def _fwd_bwd_ratios(T, dtype, amp, masked, hidden_lift=0.0, scale=ew.SCALE, fwd_bug=None, map_bug=None, bwd_bug=None):
    x, mask = ew.make_scores(T, dtype, amp, hidden_lift=hidden_lift)
    mask = mask if masked else None
    y = ew.emulate_softmax_fwd(x, mask, scale, fwd_bug, map_bug)
    r = ew.softmax_fwd_ratios(y, x, mask, scale)
    if fwd_bug is None and map_bug is None:
        dy = ew.make_dy(x)
        r.update(ew.softmax_bwd_ratios(ew.emulate_softmax_bwd(y, dy, scale, bwd_bug), y, dy, scale))
    return r


@DT_PARAMS
@pytest.mark.parametrize("T", ew.ALL_T, ids=ew.case_id)
def test_emulation_within_unit_bounds(T, dtype):
    """Every T of the GPU list (the edges of all seven dispatch branches), without and with the
    (B, R, T) mask, at score amplitude 3; amplitude 60 with lifted hidden entries at the largest T of
    the branch.  The unit bounds (F = 1; bf16: see EMU_LIMIT) hold for the emulation at amplitude 3,
    backward chain length K included.  At amplitude 60 the forward reaches 1.11 of the unit bound in
    fp32 (see MEASURED in tests/_elementwise.py) and is held to the asserted F."""
    worst = {}
    cases = [(3.0, False, 0.0), (3.0, True, 0.0)]
    if T == ew.BRANCH_T[ew.branch_of(T)[0]][-1]:
        cases.append((60.0, True, 1000.0))
    for amp, masked, lift in cases:
        r = _fwd_bwd_ratios(T, dtype, amp, masked, lift)
        ew.assert_ratios(f"T={T} amp={amp} masked={masked}", r, ew.EMU_LIMIT[dtype] if amp == 3.0 else ew.F)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in r.items()}
    print(f"\nRATIO emulation softmax case={ew.case_id(T)} dtype={ew.DT_IDS[dtype]} " +
          " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


@DT_PARAMS
def test_emulation_negative_scale(dtype):
    for T in (2049, 65537):
        ew.assert_ratios(f"T={T} scale=-0.5", _fwd_bwd_ratios(T, dtype, 3.0, True, scale=-0.5), ew.EMU_LIMIT[dtype])


@DT_PARAMS
def test_wrong_softmax_algorithms_exceed_the_bounds(dtype):
    """Each on a case of the GPU list (B = 2, 30 % hidden, scale 0.37)."""
    # the mask row map without the batch term: batch 1 reads the mask rows of batch 0
    r = _fwd_bwd_ratios(2048, dtype, 3.0, True, map_bug="mask_no_batch")
    assert r["fwd"] > ew.F, r
    # tail positions filled with 0: they add exp(-max) to the sum (ragged T, both kernels)
    for T in (9, 2049, 20001, 65537):
        r = _fwd_bwd_ratios(T, dtype, 3.0, False, fwd_bug="tail_zero")
        assert r["fwd"] > ew.F and r["rowsum"] > ew.F, (T, r)
    # the max taken before masking: the amplitude-60 case lifts its hidden entries 370 nats
    for T in (2048, 70000):
        r = _fwd_bwd_ratios(T, dtype, 60.0, True, hidden_lift=1000.0, fwd_bug="max_before_mask")
        assert r["fwd"] > ew.F, (T, r)
    # the stream combine without exp(mx - gmx) per thread
    for T in (65537, 70000):
        r = _fwd_bwd_ratios(T, dtype, 3.0, True, fwd_bug="stream_no_factor")
        assert r["fwd"] > ew.F and r["rowsum"] > ew.F, (T, r)
    # a backward dot that misses the last NPT chunk (every branch with more than one group)
    for T in (4096, 16384, 32768, 65536, 70000):
        r = _fwd_bwd_ratios(T, dtype, 3.0, True, bwd_bug="dot_misses_last_group")
        assert r["bwd"] > ew.F, (T, r)


def test_hidden_entries_and_dead_rows_are_exact():
    """What the ratios demand besides the bound: exact zeros where hidden, NaN on a dead row only."""
    x, mask = ew.make_scores(100, F32)
    mask[1, 2] = True
    y = ew.emulate_softmax_fwd(x, mask, ew.SCALE)
    assert torch.isnan(y[1, :, 2]).all() and torch.isnan(y).sum() == 2 * 100
    assert ew.softmax_fwd_ratios(y, x, mask, ew.SCALE)["fwd"] <= 1.0
    leak = y.clone()
    leak[0, 0, 0][mask[0, 0]] = 1e-30
    assert ew.softmax_fwd_ratios(leak, x, mask, ew.SCALE)["fwd"] == float("inf")
    alive = y.clone()
    alive[1, :, 2] = 0.01
    assert ew.softmax_fwd_ratios(alive, x, mask, ew.SCALE)["fwd"] == float("inf")
    assert ew.softmax_fwd_ratios(torch.zeros_like(y), x, None, ew.SCALE)["fwd"] > ew.F


# ---- the mask row map --------------------------------------------------------------------------------
def _mask_rows_via_map(scores, mask):
    from xdot.ops.softmax import _mask_map

    T = scores.shape[-1]
    m2, mdiv, mmul, mmod = _mask_map(scores, mask)
    rows = scores.numel() // T
    return m2.reshape(-1, T)[ew.mask_row_index(rows, mdiv, mmul, mmod)]


def test_mask_map_selects_the_broadcast_rows():
    B, H, R, T = 2, 3, 5, 11
    g = torch.Generator().manual_seed(0)
    s4 = torch.randn(B, H, R, T, generator=g)
    forms = [(s4, torch.rand(B, R, T, generator=g) < 0.5), (s4, torch.rand(B, 1, R, T, generator=g) < 0.5),
             (s4, torch.rand(B, H, R, T, generator=g) < 0.5),
             (s4[0], torch.rand(H, R, T, generator=g) < 0.5), (s4[0, 0], torch.rand(R, T, generator=g) < 0.5)]
    for scores, mask in forms:
        want = ew.broadcast_mask(scores, mask).reshape(-1, T)
        assert torch.equal(_mask_rows_via_map(scores, mask), want), tuple(mask.shape)
    # every batch / head / row is told apart: the map is not the same with the batch term dropped
    from xdot.ops.softmax import _mask_map

    m2, mdiv, mmul, mmod = _mask_map(s4, forms[0][1])
    wrong = m2.reshape(-1, T)[ew.mask_row_index(B * H * R, mdiv, mmul, mmod, "mask_no_batch")]
    assert not torch.equal(wrong, ew.broadcast_mask(s4, forms[0][1]).reshape(-1, T))


@pytest.mark.parametrize("shape", [(2, 5, 7), (3, 5, 11), (2, 2, 5, 11), (5, 11), (1, 3, 5, 11)])
def test_mask_map_rejects_unsupported_shapes(shape):
    from xdot.ops.softmax import _mask_map

    with pytest.raises(ValueError):
        _mask_map(torch.zeros(2, 3, 5, 11), torch.zeros(shape, dtype=torch.bool))


# ---- AdamW -------------------------------------------------------------------------------------------
@DT_PARAMS
@pytest.mark.parametrize("t", [1, 2, 1000])
def test_adamw_emulation_within_bounds(dtype, t):
    s = ew.make_adam_state(768 * 768, dtype, seed=t)
    ref = ew.adamw_ref(s.p, s.g, s.m, s.v, t)
    r = ew.assert_adamw(f"t={t}", *ew.emulate_adamw(s.p, s.g, s.m, s.v, t), ref)
    print(f"\nRATIO emulation adamw t={t} dtype={ew.DT_IDS[dtype]} " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))


@DT_PARAMS
def test_wrong_adamw_algorithms_exceed_the_bounds(dtype):
    """One step from the hand-set state of the GPU test (t = 2), and the three-step run."""
    s = ew.make_adam_state(4098, dtype, seed=2)
    ref = ew.adamw_ref(s.p, s.g, s.m, s.v, 2)
    for bug in ("no_write", "bc_prev_step") + (("no_wd",) if dtype == F32 else ()):
        # (weight decay moves a parameter by lr * wd = 3e-5 of itself: under one rounding of a 16-bit
        # parameter, so only the fp32 cases can see it in one step)
        r = ew.adamw_ratios(*ew.emulate_adamw(s.p, s.g, s.m, s.v, 2, bug=bug), ref)
        assert r["p"] > ew.F, (bug, r)
    assert ew.adamw_ratios(*ew.emulate_adamw(s.p, s.g, s.m, s.v, 1, bug="bc_prev_step"),
                           ew.adamw_ref(s.p, s.g, s.m, s.v, 1))["p"] == float("inf")
    p0, grads, want, bound = ew.make_adam_run(dtype)
    moved = ((want - p0.to(dtype).double()).abs() > bound).double().mean().item()
    assert moved >= 0.99, moved            # so a kernel that writes nothing misses the bound there
    assert ((want - p0.to(dtype).double()).abs()).min().item() > 5e-3
    for bug in (None,) + ew.ADAM_BUGS:
        p = p0.to(dtype)
        m, v = torch.zeros(p.shape), torch.zeros(p.shape)
        for t, g in enumerate(grads, 1):
            p, m, v = ew.emulate_adamw(p, g, m, v, t, bug=bug)
        frac = ((p.double() - want).abs() <= bound).double().mean().item()
        if bug is None:
            assert frac == 1.0, frac
        elif bug == "no_wd" and dtype != F32:
            continue                       # 3 * 3e-5 |p|: still under the roundings of a 16-bit parameter
        else:
            assert frac < 0.5, (bug, frac)


@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("t", [1, 2, 1000])
def test_fused_adamw_cpu_update_16bit(dtype, t):
    """FusedAdamW on CPU parameters (``_torch_update``): 16-bit parameters, fp32 moments, one step from
    a hand-set state against the fp64 step; 40 parameters in one group."""
    from xdot.ops.optim import FusedAdamW

    numels = [ew.ADAM_NUMELS[i % 8] for i in range(40)]
    states = [ew.make_adam_state(n, dtype, seed=100 * t + i) for i, n in enumerate(numels)]
    params = [s.p.clone().requires_grad_(True) for s in states]
    opt = FusedAdamW(params, lr=ew.ADAM_LR)
    for p, s in zip(params, states):
        p.grad = s.g.clone()
        opt.state[p] = {"step": t - 1, "exp_avg": s.m.clone(), "exp_avg_sq": s.v.clone()}
    opt.step()
    for i, (p, s) in enumerate(zip(params, states)):
        st = opt.state[p]
        assert st["step"] == t and p.dtype == dtype
        ew.assert_adamw(f"param {i} numel {numels[i]}", p.detach(), st["exp_avg"], st["exp_avg_sq"],
                        ew.adamw_ref(s.p, s.g, s.m, s.v, t, torch_path=True))


@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
def test_fused_adamw_no_op_update_is_caught(dtype, monkeypatch):
    """The three-step run with the update replaced by nothing: the parameters stay where they were
    and miss the run's bound on more than 99 % of the elements."""
    from xdot.ops.optim import FusedAdamW

    p0, grads, want, bound = ew.make_adam_run(dtype, numel=4098)
    for noop in (False, True):
        if noop:
            monkeypatch.setattr(FusedAdamW, "_torch_update", staticmethod(lambda *a, **k: None))
        p = p0.to(dtype).requires_grad_(True)
        opt = FusedAdamW([p], lr=ew.ADAM_LR)
        for g in grads:
            p.grad = g.clone()
            opt.step()
        frac = ((p.detach().double() - want).abs() <= bound).double().mean().item()
        assert (frac < 0.01) if noop else (frac == 1.0), (noop, frac)


@DT_PARAMS
def test_load_state_dict_keeps_fp32_moments(dtype):
    """torch casts loaded state tensors to the parameter's dtype; the moments of a 16-bit parameter
    must come back as the fp32 values that were saved."""
    from xdot.ops.optim import FusedAdamW

    s = ew.make_adam_state(1025, dtype, seed=3)
    p = s.p.clone().requires_grad_(True)
    a = FusedAdamW([p], lr=ew.ADAM_LR)
    a.state[p] = {"step": 1000, "exp_avg": s.m.clone(), "exp_avg_sq": s.v.clone()}
    sd = a.state_dict()
    q = s.p.clone().requires_grad_(True)
    b = FusedAdamW([q], lr=ew.ADAM_LR)
    b.load_state_dict(sd)
    st = b.state[q]
    assert st["exp_avg"].dtype == st["exp_avg_sq"].dtype == torch.float32
    assert torch.equal(st["exp_avg"], s.m) and torch.equal(st["exp_avg_sq"], s.v)
    assert int(st["step"]) == 1000


# ---- partial sums / prescale / MSE references ----------------------------------------------------------
def test_reference_helpers():
    part = torch.tensor([[1.0, 2.0 ** 24], [2.0 ** -1, 1.0], [2.0 ** -1, 1.0]])
    # slot order matters in fp32: (2^24 + 1) + 1 stays 2^24, 2^24 + (1 + 1) does not
    assert ew.sum_partials_ref(part, F32).tolist() == [2.0, 2.0 ** 24]
    assert ew.sum_partials_ref(part, BF16).dtype == BF16
    x = torch.tensor([1.0, -3.0, 0.5], dtype=BF16)
    assert torch.equal(ew.prescale_ref(x, 1.0), (x.float() * ew.LOG2E_F32).to(BF16))
    y, t = torch.tensor([1.0, 2.0, 3.0, 5.0]), torch.tensor([0.0, 2.0, 1.0, 1.0])
    loss, dy, bound = ew.mse_ref(y, t)
    assert loss == 21.0 / 4 and torch.equal(dy, (y - t) * 0.5) and bound < 2e-6
