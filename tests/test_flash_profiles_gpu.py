"""16-bit flash kernels on score profiles that move the running max (GPU only).

``randn`` operands never take the deferred rescale of csrc/flash_fwd.hip (``rescale_to``) and of
csrc/flash_wide.hip (``scale_pinned``) with a finite running max and nonzero accumulators, never
let the wave-wide trigger fire for some rows only, never put a masked or padded column above the live
ones, and never hand the combine / merge kernels partial LSEs that are far apart.  The profiles of
tests/_flash_profiles.py do; tests/test_flash_profiles.py shows on the CPU that a correct algorithm
stays within the bounds asserted here and that three wrong ones do not.

Every case checks its profile first (``check_profile``), compares the forward with the fp64 reference
and the backward with the operation ``flash.bwd`` is documented to compute from the ``out`` / ``lse`` it
is handed (``backward_spec``), and prints its ratios to the bounds (``-s`` shows them)."""
import pytest
import torch

import _flash_profiles as fp

pytestmark = pytest.mark.gpu

BF16, FP16 = torch.bfloat16, torch.float16
DT_IDS = {BF16: "bf16", FP16: "fp16"}

# (B, R, T, H, D)
NARROW_SHAPES = [(1, 128, 300, 2, 64), (1, 200, 600, 2, 96), (2, 77, 300, 3, 32), (1, 130, 330, 2, 128)]
NARROW_KINDS = ("ramp", "late_spike", "late_spike_tail", "plateau", "deep_negative", "masked_peak", "masked_peak_lead")
NARROW_CASES = [(kind, shape) for shape in NARROW_SHAPES for kind in NARROW_KINDS] + [("creep", NARROW_SHAPES[1])]

WIDE_KINDS = ("ramp", "late_spike", "late_spike_tail", "deep_negative", "masked_peak")
WIDE_CASES = [(kind, (1, 96, 200, 1, D), BF16) for D in (160, 192, 256, 384) for kind in WIDE_KINDS] + \
             [(kind, (1, 96, 200, 1, 256), FP16) for kind in WIDE_KINDS] + \
             [(kind, (1, 160, 330, 2, 160), BF16) for kind in WIDE_KINDS]

SPLIT_SHAPE = (1, 150, 1000, 2, 96)
HEAVY_SHAPE = (1, 65 * 128, 2048, 8, 64)   # tests/test_flash_gpu.py::test_flash_head_heavy_grid


def _report(family, c, **ratios):
    print(f"\nRATIO family={family} kind={c.kind} shape={c.shape} dtype={DT_IDS[c.dtype]} " +
          " ".join(f"{k}={v:.3f}" for d in ratios.values() for k, v in d.items()))


def _reference(c, rk, prescaled):
    ref_out, ref_lse, s2 = fp.reference(rk, c.kc, c.vc, c.mask, c.H, c.scale, prescaled, c.Hg)
    fp.check_profile(s2, c.tile, c.kind, c.mask)
    return ref_out, ref_lse


def _fwd_bwd(family, gpu, kind, shape, dtype, prescaled, Hg=None):
    from xdot.ops import flash

    c = fp.make_case(kind, shape, dtype, gpu, Hg)
    B, R, T, H, D = shape
    rk = flash.prescale(c.rows, c.scale) if prescaled else c.rows
    ref_out, ref_lse = _reference(c, rk, prescaled)
    mk = flash.prepare_mask(c.mask, B, R, T)
    out, lse = flash.fwd(rk, c.kc, c.vc, mk, H, c.scale, prescaled=prescaled, Hg=Hg)
    f = fp.assert_forward(kind, out, lse, ref_out, ref_lse, dtype)
    d_rows, d_kc, d_vc = flash.bwd(c.dout, rk, c.kc, c.vc, out, lse, mk, H, c.scale, prescaled=prescaled, Hg=Hg)
    assert d_rows.dtype == dtype and d_kc.dtype == d_vc.dtype == torch.float32
    spec = fp.backward_spec(c.dout, rk, c.kc, c.vc, out, lse, c.mask, H, c.scale, prescaled, Hg)
    b = fp.assert_backward(kind, d_rows, d_kc, d_vc, spec, dtype)
    _report(family, c, fwd=f, bwd=b)


@pytest.mark.parametrize("dtype", [BF16, FP16], ids=DT_IDS.values())
@pytest.mark.parametrize("prescaled", [False, True], ids=["plain", "prescaled"])
@pytest.mark.parametrize("kind,shape", NARROW_CASES)
def test_narrow_fwd_bwd(gpu, kind, shape, dtype, prescaled):
    """csrc/flash_fwd.hip + csrc/flash_bwd.hip / flash_cols.hip, D <= 128."""
    _fwd_bwd("narrow", gpu, kind, shape, dtype, prescaled)


@pytest.mark.parametrize("kind,shape,dtype", WIDE_CASES)
def test_wide_fwd_bwd(gpu, kind, shape, dtype):
    """csrc/flash_wide.hip, 16-bit policy (column tile 32, AGPR-pinned accumulators)."""
    _fwd_bwd("wide", gpu, kind, shape, dtype, False)


@pytest.mark.parametrize("prescaled", [False, True], ids=["plain", "prescaled"])
def test_grouped_heads(gpu, prescaled):
    """H = 4 row heads on Hg = 1 gathered head: the narrow operand carries the profile."""
    _fwd_bwd("grouped", gpu, "ramp", (1, 128, 300, 4, 64), BF16, prescaled, Hg=1)


# ---- column splits and partial slots ---------------------------------------------------------------
def _split_case(gpu, kind, masked=False):
    """ramp / late_spike (150 log2 units: > 100 nats) at the split shape; the column segments of the
    partial-slot tests cut where the profile steps, so their LSEs are > 100 nats apart on the b = +-8 rows.
    ``masked``: the first segment is hidden from rows 0-39 only."""
    c = fp.make_case(kind, SPLIT_SHAPE, BF16, gpu, spike_log2=150.0)
    T, tile = SPLIT_SHAPE[2], c.tile
    cut = tile if kind == "ramp" else (T // tile - 2) * tile       # after tile 0 / before the spike tile
    if masked:
        c.mask = torch.zeros(SPLIT_SHAPE[0], SPLIT_SHAPE[1], T, dtype=torch.bool, device=gpu)
        c.mask[:, :40, :cut] = True
    ref_out, ref_lse = _reference(c, c.rows, False)
    return c, [(0, cut), (cut, T)], ref_out, ref_lse


_SPLIT_REF = {}


def _split_ref(gpu, kind):
    """The case, its reference and the nsplit = 1 run, computed once per kind and left unchanged."""
    from xdot.ops import flash

    if kind not in _SPLIT_REF:
        c, segs, ref_out, ref_lse = _split_case(gpu, kind)
        o1, l1 = flash.fwd(c.rows, c.kc, c.vc, None, c.H, c.scale, nsplit=1)
        _report("split1", c, fwd=fp.assert_forward(kind, o1, l1, ref_out, ref_lse, BF16))
        _SPLIT_REF[kind] = (c, segs, ref_out, ref_lse, o1, l1)
    return _SPLIT_REF[kind]


def _vs_unsplit(o, l, o1, l1):
    """today's split tolerances (tests/test_flash_gpu.py::test_flash_column_split)"""
    assert (o1.float() - o.float()).abs().max().item() < 2e-2
    assert (l1 - l).abs().max().item() < 1e-3


def _spread(lpart):
    """largest difference between two slots' (finite) LSEs of one row, in nats"""
    hi = lpart.amax(0)
    lo = torch.where(torch.isfinite(lpart), lpart, hi.unsqueeze(0).expand_as(lpart)).amin(0)
    return (hi - lo).max().item()


@pytest.mark.parametrize("nsplit", [2, 5])
@pytest.mark.parametrize("kind", ["ramp", "late_spike"])
def test_column_split(gpu, kind, nsplit):
    """``flash.fwd`` with column splits, and the same through ``fwd_partial`` + ``fwd_combine``."""
    from xdot.ops import flash

    c, _, ref_out, ref_lse, o1, l1 = _split_ref(gpu, kind)
    B, R, T, H, D = c.shape
    o2, l2 = flash.fwd(c.rows, c.kc, c.vc, None, H, c.scale, nsplit=nsplit)
    f2 = fp.assert_forward(f"{kind} nsplit {nsplit}", o2, l2, ref_out, ref_lse, BF16)
    _vs_unsplit(o2, l2, o1, l1)
    opart = torch.full((nsplit, B, R, H * D), float("nan"), dtype=torch.float32, device=gpu)
    lpart = torch.full((nsplit, B, H, R), float("nan"), dtype=torch.float32, device=gpu)
    flash.fwd_partial(c.rows, c.kc, c.vc, None, H, c.scale, opart, lpart, 0, nsplit)
    o3, l3 = flash.fwd_combine(opart, lpart, H, c.rows)
    f3 = fp.assert_forward(f"{kind} partial + combine {nsplit}", o3, l3, ref_out, ref_lse, BF16)
    _vs_unsplit(o3, l3, o1, l1)
    assert _spread(lpart) > 50.0          # the slots' LSEs really are far apart
    _report("split", c, fwd=f2, combine=f3)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "slot_masked_for_some_rows"])
@pytest.mark.parametrize("dominant", ["first", "last"])
@pytest.mark.parametrize("kind", ["ramp", "late_spike"])
def test_partial_merge_far_apart(gpu, kind, dominant, masked):
    """``fwd_partial`` over two column segments whose LSEs differ by > 100 nats, merged by ``fwd_merge``
    (in place, fp32) and by ``fwd_combine``, with the dominant segment (for the b = 8 rows) in the
    first slots or in the last; ``masked``: the first segment is hidden from rows 0-39 only (its LSE
    is -inf there and its output NaN)."""
    from xdot.ops import flash

    if masked:
        c, segs, ref_out, ref_lse = _split_case(gpu, kind, masked=True)
        o1, l1 = flash.fwd(c.rows, c.kc, c.vc, flash.prepare_mask(c.mask, *c.mask.shape), c.H, c.scale, nsplit=1)
    else:
        c, segs, ref_out, ref_lse, o1, l1 = _split_ref(gpu, kind)
    B, R, T, H, D = c.shape
    order = segs[::-1] if dominant == "first" else segs      # (the b = 8 rows peak in the second segment)
    ns = [1 if b - a <= c.tile else 2 for a, b in order]
    opart = torch.full((sum(ns), B, R, H * D), float("nan"), dtype=torch.float32, device=gpu)
    lpart = torch.full((sum(ns), B, H, R), float("nan"), dtype=torch.float32, device=gpu)
    for i, (a, b) in enumerate(order):
        mk = flash.prepare_mask(c.mask[..., a:b].contiguous(), B, R, b - a) if c.mask is not None else None
        flash.fwd_partial(c.rows, c.kc[:, a:b], c.vc[:, a:b], mk, H, c.scale, opart, lpart, sum(ns[:i]), ns[i])
    assert _spread(lpart) > 100.0, f"slot LSEs only {_spread(lpart):.1f} nats apart"
    if masked:
        i = order.index(segs[0])
        dead = lpart[sum(ns[:i]):sum(ns[:i + 1])]
        assert (dead[..., :40] == -float("inf")).all() and torch.isfinite(dead[..., 40:]).all()
    o2, l2 = flash.fwd_combine(opart, lpart, H, c.rows)
    f2 = fp.assert_forward(f"{kind} combine", o2, l2, ref_out, ref_lse, BF16)
    _vs_unsplit(o2, l2, o1, l1)
    lrun = torch.empty(B, H, R, dtype=torch.float32, device=gpu)
    flash.fwd_merge(opart, lpart, lrun, H)                   # every slot into slot 0, its LSE into lrun
    lpart[0].copy_(lrun)
    o3, l3 = flash.fwd_combine(opart[:1], lpart[:1], H, c.rows)
    f3 = fp.assert_forward(f"{kind} merge", o3, l3, ref_out, ref_lse, BF16)
    _vs_unsplit(o3, l3, o1, l1)
    _report("merge", c, combine=f2, merge=f3)


def test_head_heavy_grid(gpu):
    """``ramp`` on the shape that reaches the head-heavy grid and ``flash_fwd_combine_tail`` (the
    automatic launch of tests/test_flash_gpu.py::test_flash_head_heavy_grid)."""
    from xdot import _ext
    from xdot.ops import flash

    c = fp.make_case("ramp", HEAVY_SHAPE, BF16, gpu)
    B, R, T, H, D = c.shape
    with torch.cuda.device(gpu):
        _, heavy, _, _ = _ext.ops().flash_fwd_plan(B, R, T, H, D, BF16, 0, False, 0)
    assert heavy, "this shape no longer takes the head-heavy grid"
    ref_out, ref_lse = _reference(c, c.rows, False)
    out, lse = flash.fwd(c.rows, c.kc, c.vc, None, H, c.scale)            # head-heavy (auto)
    f = fp.assert_forward("head-heavy", out, lse, ref_out, ref_lse, BF16)
    o1, l1 = flash.fwd(c.rows, c.kc, c.vc, None, H, c.scale, nsplit=1)    # uniform, whole blocks
    f1 = fp.assert_forward("uniform", o1, l1, ref_out, ref_lse, BF16)
    assert torch.equal(out[:, : 64 * 128], o1[:, : 64 * 128])            # whole blocks: the same kernel path
    _vs_unsplit(out, lse, o1, l1)
    _report("heavy", c, heavy=f, uniform=f1)


@pytest.mark.parametrize("nsplit", [1, 3])
def test_split_row_side_backward(gpu, nsplit):
    """``bwd_rows`` alone, unsplit and with 3 column splits, on ``ramp``: the d_rows part of the bounds."""
    from xdot.ops import flash

    c, _, ref_out, ref_lse, o1, l1 = _split_ref(gpu, "ramp")
    H = c.H
    delta = flash.bwd_delta(c.dout, o1, H)
    d = flash.bwd_rows(c.dout, c.rows, c.kc, c.vc, l1, delta, None, H, c.scale, nsplit=nsplit)
    spec = fp.backward_spec(c.dout, c.rows, c.kc, c.vc, o1, l1, None, H, c.scale, False)
    _report("rows_split", c, bwd=fp.assert_backward(f"bwd_rows nsplit {nsplit}", d, None, None, spec, BF16))
