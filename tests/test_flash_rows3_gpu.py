"""The three-workgroups-per-CU row-side flash backward kernel (csrc/flash_bwd.hip, XDOT_ROWS_WPC=3:
pre-scaled 16-bit launches with D <= 96, plain tile body, two-stage ring) against the two-per-CU
software-pipelined kernel and the torch fp32 reference of tests/test_flash_gpu.py (GPU only).

Every accumulator of the two kernels sees the same products in the same order, so for one column
split their outputs are bitwise equal.  Shapes are the smallest that reach every path of the kernel:
R = 200 (partial last 128-row block, a wave with 8 live rows, a wave past R) and R = 33; T = 64 (one
tile, nothing prefetched), 150 (three tiles, 22 tail columns) and 321 (six tiles, a 1-column tail);
column splits and partial-slot launches at T = 321.
"""
import math

import pytest
import torch

from test_flash_gpu import _close, _ref

pytestmark = pytest.mark.gpu

SHAPES = [(200, 64), (200, 150), (200, 321), (33, 64), (33, 150), (33, 321)]  # (R, T)


def _mask(R, T, g):
    """10 % random, with one 32x64 tile fully masked (rows 0-31 x columns 0-63), one fully open (the
    last 32-row block x columns 0-63) and fully masked rows (row 5; row 40 inside a partly masked
    block).  With T = 64 the masked tile makes rows 0-31 dead."""
    m = torch.rand(1, R, T, generator=g) < 0.1
    m[:, :32, :64] = True
    m[:, 32 * ((R - 1) // 32):, :64] = False
    m[:, 5] = True
    if R > 40:
        m[:, 40] = True
    return m


def _same_bits(a, b):
    """bitwise equal, NaNs compared by position"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [32, 64, 96])
@pytest.mark.parametrize("heads", [(2, 1), (4, 2)])  # (H, G)
@pytest.mark.parametrize("masked", [False, True])
def test_rows3_matches_rows2_bitwise_and_reference(gpu, monkeypatch, dt, D, heads, masked):
    from xdot import _ext
    from xdot.ops import flash

    H, G = heads
    Hg, B, C, scale = H // G, 1, H * D, 1.0 / math.sqrt(D)
    gfro = 1.5e-2 if dt == torch.bfloat16 else 4e-3  # the row-side bound of tests/test_flash_gpu.py
    g = torch.Generator(device="cpu").manual_seed(1000 * D + 10 * H + G)
    for R, T in SHAPES:
        rows = torch.randn(B, R, C, generator=g).to(gpu, dt)
        kc = torch.randn(B, T, Hg * D, generator=g).to(gpu, dt)
        vc = torch.randn(B, T, Hg * D, generator=g).to(gpu, dt)
        do = torch.randn(B, R, C, generator=g).to(gpu, dt)
        mask = _mask(R, T, g).to(gpu) if masked else None
        mk = flash.prepare_mask(mask, B, R, T)
        rk = flash.prescale(rows, scale)
        out, lse = flash.fwd(rk, kc, vc, mk, H, scale, prescaled=True, Hg=Hg)
        delta = flash.bwd_delta(do, out, H)
        live = torch.ones(R, dtype=torch.bool, device=gpu) if mask is None else ~mask[0].all(-1)
        assert bool(torch.isnan(out[0, ~live]).all()) and not bool(torch.isnan(out[0, live]).any())

        # torch fp32 reference (row head h reads gathered head h // G)
        def full(x):
            return x.view(B, T, Hg, 1, D).expand(B, T, Hg, G, D).reshape(1, B, T, C)

        k, _, _, ref_o, _ = _ref(rows, full(kc), full(vc), mask, H, scale)
        ref_o.backward(do.float())
        dk_ref = k.grad.transpose(1, 2).reshape(B, R, C)

        def rows_grad(wpc, nsplit):
            monkeypatch.setenv("XDOT_ROWS_WPC", wpc)
            with torch.cuda.device(gpu):
                plan = _ext.ops().flash_rows_plan(B, R, T, H, D, dt, 0, True, nsplit)
            assert plan[1] == int(wpc), f"XDOT_ROWS_WPC={wpc} runs {plan[1]} workgroups per CU"
            return flash.bwd_rows(do, rk, kc, vc, lse, delta, mk, H, scale, nsplit, prescaled=True, Hg=Hg)

        def rows_partial(wpc, nsplit):
            monkeypatch.setenv("XDOT_ROWS_WPC", wpc)
            dpart = torch.zeros(nsplit + 1, B, R, C, dtype=torch.float32, device=gpu)
            flash.bwd_rows_partial(do, rk, kc, vc, lse, delta, mk, H, scale, dpart, 1, nsplit, prescaled=True, Hg=Hg)
            assert not bool(dpart[0].any()), "slot 0 is not this launch's"
            return dpart

        for nsplit in ((1, 3, 4) if T == 321 else (1,)):
            what = f"R={R} T={T} nsplit={nsplit}"
            d2, d3, d3b = rows_grad("2", nsplit), rows_grad("3", nsplit), rows_grad("3", nsplit)
            assert _same_bits(d3, d2), f"{what}: 3 per CU differs from 2 per CU"
            assert _same_bits(d3, d3b), f"{what}: two runs differ"
            # fully masked rows: whatever the two-per-CU kernel gives (the comparison above) -- zeros where
            # every tile of the row is skipped, NaN for a row inside a partly masked block
            if masked and R > 40:
                assert bool(torch.isnan(d3[0, 40]).all()), f"{what}: the fully masked row 40 is NaN"
            _close(f"{what} d rows", d3[:, live], dk_ref[:, live], gfro)
        if T == 321:  # launches into partial slots (force_partial), one and three slots
            for nsplit in (1, 3):
                p2, p3, p3b = rows_partial("2", nsplit), rows_partial("3", nsplit), rows_partial("3", nsplit)
                assert _same_bits(p3, p2), f"R={R} partial slots {nsplit}: 3 per CU differs from 2 per CU"
                assert _same_bits(p3, p3b), f"R={R} partial slots {nsplit}: two runs differ"
                _close(f"R={R} partial slots {nsplit} d rows", flash.bwd_rows_sum(p3[1:].contiguous(), H, rows)[:, live],
                       dk_ref[:, live], gfro)


def test_rows3_knob_and_plan(gpu, monkeypatch):
    """XDOT_ROWS_WPC is read on every call; 3 is honoured only where the kernel exists (pre-scaled,
    D <= 96), and the plan's rounds are those of the slots of the kernel it names."""
    from xdot import _ext

    q = lambda D, prescaled: _ext.ops().flash_rows_plan(1, 25000, 25000, 8, D, torch.bfloat16, 0, prescaled, 0)  # noqa: E731
    with torch.cuda.device(gpu):
        cus = torch.cuda.get_device_properties(gpu).multi_processor_count
        monkeypatch.setenv("XDOT_ROWS_WPC", "3")
        ns, wpc, rounds = q(96, True)
        assert wpc == 3 and rounds == -(-196 * 8 * ns // (3 * cus))
        assert q(96, False)[1] == 2 and q(128, True)[1] == 2
        monkeypatch.setenv("XDOT_ROWS_WPC", "2")
        ns2, wpc, rounds = q(96, True)
        assert ns2 == ns and wpc == 2 and rounds == -(-196 * 8 * ns // (2 * cus))
        monkeypatch.delenv("XDOT_ROWS_WPC")
        assert q(96, True)[1] in (2, 3) and q(96, True)[0] == ns
