"""Which decode calls the chunked-prefill kernel (csrc/flash_extend.hip) takes, and that a CPU call with that
many rows still runs the torch reference."""
import pytest
import torch

from xdot.ops import flash

bf16, f16, f32, f8 = torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn


@pytest.mark.parametrize("args,want", [
    ((bf16, 96, 96, 4, 17), True), ((f16, 32, 32, 5, 13), True), ((bf16, 128, 128, 1, 65), True),
    ((bf16, 64, 64, 1, 4096, bf16), True), ((bf16, 64, 64, 128, 1), True),
    ((bf16, 96, 96, 4, 16), False),            # G * Rn = 64: the decode kernel's
    ((f32, 64, 64, 4, 17), False), ((bf16, 160, 160, 4, 17), False), ((bf16, 64, 32, 4, 17), False),
    ((bf16, 96, 96, 4, 17, f8), False), ((bf16, 96, 96, 4, 17, f16), False),
    ((bf16, 64, 64, 129, 1), False),           # a group wider than the smallest row block
    ((f16, 96, 96, 1, 128), True), ((f16, 96, 96, 1, 129), False),   # routed away by profiles/extend.md
])
def test_extend_eligible(args, want):
    assert flash.extend_eligible(*args) is want
    if want:
        assert not flash.decode_eligible(*args)


def test_cpu_call_above_64_rows_runs_the_torch_reference():
    from xdot.parallel import _ref

    g = torch.Generator().manual_seed(0)
    B, Tcap, H, Hg, D, Rn = 1, 50, 4, 2, 32, 40
    rows, qc, vc = (torch.randn(B, L, h * D, generator=g).bfloat16() for L, h in ((Rn, H), (Tcap, Hg), (Tcap, Hg)))
    pos = torch.arange(Tcap, dtype=torch.int32).repeat(B, 1)
    assert flash.extend_eligible(bf16, D, D, H // Hg, Rn)
    out, lse = flash.decode(rows, qc, vc, pos, 10, H, 0.2, window=7, Hg=Hg)
    ro, rl = _ref.decode(rows, qc, vc, pos, 10, H, 0.2, 7, Hg)
    assert out.dtype == bf16 and torch.equal(out, ro.to(bf16)) and torch.equal(lse, rl)
    with pytest.raises(ValueError, match="flash.extend"):
        flash.extend(rows, qc, vc, pos, 10, H, 0.2, Hg=Hg)
