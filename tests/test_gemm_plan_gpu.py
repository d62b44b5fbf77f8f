"""``xdot.ops.gemm.gemm_plan`` is what ``strided_gemm`` launches (GPU): one small product per route of
csrc/gemm_plan.h, planned and then run with the same arguments, against an fp64 torch product.

Operands are integers in [-3, 3], so every partial sum is an integer below 2^24: the exact-fp32 kernels
and the 16-bit kernels (fp32 accumulation, fp32 output) must be bit-exact whatever the route, the split-K
count or the slab geometry.  Split fp32 keeps the bound tests/test_gemm3_gpu.py holds path 4 to."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16

# route -> (operand dtype, a_mc, b_mc, M, N, K, nseg, batches, beta, path)
CASES = {
    "SPLIT3": (F32, False, True, 264, 296, 96, 3, 2, 0.0, 4),
    # the smallest margin over the library's 2e10 flop gate: 2 x 1280 x 1280 x 2048 x 3 = 2.013e10
    "LIBRARY": (F32, False, True, 1280, 1280, 2048, 1, 3, 1.0, 0),
    "G2_F32": (F32, True, False, 300, 260, 2048, 2, 2, 1.0, 0),   # K x nseg = 4096: the long-K rule, split-K
    "G3": (BF16, False, True, 512, 264, 2048, 1, 2, 0.0, 5),
    "G2": (F16, False, True, 512, 264, 2048, 1, 2, 1.0, 5),       # beta: the 8-phase kernel declines
    "SLABS": (F32, False, False, 300, 200, 2047, 1, 2, 1.0, 0),   # K % 4: off the 256x256 kernel; 2 batches
    "G1": (BF16, True, True, 300, 200, 97, 2, 4, 1.0, 0),
}


def _run(dev, dt, a_mc, b_mc, M, N, K, nseg=1, nb=1, beta=0.0, path=0, lda=None, ldb=None, seed=0):
    """plan, then run, one product over dense [nb][nseg] operands (rows padded to lda / ldb); fp32 output.
    -> (plan, C, fp64 reference)"""
    from xdot.ops.gemm import gemm_plan, strided_gemm

    g = torch.Generator(device="cpu").manual_seed(seed + M * 7 + N + K)
    ra, ca = (K, M) if a_mc else (M, K)
    rb, cb = (K, N) if b_mc else (N, K)
    lda, ldb = lda or ca, ldb or cb
    A = torch.randint(-3, 4, (nb, nseg, ra, lda), generator=g).to(dev, dt)
    B = torch.randint(-3, 4, (nb, nseg, rb, ldb), generator=g).to(dev, dt)
    C0 = torch.randint(-3, 4, (nb, M, N), generator=g).to(dev, F32)
    C = C0.clone()
    kw = dict(M=M, N=N, K=K, nseg=nseg, nb2=nb, lda=lda, ldb=ldb, ldc=N, sA2=nseg * ra * lda, sB2=nseg * rb * ldb,
              sC2=M * N, sAseg=ra * lda, sBseg=rb * ldb, a_mc=a_mc, b_mc=b_mc, beta=beta, path=path)
    plan = gemm_plan(A, B, C, **kw)
    strided_gemm(A, B, C, **kw)
    Ad, Bd = A[..., :ca].double(), B[..., :cb].double()
    opA = Ad.transpose(-1, -2) if a_mc else Ad    # (b, s, M, K)
    opB = Bd if b_mc else Bd.transpose(-1, -2)    # (b, s, K, N)
    return plan, C, torch.matmul(opA, opB).sum(1) + beta * C0.double()


def _check_route(dev, route):
    dt, a_mc, b_mc, M, N, K, nseg, nb, beta, path = CASES[route]
    plan, C, ref = _run(dev, dt, a_mc, b_mc, M, N, K, nseg, nb, beta, path)
    assert plan.route == route, plan
    if route in ("G2_F32", "G3", "G2"):
        assert plan.splits > 1, plan    # these shapes leave CUs idle without split-K
    if route == "SPLIT3":
        assert ((C.double() - ref).norm() / ref.norm()).item() <= 2e-5
    else:
        assert torch.equal(C.double(), ref)


@pytest.mark.parametrize("route", list(CASES))
def test_gemm_plan_query_is_what_the_launch_uses(gpu, route):
    if route != "LIBRARY":
        return _check_route(gpu, route)
    # the library route is switched by XDOT_GEMM_LIB, which the extension reads once per process
    r = subprocess.run([sys.executable, os.path.abspath(__file__), route], env=dict(os.environ, XDOT_GEMM_LIB="fp32"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout


def test_slab_route_fp32_ragged_last_slab(gpu):
    """fp32, both operands mn-contiguous, 130 x 130 x 2000 with lda = ldb = 130 (no 16-byte loads): 4 tiles
    -> 7 K slabs of 288, 6 of them full, the last 272 long."""
    plan, C, ref = _run(gpu, F32, True, True, 130, 130, 2000)
    assert (plan.route, plan.Ks, plan.slabs, plan.full) == ("SLABS", 288, 7, 6), plan
    assert not (plan.vec or plan.vec_full or plan.vec_last), plan
    assert torch.equal(C.double(), ref)


def test_slab_route_bf16_ragged_last_slab(gpu):
    """bf16 operands, fp32 output, both k-contiguous, K = 2004 (K % 8 keeps it off the 256x256 kernels):
    7 K slabs of 288, 6 of them full, the last 276 long."""
    plan, C, ref = _run(gpu, BF16, False, False, 130, 130, 2004)
    assert (plan.route, plan.Ks, plan.slabs, plan.full) == ("SLABS", 288, 7, 6), plan
    assert torch.equal(C.double(), ref)


def test_slab_route_vector_loads_full_and_last(gpu):
    """the slab route with 16-byte operand loads in the full slabs and in the last one (leading dimensions
    padded to 16 bytes, K % 4 != 0 keeps the product off the 256x256 kernel)."""
    plan, C, ref = _run(gpu, F32, False, False, 130, 130, 2002, lda=2004, ldb=2004)
    assert (plan.route, plan.Ks, plan.slabs, plan.full) == ("SLABS", 288, 7, 6), plan
    assert plan.vec and plan.vec_full and plan.vec_last, plan
    assert torch.equal(C.double(), ref)


if __name__ == "__main__":  # the child process of the LIBRARY case
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import xdot._ext as ext

    assert ext.load()
    _check_route(torch.device("cuda", 0), sys.argv[1])
