"""The GEMM route planner (csrc/gemm_plan.h) on the host, no GPU: the header compiles with plain g++
and reproduces tests/golden/gemm_plan.txt, the table recorded from the dispatch code of ``xdot.gemm``
as it stood before it moved into the header (tests/host/gemm_plan_dump.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GXX = shutil.which("g++")

pytestmark = pytest.mark.skipif(GXX is None, reason="no g++")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_dump")
    subprocess.run([GXX, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "csrc"),
                    os.path.join(ROOT, "tests", "host", "gemm_plan_dump.cpp"), "-o", exe], check=True)
    return subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout


def test_planner_matches_golden_table(table):
    with open(os.path.join(ROOT, "tests", "golden", "gemm_plan.txt"), "rb") as fh:
        assert table == fh.read()


def _case(M, N, K, dt_in, dt_out, a_mc, b_mc, nseg=1, nb1=1, nb2=1, path=0, ncu=256, lib=0, g3=1, free="6.4e+10",
          beta0=1, lda=None, ldb=None, ldc=None, **strides):
    """the dump's line key: operands dense [nb1][nb2][nseg][rows][cols] (``dense`` in the dump program) unless
    strides are given by keyword"""
    dense = dict(sA1=nb2 * nseg * M * K, sA2=nseg * M * K, sB1=nb2 * nseg * N * K, sB2=nseg * N * K, sC1=nb2 * M * N,
                 sC2=M * N, sAseg=M * K, sBseg=N * K)
    st = dict(dense, **strides)
    return (f"gemm {M} {N} {K} {nseg} {nb1} {nb2} {lda or (M if a_mc else K)} {ldb or (N if b_mc else K)} {ldc or N} "
            + ("dense" if st == dense else " ".join(str(v) for v in st.values()))
            + f" {'km'[a_mc]}{'km'[b_mc]} b{1 - beta0} {dt_in} {dt_out} 111 p{path} | {ncu} {lib} {g3} {free}")


def test_planner_spot_values(table):
    """result fields: route, split-K slices, vec of a plain launch; SLABS: slab length, slabs, full slabs,
    vec of the full / the last slab, vec of a plain launch; LIBRARY: merged K and the three batch strides"""
    got = dict(line.split(" -> ") for line in table.decode().splitlines())
    T, d, D, R8 = 25000, 768, 96, 3125
    heads = dict(nb2=8, lda=d, ldb=d, sA1=0, sA2=D, sB1=0, sB2=D, sAseg=0, sBseg=0)  # head-split views of (R, 768)
    # the workload's bf16 nt product on one rank: (8 heads) 25000 x 25000 x 96 -> the 8-phase kernel, no split
    nt1 = dict(heads, ldc=T, sC1=T, sC2=T * T)
    assert got[_case(T, T, D, "bf16", "bf16", 0, 0, **nt1)] == "G3 1 1"
    # the same product in fp32: the exact 256x256 kernel; with the split route allowed (path 6): split fp32
    assert got[_case(T, T, D, "f32", "f32", 0, 0, **nt1)] == "G2_F32 1 1"
    assert got[_case(T, T, D, "f32", "f32", 0, 0, path=6, **nt1)] == "SPLIT3 1 1"
    # nt on a rank of 8 as one GEMM over all T columns
    nt8 = dict(heads, ldc=T, sC1=0, sC2=R8 * T)
    assert got[_case(R8, T, D, "bf16", "bf16", 0, 0, **nt8)] == "G3 1 1"
    # the `all` product on a rank of 8: K = 3125 rows per rank segment, odd segment stride -> no 16-byte
    # loads, off the 256x256 kernels: 4 K slabs of 784 (3 full) on the 128x128 kernel
    all8 = dict(nseg=8, nb2=8, lda=T, ldb=d, ldc=d, sA1=0, sA2=R8 * T, sB1=0, sB2=D, sC1=0, sC2=D, sAseg=R8,
                sBseg=R8 * d)
    assert got[_case(R8, D, R8, "bf16", "bf16", 0, 1, **all8)] == "SLABS 784 4 3 0 0 0"
    # tn on a rank of 8 as one GEMM over all T rows (N = 96: the 8-phase kernel declines, the 256x256 one splits K in 2)
    tn8 = dict(nb2=8, lda=T, ldb=d, ldc=d, sA1=0, sA2=R8 * T, sB1=0, sB2=D, sC1=0, sC2=D, sAseg=0, sBseg=0)
    assert got[_case(T, D, R8, "bf16", "bf16", 1, 1, **tn8)] == "G2 2 1"
    # fp32 weight gradient 768 x 768 x 25000, both operands mn-contiguous: the exact 256x256 kernel, split-K
    assert got[_case(d, d, T, "f32", "f32", 1, 1)] == "G2_F32 27 1"
    # fp32 projection 25000 x 768 x 768: few tiles, short K -> the 128x128 kernel
    assert got[_case(T, d, d, "f32", "f32", 0, 0)] == "G1 1 1"
    # bf16 weight gradient at 3125 rows (path 5): 12 slices on 256 CUs, 7 on 64 -- the CU count is a parameter
    assert got[_case(d, d, R8, "bf16", "f32", 1, 1, path=5)] == "G3 12 1"
    assert got[_case(d, d, R8, "bf16", "f32", 1, 1, path=5, ncu=64)] == "G3 7 1"
    # the slab cases tests/test_gemm_plan_gpu.py runs: 7 slabs of 288, 6 full (the last is 272 / 276 long), no vec
    assert got[_case(130, 130, 2000, "f32", "f32", 1, 1)] == "SLABS 288 7 6 0 0 0"
    assert got[_case(130, 130, 2004, "bf16", "f32", 0, 0)] == "SLABS 288 7 6 0 0 0"
    # fp32 -> fp16: no kernel writes it directly (error 6), but the slab route's ordered sum does
    assert got[_case(256, 256, 64, "f32", "f16", 0, 0)] == "error 6 0"
    assert got[_case(130, 130, 2000, "f32", "f16", 1, 1)] == "SLABS 288 7 6 0 0 0"
    # XDOT_GEMM_LIB=1: a 16-bit product on the library from 2e10 flop
    assert got[_case(8192, 8192, 144, "bf16", "bf16", 0, 0, lib=2)] == "G3 1 1"
    assert got[_case(8192, 8192, 152, "bf16", "bf16", 0, 0, lib=2)] == "LIBRARY 152 1245184 1245184 67108864"
    # split fp32 with 1.0003e9 bytes of operand copies: only with four times that free
    assert got[_case(4096, 4096, 20352, "f32", "f32", 0, 0, path=6, free="4e+09")] == "G2_F32 1 1"
    assert got[_case(4096, 4096, 20352, "f32", "f32", 0, 0, path=6, free="4.1e+09")] == "SPLIT3 1 1"
    # 9 tiles x 65535 batches: past the 8-phase kernel's 2048 items per workgroup on 256 CUs, within on 304
    assert got[_case(768, 768, 64, "bf16", "bf16", 0, 0, nb2=65535)] == "G2 1 1"
    assert got[_case(768, 768, 64, "bf16", "bf16", 0, 0, nb2=65535, ncu=304)] == "G3 1 1"
    # forced paths that raise: 4 with beta != 0 (1), fp32 path 2 with M % 4 != 0 (2), 3 on fp32 (3), 3 with M < 256 (4)
    assert got[_case(256, 256, 64, "f32", "f32", 0, 0, path=4, beta0=0)] == "error 1 0"
    assert got[_case(514, 514, 2048, "f32", "f32", 1, 1, path=2, lda=520, ldb=520)] == "error 2 0"
    assert got[_case(130, 130, 2000, "f32", "f32", 1, 1, path=3)] == "error 3 0"
    assert got[_case(130, 130, 2000, "bf16", "bf16", 0, 0, path=3)] == "error 4 -3"
    # thresholds on M: 64 for the 16-bit 256x256 kernels (512 batches: past the tile gate), 128 for the fp32 one
    # (K = 4096: past the long-K gate; below it K slabs), 256 for the 8-phase kernel (path 5)
    assert got[_case(63, 300, 64, "bf16", "bf16", 0, 0, nb2=512)] == "G1 1 1"
    assert got[_case(64, 300, 64, "bf16", "bf16", 0, 0, nb2=512)] == "G2 1 1"
    assert got[_case(127, 300, 4096, "f32", "f32", 0, 0)] == "SLABS 256 16 16 1 0 1"
    assert got[_case(128, 300, 4096, "f32", "f32", 0, 0)] == "G2_F32 31 1"
    assert got[_case(255, 300, 64, "bf16", "bf16", 0, 0, path=5)] == "G2 1 1"
    assert got[_case(256, 300, 64, "bf16", "bf16", 0, 0, path=5)] == "G3 1 1"
    # the pickers on their own: 9 tiles over 49 k-tiles on 256 CUs; the 768 x 768 weight gradient over 25000 rows
    assert got["pick_splits 9 49 256"] == "12"
    assert got["wgrad_slabs 25000 768 768 0"] == "12"
