"""The flash kernels' grid planner (csrc/flash_plan.h) on the host, no GPU: the header compiles
with plain g++ and reproduces tests/golden/flash_plan.txt, the table recorded from the planner
functions as they stood before they moved into the header (tests/host/flash_plan_dump.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GXX = shutil.which("g++")

pytestmark = pytest.mark.skipif(GXX is None, reason="no g++")


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("flash_plan") / "flash_plan_dump")
    subprocess.run([GXX, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "csrc"),
                    os.path.join(ROOT, "tests", "host", "flash_plan_dump.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def table(dump):
    return subprocess.run([dump], check=True, stdout=subprocess.PIPE).stdout


def test_planner_matches_golden_table(table):
    with open(os.path.join(ROOT, "tests", "golden", "flash_plan.txt"), "rb") as fh:
        assert table == fh.read()


def test_planner_spot_values(table):
    got = dict(line.split(" -> ") for line in table.decode().splitlines())
    assert got["pick_split 1568 25000 512 0"] == "3"
    # head-heavy forward, (W, tiles of 64 columns, slots per XCD, uniform split to beat): the 16-bit
    # N=1 forward (T = 25000 -> 391 tiles, uniform split 3) and the N=8 rank's 200 blocks
    assert got["heavy_fwd 1568 391 64 3"] == "192 4 11"
    assert got["heavy_fwd 200 391 64 5"] == "no"
    assert got["rows_split 1 25000 25000 8"] == "3"
    assert got["rows_split 1 3125 25000 8"] == "6"
    assert got["pick_csplit 200 782 768 32 0.001"] == "19"
    assert got["pick_csplit 776 32 768 32 0.001"] == "2"
    # the exact-fp32 forward at 776 blocks, T = 1024 (16 tiles): 3 workgroups per CU against the
    # occupancy split 2 takes the grid, 2 per CU against split 1 does not
    assert got["heavy_fwd 776 16 96 2"] == "96 1 2"
    assert got["heavy_fwd 776 16 64 1"] == "no"


@pytest.mark.parametrize("value,want", [(None, (-1, -1, -1)), ("", (-1, -1, -1)), ("auto", (-1, -1, -1)),
                                        ("0", (1, 1, 0)), ("3", (3, 3, 3)), ("99", (8, 4, 99))])
def test_env_int(dump, value, want):
    """unset / empty / auto -> -1, else atoi clamped: XDOT_CSPLIT to 1..8 (flash_f32.hip) and 1..4
    (flash_x3.hip, flash_cols.hip), XDOT_WIDE_SPLIT from 0 with no upper bound."""
    env = {k: v for k, v in os.environ.items() if k != "XDOT_TEST_KNOB"}
    if value is not None:
        env["XDOT_TEST_KNOB"] = value
    got = tuple(int(subprocess.run([dump, "env", "XDOT_TEST_KNOB", lo, hi], check=True, env=env,
                                   stdout=subprocess.PIPE).stdout)
                for lo, hi in (("1", "8"), ("1", "4"), ("0", str(2**31 - 1))))
    assert got == want
