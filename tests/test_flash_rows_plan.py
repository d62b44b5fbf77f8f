"""The row-side backward's planning of its two 16-bit kernels (csrc/flash_plan.h: rows_rounds,
rows_wpc) on the host, no GPU: the three-per-CU kernel is planned over 768 resident slots, the
two-per-CU one over 512, and the functions that were there before still print the recorded table."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GXX = shutil.which("g++")

pytestmark = pytest.mark.skipif(GXX is None, reason="no g++")


def _compile(tmp, name):
    exe = str(tmp / name)
    subprocess.run([GXX, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "csrc"),
                    os.path.join(ROOT, "tests", "host", name + ".cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rows_plan")
    return _compile(tmp, "rows_plan_dump"), _compile(tmp, "flash_plan_dump")


def _run(exe, *args):
    return subprocess.run([exe, *map(str, args)], check=True, stdout=subprocess.PIPE).stdout


@pytest.mark.parametrize("R,nsplit,wgs", [(25000, 3, 196 * 8 * 3), (3125, 6, 25 * 8 * 6), (25000, 1, 196 * 8), (128, 1, 8)])
def test_rows_rounds_counts_the_kernels_own_slots(tools, R, nsplit, wgs):
    """rounds = ceil(row blocks x heads x splits / (workgroups per CU x 256 CUs)): 768 slots for the
    three-per-CU kernel, 512 for the two-per-CU one (nsplit: what rows_split gives at T = 25000)."""
    r3, r2 = (int(_run(tools[0], "rounds", 1, R, 8, nsplit, w)) for w in (3, 2))
    assert r3 == -(-wgs // 768) and r2 == -(-wgs // 512)


def test_rows_rounds_headline_values(tools):
    assert int(_run(tools[0], "rounds", 1, 25000, 8, 3, 3)) == 7    # 4704 workgroups / 768
    assert int(_run(tools[0], "rounds", 1, 25000, 8, 3, 2)) == 10   # / 512
    assert int(_run(tools[0], "rounds", 1, 3125, 8, 6, 3)) == 2     # 1200 / 768
    assert int(_run(tools[0], "rounds", 1, 3125, 8, 6, 2)) == 3


def test_rows_wpc_requests(tools):
    """A forced 2 or 3 is honoured, 3 only where three workgroups are resident; auto never picks the
    three-per-CU kernel where its larger rounds are no fewer."""
    wpc = lambda R, ns, req, occ3: int(_run(tools[0], "wpc", 1, R, 8, ns, req, occ3))  # noqa: E731
    assert wpc(25000, 3, 2, 3) == 2 and wpc(25000, 3, 3, 3) == 3
    assert wpc(25000, 3, 3, 2) == 2 and wpc(25000, 3, -1, 2) == 2
    assert wpc(25000, 3, -1, 3) in (2, 3)
    assert wpc(128, 1, -1, 3) == 2  # 8 workgroups: one round either way


def test_old_planner_table_unchanged(tools):
    with open(os.path.join(ROOT, "tests", "golden", "flash_plan.txt"), "rb") as fh:
        assert _run(tools[1]) == fh.read()
