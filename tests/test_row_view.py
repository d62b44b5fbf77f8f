"""The strided-row-view rule of the rope, headnorm, sink and gate bindings (csrc/row_view.h) on the host, no
GPU: the header compiles with plain g++, and tests/host/row_view_dump.cpp answers for the views the GPU tests
of those ops launch on -- described here by real CPU tensors (shape, strides, storage size and offset; the
base address is ``BASE`` plus the view's byte offset) -- what this file states literally."""
import os
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GXX = shutil.which("g++")
BASE = 4096  # of every storage: on the 16-byte grid
BF16 = torch.bfloat16

pytestmark = pytest.mark.skipif(GXX is None, reason="no g++")


def _line(t, written=False, stride=None, avail=None):
    """the case line of the view ``t``; ``stride`` / ``avail`` forge what no tensor can have"""
    es = t.element_size()
    B, R, C = t.shape
    s0, s1, s2 = stride or t.stride()
    if avail is None:
        avail = t.untyped_storage().nbytes() // es - t.storage_offset()
    return f"{B} {R} {C} {s0} {s1} {s2} {avail} {es} {BASE + t.storage_offset() * es} {int(written)}"


def _views():
    z = lambda *shape, dtype=BF16: torch.zeros(*shape, dtype=dtype)  # noqa: E731
    out = z(1, 4, 128)
    big = z(1, 9, 128)
    dense = z(2, 5, 128)
    return [
        # name, case line, expected: "ok sb sr vec lo hi" (strides in elements, span in bytes) or the error
        ("contiguous", _line(dense), "ok 640 128 1 4096 6656"),
        ("q half of a packed [q | v]", _line(z(2, 5, 256)[..., :128]), "ok 1280 256 1 4096 8960"),
        ("q half of slot 1 of a (3, B, R, 2C) gather buffer", _line(z(3, 2, 5, 256)[1][..., :128]), "ok 1280 256 1 9216 14080"),
        ("v half of that slot", _line(z(3, 2, 5, 256)[1][..., 128:]), "ok 1280 256 1 9472 14336"),
        ("padded batch", _line(z(2, 8, 128)[:, :5]), "ok 1024 128 1 4096 7424"),
        ("padded batch, written", _line(z(2, 8, 128)[:, :5], written=True), "ok 1024 128 1 4096 7424"),
        ("base one element off the grid", _line(z(1281)[1:].view(2, 5, 128)), "ok 640 128 0 4098 6658"),
        ("fp32, base four elements in: on the grid", _line(z(1, 4, 132, dtype=torch.float32)[..., 4:]), "ok 0 132 1 4112 6208"),
        ("bf16, the same view: base and row stride off it", _line(z(1, 4, 132)[..., 4:]), "ok 0 132 0 4104 5152"),
        ("40-byte row stride (bf16, C = 20)", _line(z(1, 4, 20)), "ok 0 20 0 4096 4256"),
        ("C = 20 inside a 40-wide buffer: 80-byte rows", _line(z(1, 4, 40)[..., :20]), "ok 0 40 1 4096 4376"),
        ("B = 1: its stride is not looked at", _line(out.as_strided((1, 4, 128), (7, 128, 1))), "ok 0 128 1 4096 5120"),
        ("B = 1, forged negative batch stride", _line(out, stride=(-5, 128, 1)), "ok 0 128 1 4096 5120"),
        ("R = 1: its stride is not looked at", _line(z(2, 128).as_strided((2, 1, 128), (128, 3, 1))), "ok 128 0 1 4096 4608"),
        ("C = 1: its stride is not looked at", _line(z(2, 5, 2)[..., ::2]), "ok 10 2 0 4096 4134"),
        ("every second element", _line(z(1, 4, 256)[..., ::2]), "inner_stride"),
        ("one row expanded to four, read", _line(out[:, :1].expand(1, 4, 128)), "ok 0 0 1 4096 4352"),
        ("one row expanded to four, written", _line(out[:, :1].expand(1, 4, 128), written=True), "rows_overlap"),
        ("batches that overlap, read", _line(z(8, 128).as_strided((2, 4, 128), (256, 128, 1))), "ok 256 128 1 4096 5632"),
        ("batches that overlap, written", _line(z(8, 128).as_strided((2, 4, 128), (256, 128, 1)), written=True), "rows_overlap"),
        ("rows that overlap by one element, written", _line(z(520).as_strided((1, 4, 128), (0, 127, 1)), written=True), "rows_overlap"),
        ("forged negative row stride", _line(dense, stride=(640, -128, 1)), "negative_stride"),
        ("forged negative batch stride", _line(dense, stride=(-640, 128, 1)), "negative_stride"),
        ("exactly to the end of the storage", _line(dense, avail=1280), "ok 640 128 1 4096 6656"),
        ("one element past its storage", _line(dense, avail=1279), "out_of_bounds"),
        ("forged strides whose extent passes int64", _line(dense, stride=(2**62, 2**62, 1), avail=2**63 - 1), "out_of_bounds"),
        ("empty B", _line(z(0, 5, 128)), "ok 0 0 1 4096 4096"),
        ("empty R, strides not looked at", _line(z(2, 0, 128), stride=(-1, -1, 2), written=True), "ok 0 0 1 4096 4096"),
        # the operands of tests/test_gate_gpu.py's shared-memory cases
        ("big[:, 0:4]", _line(big[:, 0:4]), "ok 0 128 1 4096 5120"),
        ("big[:, 2:6]", _line(big[:, 2:6]), "ok 0 128 1 4608 5632"),
        ("big[:, 0:8:2]", _line(big[:, 0:8:2]), "ok 0 256 1 4096 5888"),
        ("big[:, 4:8]", _line(big[:, 4:8]), "ok 0 128 1 5120 6144"),
    ]


PAIRS = [  # (a, b, disjoint, same_view)
    ("big[:, 0:4]", "big[:, 2:6]", 0, 0),     # dout over part of dy
    ("big[:, 0:8:2]", "big[:, 0:8:2]", 0, 1),  # dy itself, strided: in place
    ("big[:, 0:8:2]", "big[:, 0:4]", 0, 0),    # dy's base with other strides
    ("big[:, 0:4]", "big[:, 4:8]", 1, 0),      # end to end: apart
    ("big[:, 4:8]", "big[:, 0:4]", 1, 0),
    ("big[:, 0:4]", "big[:, 0:4]", 0, 1),
]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("row_view") / "row_view_dump")
    subprocess.run([GXX, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "csrc"),
                    os.path.join(ROOT, "tests", "host", "row_view_dump.cpp"), "-o", exe], check=True)
    views = _views()
    index = {name: i for i, (name, _l, _e) in enumerate(views)}
    lines = [l for _n, l, _e in views] + [f"pair {index[a]} {index[b]}" for a, b, _d, _s in PAIRS]
    got = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, stdout=subprocess.PIPE, text=True).stdout
    got = got.splitlines()
    assert len(got) == len(lines)
    return views, got


def test_views(answers):
    views, got = answers
    wrong = [(name, line, want, have) for (name, line, want), have in zip(views, got) if want != have]
    assert not wrong


def test_disjoint_and_same_view(answers):
    views, got = answers
    wrong = [(p, have) for p, have in zip(PAIRS, got[len(views):]) if have != f"pair {p[2]} {p[3]}"]
    assert not wrong
