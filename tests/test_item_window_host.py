"""The item window of the pointwise kernels (paos_amd/csrc/item_window.h) on the CPU: tests/item_window_main.cpp is compiled
with the address and undefined-behaviour sanitizers and run as a child process.  ``all`` holds every rows x columns window
of the layouts that exist (4 x 2 and 8 x 2 blocks, the pitch padded by three blocks) at n = 16 and 64 to one rule: the start
writes (dense walk) what the power sum reads (filtered walk, whatever the grid) and what the zeroing spares (outside)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD_BLOCKS, BC = 3, 2


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("item_window") / "item_window_main")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "item_window_main.cpp"), "-o", exe], check=True)
    return exe


def test_every_window_of_every_layout(program):
    out = subprocess.run([program, "all"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")
    # per axis B = n (n + 1) / 2 windows and null: each row window with null columns, each column window with one row
    # window, every sixteenth column window with null rows
    count = lambda n: 2 * (n * (n + 1) // 2 + 1) + -(-(n * (n + 1) // 2 + 1) // 16)  # noqa: E731
    want = [f"{n} {br} windows {count(n)}" for n in (16, 64) for br in (4, 8)]
    assert lines[:4] == want and lines[4] == "ok"


# ---- the rule, restated: the slots of the pixels of the box, rounded outward to blocks ---------------------------------
def slot(n, br, r, c):
    pitch = n * br + PAD_BLOCKS * br * BC
    return (r // br) * pitch + (c // BC) * (br * BC) + (r % br) * BC + c % BC


def box(n, br, rows, cols):
    rlo, rhi = (0, n) if rows is None else (rows[0] // br * br, -(-rows[1] // br) * br)
    clo, chi = (0, n) if cols is None else (cols[0] // BC * BC, -(-cols[1] // BC) * BC)
    return [(r, c) for r in range(rlo, min(rhi, n)) for c in range(clo, min(chi, n))], (rlo, min(rhi, n))


WALKS = [  # n, block rows, rows, cols, workgroups
    (16, 4, (5, 7), (3, 6), 3),
    (16, 4, None, None, 1),
    (16, 8, (8, 9), None, 3),
    (16, 8, None, (0, 1), 1024),
    (64, 4, (63, 64), (62, 64), 3),
    (64, 8, (1, 63), (1, 63), 1024),
    (64, 4, (0, 1), (0, 64), 1),
]


@pytest.mark.parametrize("n,br,rows,cols,grid", WALKS)
def test_walks_against_the_rule(program, n, br, rows, cols, grid):
    args = [n, br, *(rows or (-1, -1)), *(cols or (-1, -1)), grid]
    out = subprocess.run([program, "walk", *map(str, args)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = {line.split()[0]: line.split()[1:] for line in out.stdout.splitlines()}
    pixels, (rlo, rhi) = box(n, br, rows, cols)
    slots = sorted(slot(n, br, r, c) for r, c in pixels)
    assert [int(m) for m in got["filtered"]] == slots
    assert got["inside"] == [f"{r},{c}" for r, c in pixels]
    pitch = n * br + PAD_BLOCKS * br * BC
    if cols is None:  # whole block rows, in memory order, padding included
        assert [int(m) for m in got["dense"]] == list(range(rlo // br * pitch, rhi // br * pitch))
    else:
        assert [int(m) for m in got["dense"]] == slots


def test_a_known_window(program):
    """The answer itself: rows [5, 7) of 4-row blocks are rows 4..7, columns [3, 6) of 2-column blocks are 2..5 -- block row
    1 (pitch 88), blocks 1 and 2 of 8 slots each."""
    out = subprocess.run([program, "walk", "16", "4", "5", "7", "3", "6", "1"], capture_output=True, text=True, timeout=60)
    assert out.stdout.splitlines()[0].split() == ["filtered"] + [str(m) for m in range(88 + 8, 88 + 24)]
