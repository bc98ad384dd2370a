"""Which launches take the narrow-window variant of their central-half build (paos_amd/csrc/pass_program.h: pick_narrow;
frugal_pass.h: CH = 2) -- on the CPU: tests/narrow_windows_main.cpp builds the launch records by hand, is compiled with the
address and undefined-behaviour sanitizers and run as a child process.  The rule: the build is a central-half one, the
context's switch is on, every active item of the launch's first pass loads positions of [5 n / 16, 11 n / 16) only and every
active item of its last pass stores positions of that window only.  The kernel has no guard of its own, so an answer of 1
for a window that reaches one position further would lose that position."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096
LO, HI = 5 * N // 16, 11 * N // 16   # 1280, 2816


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("narrow_windows") / "narrow_windows_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "narrow_windows_main.cpp"), "-o", exe], check=True)
    return exe


def ask(program, items, central=1, switch=1, count=2, n=N):
    """items: (active, pos_lo, pos_hi, spos_lo, spos_hi) each -> 0 / 1."""
    text = f"launch {n} {len(items)} {central} {switch} {count}\n" + "".join(" ".join(str(v) for v in it) + "\n" for it in items)
    out = subprocess.run([program], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    words = out.stdout.split()
    assert len(words) == 2 and words[0] == "narrow", out.stdout
    return int(words[1])


INSIDE = (1, LO, HI, LO, HI)


@pytest.mark.parametrize("count", [1, 2, 3])
def test_windows_exactly_on_the_edges_are_narrow(program, count):
    assert ask(program, [INSIDE, INSIDE], count=count) == 1
    assert ask(program, [(1, 1532, 2564, 1532, 2564), (1, LO, LO + 1, HI - 1, HI)], count=count) == 1


@pytest.mark.parametrize("count", [1, 2, 3])
@pytest.mark.parametrize("item", [(1, LO - 1, HI, LO, HI), (1, LO, HI + 1, LO, HI), (1, LO, HI, LO - 1, HI), (1, LO, HI, LO, HI + 1)],
                         ids=["load-lo", "load-hi", "store-lo", "store-hi"])
def test_one_position_beyond_either_edge_of_either_window_is_not(program, item, count):
    assert ask(program, [item], count=count) == 0
    assert ask(program, [INSIDE, item, INSIDE], count=count) == 0  # one item of the batch outside: the whole launch


def test_stores_of_whole_lines_are_not(program):
    assert ask(program, [(1, 1532, 2564, 0, N)]) == 0


def test_only_central_half_builds_have_the_variant(program):
    assert ask(program, [INSIDE], central=0) == 0


def test_the_switch_turns_it_off(program):
    assert ask(program, [INSIDE], switch=0) == 0


def test_an_inactive_item_outside_the_windows_does_not_matter(program):
    assert ask(program, [INSIDE, (0, 0, N, 0, N)]) == 1
    assert ask(program, [(0, 0, N, 0, N), (0, 0, N, 0, N)]) == 0  # ... but a launch without an active item is nobody's business


def test_other_grid_sizes_scale_the_window(program):
    assert ask(program, [(1, 640, 1408, 640, 1408)], n=2048) == 1
    assert ask(program, [(1, 639, 1408, 640, 1408)], n=2048) == 0
