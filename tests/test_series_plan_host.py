"""The chunk plan of a pointing series (paos_amd/csrc/series_plan.h) against its rule, on the CPU:
tests/series_plan_main.cpp is compiled with the address and undefined-behaviour sanitizers and run as a child process."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_CHUNK_FRAMES = 32768  # kSeriesMaxChunkFrames: the frames of a chunk are a grid dimension


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("series_plan") / "series_plan_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "series_plan_main.cpp"), "-o", exe], check=True)
    return exe


def ask(program, lines):
    out = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    return out.stdout.splitlines()


def parse(line):
    head, _, tail = line.partition(":")
    items, frames, nbytes = (int(v) for v in head.split()[1:])
    chunks = [tuple(int(v) for v in part.split()) for part in tail.split(";") if part.strip()]
    return items, frames, nbytes, chunks


CASES = [(3, 7, 37 * 29, k * 3 * 37 * 29 * 8) for k in (1, 2, 3, 7, 100)]  # chunks of 1, 2, 3 frames; all; more than all
CASES += [(3, 7, 37 * 29, 3 * 3 * 37 * 29 * 8 + 8), (3, 7, 37 * 29, 3 * 37 * 29 * 8 - 1)]  # a little more / less than whole frames
CASES += [(3, 7, 37 * 29, 37 * 29 * 8), (3, 7, 37 * 29, 2 * 37 * 29 * 8), (3, 7, 37 * 29, 1), (5, 2, 10, 3 * 80)]  # not every item fits
CASES += [(1, 1, 1, 8), (1, 65536, 1, 1 << 29), (32, 256, 4096, 512 << 20), (32, 1024, 4096, 512 << 20), (2, 3, 4096 * 4096, 512 << 20),
          (32, 3, 4096 * 4096, 512 << 20), (512, 65536, 64, 512 << 20)]


def test_every_plan_covers_the_series_once_in_frame_order(program):
    lines = ask(program, [f"plan {b} {t} {npix} {cap}" for b, t, npix, cap in CASES])
    assert len(lines) == len(CASES)
    for (batch, frames, npix, cap), line in zip(CASES, lines):
        items, per, nbytes, chunks = parse(line)
        one = npix * 8
        # the rule: whole frames of every item while they fit (at least one, at most a grid dimension's worth); else one
        # frame of as many items as fit (at least one)
        if batch * one <= cap:
            assert (items, per) == (batch, min(cap // (batch * one), frames, MAX_CHUNK_FRAMES)), line
        else:
            assert (items, per) == (max(cap // one, 1), 1), line
        assert 1 <= items <= batch and 1 <= per <= frames and nbytes == items * per * one
        assert nbytes <= cap or (per == 1 and (items == 1 or items == batch)), line
        # the chunks: every (frame, item) once, frames ascending, items ascending within a frame range
        seen = []
        for t0, nt, i0, ni in chunks:
            assert 1 <= nt <= per and 1 <= ni <= items and t0 + nt <= frames and i0 + ni <= batch, line
            seen.append((t0, i0))
            if len(seen) < 3000:  # (the long plans are checked by their sums below)
                assert seen == sorted(seen)
        assert sum(nt * ni for _, nt, _, ni in chunks) == frames * batch, line
        assert len(set(seen)) == len(seen) and seen == sorted(seen)
        starts = sorted({t0 for t0, _, _, _ in chunks})
        assert starts == list(range(0, frames, per))
        for t0 in starts[:50]:
            group = [(i0, ni) for s, _, i0, ni in chunks if s == t0]
            assert [i0 for i0, _ in group] == list(range(0, batch, items)) and sum(ni for _, ni in group) == batch


def test_the_split_the_gpu_test_asks_for(program):
    one = 3 * 37 * 29 * 8
    got = [parse(line)[3] for line in ask(program, [f"plan 3 7 {37 * 29} {k * one}" for k in (1, 2, 3)])]
    assert [[nt for _, nt, _, _ in chunks] for chunks in got] == [[1] * 7, [2, 2, 2, 1], [3, 3, 1]]
    items = parse(ask(program, [f"plan 3 7 {37 * 29} {2 * 37 * 29 * 8}"])[0])[3]
    assert items[:2] == [(0, 1, 0, 2), (0, 1, 2, 1)] and len(items) == 14


def test_the_environment_switch(program):
    lines = ask(program, ["cap 512", "cap 512 4096", "cap 512 1", "cap 512 0", "cap 512 -5", "cap 512 12x", "cap 512 x", "cap 512 1e6",
                          "cap 512 18446744073709551615"])
    assert [int(line.split()[1]) for line in lines] == [512, 4096, 1, 512, 512, 512, 512, 512, 18446744073709551615]
