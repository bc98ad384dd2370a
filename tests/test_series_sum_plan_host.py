"""The size rule and the launch ranges of a broadband series sum (paos_amd/csrc/series_sum_plan.h) on the CPU:
tests/series_sum_plan_main.cpp is compiled with the address and undefined-behaviour sanitizers and run as a child process
(a signed or 32-bit overflow in the size arithmetic ends it)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_CHUNK_FRAMES = 32768  # kSeriesMaxChunkFrames: the frames of a launch are a grid dimension
MAX_DOUBLES = 1 << 27  # kSeriesSumMaxDoubles, PAOS_SERIES_SUM_MAX_DOUBLES


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("series_sum_plan") / "series_sum_plan_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "series_sum_plan_main.cpp"), "-o", exe], check=True)
    return exe


def ask(program, lines):
    out = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    return out.stdout.splitlines()


def test_the_public_header_names_the_same_limit():
    with open(os.path.join(ROOT, "include", "paos_hip.h")) as fh:
        assert "PAOS_SERIES_SUM_MAX_DOUBLES = 1 << 27" in fh.read()
    from paos_amd import _lib

    assert _lib.SERIES_SUM_MAX_DOUBLES == MAX_DOUBLES


def test_frame_ranges_cover_the_series_once_in_order(program):
    counts = [1, 2, 5, 32767, 32768, 32769, 65535, 65536]
    lines = ask(program, [f"ranges {t}" for t in counts])
    for frames, line in zip(counts, lines):
        ranges = [tuple(int(v) for v in part.split()) for part in line.partition(":")[2].split(";") if part.strip()]
        at = 0
        for t0, nt in ranges:
            assert t0 == at and 1 <= nt <= MAX_CHUNK_FRAMES, line
            at += nt
        assert at == frames and len(ranges) == -(-frames // MAX_CHUNK_FRAMES), line
    assert lines[-1].split(":")[1].split(";")[:2] == [" 0 32768 ", " 32768 32768 "]
    assert ask(program, ["ranges 0"]) == ["ranges :"]


def test_the_size_rule_at_its_edge_and_without_overflow(program):
    cases = [(1, 1, 1, 1), (5, 37, 29, 1), (256, 64, 64, 1), (65536, 2, 2, 1), (8, 4096, 4096, 1),  # 2^27 exactly
             (32768, 64, 64, 1), (65536, 32, 64, 1),  # 2^27 exactly
             (32769, 64, 64, 0), (65536, 64, 64, 0), (9, 4096, 4096, 0), (8, 4096, 4095, 1),
             (65536, 4096, 4096, 0),  # 2^40: no overflow, refused
             (0, 9, 7, 0), (-1, 9, 7, 0), (65537, 1, 1, 0), (1, 0, 7, 0), (1, 9, 4097, 0), (1, -3, 7, 0)]
    lines = ask(program, [f"size {t} {nx} {ny}" for t, nx, ny, _ in cases])
    for (frames, nx, ny, ok), line in zip(cases, lines):
        _, got, doubles = line.split()
        assert int(got) == ok, (frames, nx, ny, line)
        if ok:
            assert int(doubles) == frames * nx * ny <= MAX_DOUBLES
        elif frames >= 1 and nx >= 1 and ny >= 1 and frames <= 65536 and nx <= 4096 and ny <= 4096:
            assert frames * nx * ny > MAX_DOUBLES
    # the rule on the count itself (2^27 + 1 = 3^4 x 19 x 87211 is no frames x ny x nx within the limits of each)
    lines = ask(program, [f"fits {v}" for v in (0, 1, MAX_DOUBLES - 1, MAX_DOUBLES, MAX_DOUBLES + 1, 1 << 40, (1 << 64) - 1)])
    assert [int(line.split()[1]) for line in lines] == [0, 1, 1, 1, 0, 0, 0]


def test_tiles_of_a_frame(program):
    lines = ask(program, ["tiles 1 256", "tiles 256 256", "tiles 257 256", "tiles 1073 256", f"tiles {4096 * 4096} 256"])
    assert [int(line.split()[1]) for line in lines] == [1, 1, 2, 5, 65536]
