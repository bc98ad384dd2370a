"""The block renderer of ellipse line records on the CPU (paos_amd/csrc/record_blocks.h; the kernel: pointwise.h,
mask_blocks_kernel): tests/record_blocks_main.cpp is compiled with the address and undefined-behaviour sanitizers and run as
a child process.

Classification: the renderer calls a window pixel `in` (the record holds 1.0), `out` (0.0) or undecided (the exact overlap
is evaluated).  Whatever it decides must be what oracle.aperture_np.ellipse_mask computes for that pixel, exactly -- over
random ellipses at n = 64 and 256: round, flat and tiny ones, centres on integers, on half-integers and anywhere, boxes
that cross the grid's edges, both axes.  And it must decide: on a round ellipse with a >= 32, of the pixels with mask exactly
0 or 1 that touch a partially covered pixel (its 3 x 3 neighbourhood) at most half may be left to the exact overlap --
window pixels called undecided and every pixel of a line that fits no window (pixels outside a fitting line's windows are
decided by window_fit's span tests).  Over the inputs below (such ellipses occur at n = 256 only) the largest fraction is
0.099, all of it lines at the tips that fit no window: a window pixel with mask 1.0 has its four corners inside and one with
0.0 stays outside by more than the margin, but for accidents of 1e-9.

List layout: where the undecided pixels of a block's lines go in the wave's list -- exclusive prefix sums, nothing behind
the capacity, and which lines are handed over."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle.aperture_np import ellipse_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 1024


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("record_blocks") / "record_blocks_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "record_blocks_main.cpp"), "-o", exe], check=True)
    return exe


def _run(program, text):
    out = subprocess.run([program], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.splitlines()


def _centre(rng, kind, n):
    c = rng.uniform(0.3 * n, 0.7 * n, 2)
    if kind == 0:
        return np.round(c)
    if kind == 1:
        return np.round(c) + 0.5
    return c


def _ellipses(n, count, seed):
    """(family, xc, yc, a, b): round, flat (either way), tiny, and round ones whose box crosses one or two grid edges."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        family = ("round", "flat", "tiny", "edge")[i % 4]
        xc, yc = _centre(rng, (i // 4) % 3, n)
        if family == "round":
            a = b = rng.uniform(32.0, 0.29 * n) if n >= 128 and i % 8 else rng.uniform(8.0, 0.29 * n)
        elif family == "flat":
            a, b = rng.uniform(0.15 * n, 0.29 * n), rng.uniform(2.0, 0.04 * n + 2.0)
            if i % 8 >= 4:
                a, b = b, a
        elif family == "tiny":
            a, b = rng.uniform(2.0, 6.0, 2)
        else:
            a = b = rng.uniform(0.1 * n, 0.4 * n)
            xc = rng.choice([rng.uniform(-0.05 * n, 0.1 * n), rng.uniform(0.9 * n, 1.05 * n)])
            if i % 8 >= 4:
                yc = rng.choice([rng.uniform(-0.05 * n, 0.1 * n), rng.uniform(0.9 * n, 1.05 * n)])
        out.append((family, float(xc), float(yc), float(a), float(b)))
    return out


def _classes(program, n, ellipses):
    """Per (ellipse, axis): the program's lines [(line, W, wl0, wr0, classes)]."""
    text = "".join(f"ellipse {n} {axis} {xc.hex()} {yc.hex()} {a.hex()} {b.hex()}\n" for _, xc, yc, a, b in ellipses for axis in (0, 1))
    runs, cur = [], []
    for row in _run(program, text):
        if row == "end":
            runs.append(cur)
            cur = []
        else:
            w = row.split()
            assert w[0] == "L", row
            cur.append((int(w[1]), int(w[2]), int(w[3]), int(w[4]), w[5]))
    assert len(runs) == 2 * len(ellipses)
    return runs


@pytest.mark.parametrize("n,count", [(64, 2400), (256, 1200)])
def test_decided_pixels_are_exact_and_the_boundary_is_mostly_decided(program, n, count):
    ellipses = _ellipses(n, count, seed=n)
    runs = _classes(program, n, ellipses)
    decided = undecided = fitted = handed = 0
    worst = 0.0
    for e, (family, xc, yc, a, b) in enumerate(ellipses):
        mask = ellipse_mask((n, n), xc, yc, a, b)
        if mask is None:
            assert not runs[2 * e] and not runs[2 * e + 1]
            continue
        partial = (mask > 0.0) & (mask < 1.0)
        near = np.zeros_like(partial)
        p = np.pad(partial, 1)
        for dy in range(3):
            for dx in range(3):
                near |= p[dy:dy + n, dx:dx + n]
        rim = near & ~partial  # exact 0 or 1 next to a partially covered pixel
        for axis in (0, 1):
            m = mask if axis == 0 else mask.T
            left = np.zeros((n, n), dtype=bool)  # [line, pos]: left to the exact overlap
            for line, W, wl0, wr0, classes in runs[2 * e + axis]:
                if W == 0:
                    handed += 1
                    left[line, :] = True
                    continue
                fitted += 1
                assert len(classes) == 2 * W and 0 <= wl0 and wl0 + W <= wr0 and wr0 + W <= n, (family, xc, yc, a, b, axis, line, W, wl0, wr0)
                pos = np.concatenate([np.arange(wl0, wl0 + W), np.arange(wr0, wr0 + W)])
                cls = np.frombuffer(classes.encode(), dtype=np.uint8)
                vals = m[line, pos]
                bad = ((cls == ord("i")) & (vals != 1.0)) | ((cls == ord("o")) & (vals != 0.0))
                assert not bad.any(), f"{family} ellipse {(xc, yc, a, b)} axis {axis} line {line}: position {pos[bad][0]} called {chr(cls[bad][0])}, mask {vals[bad][0]!r}"
                left[line, pos[cls == ord("u")]] = True
                decided += int((cls != ord("u")).sum())
                undecided += int((cls == ord("u")).sum())
            if family == "round" and a >= 32.0:
                r = rim if axis == 0 else rim.T
                frac = float((left & r).sum()) / float(r.sum())
                worst = max(worst, frac)
                assert frac <= 0.5, f"round ellipse {(xc, yc, a, b)} axis {axis}: {frac:.3f} of the exact pixels at the boundary were left undecided"
    print(f"n = {n}: {fitted} lines fit windows, {handed} are handed over; window pixels decided {decided}, undecided {undecided}; "
          f"largest undecided fraction of the exact boundary pixels of a round ellipse: {worst:.4f}")
    assert fitted > handed > 0 and decided > undecided > 0  # (the inputs exercise the classes and the hand-over)


def _layout(program, counts):
    rows = _run(program, "layout " + " ".join(str(c) for c in counts) + "\n")
    got = {r.split()[0]: r.split()[1:] for r in rows}
    assert got["guard"] == ["ok"] and got["capacity"] == [str(CAP)], rows
    return [int(v) for v in got["offsets"]], [int(v) for v in got["kept"]], int(got["total"][0]), int(got["used"][0])


LAYOUTS = {
    "empty lines and full ones": [0, 64, 0, 3, 64, 0, 0, 12, 1, 0],
    "exactly the capacity": [16] * 64,
    "one over, in the last line": [16] * 63 + [17],
    "one over, early": [64] * 15 + [63, 2] + [0, 5, 0],
    "the maximum everywhere": [64] * 64,
    "nothing": [0] * 64,
    "a short block": [7, 0, 9],
    "zeros behind a full list": [64] * 16 + [0, 0, 1, 0],
}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_list_layout(program, name):
    counts = LAYOUTS[name]
    offsets, kept, total, used = _layout(program, counts)
    want = [int(v) for v in np.concatenate([[0], np.cumsum(counts)[:-1]])]
    assert offsets == want                                         # exclusive prefix sums, handed-over lines included
    assert kept == [int(o + c <= CAP) for o, c in zip(want, counts)]  # the rule: a line whose entries would end behind the capacity
    ends = [o + c for o, c, k in zip(want, counts, kept) if k]
    assert total == max(ends) and used == max([o + c for o, c, k in zip(want, counts, kept) if k and c] + [0])
    assert used <= total <= CAP


def test_the_cases_reach_the_capacity_from_both_sides(program):
    assert sum(LAYOUTS["exactly the capacity"]) == CAP and sum(LAYOUTS["one over, in the last line"]) == CAP + 1
    _, kept, total, _ = _layout(program, LAYOUTS["exactly the capacity"])
    assert all(kept) and total == CAP
    _, kept, total, _ = _layout(program, LAYOUTS["one over, in the last line"])
    assert kept == [1] * 63 + [0] and total == CAP - 16
    _, kept, _, _ = _layout(program, LAYOUTS["zeros behind a full list"])
    assert kept == [1] * 16 + [1, 1, 0, 0]  # a line without entries behind an overflow is handed over with it
