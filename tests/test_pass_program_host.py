"""The planner of the pass programs (paos_amd/csrc/pass_program.h on the records of pass_records.h) on the CPU:
tests/pass_program_main.cpp is compiled with the address and undefined-behaviour sanitizers, without FMA contraction, and run
as a child process -- one per family for the recipes of tests/pass_builds.py, so the file stays in seconds.

1. every recipe of pass_builds.py: launch ``rc.index`` of the planner's output is exactly the record (what
   test_gpu_pass_builds.py asserts from DeviceFields.pass_builds() on the device);
2. the invariants the planner states (plan_pruning's comment) on seeded random programs;
3. the smallest shapes at which each rule around it can go wrong;
4. the program exits 0 under both sanitizers for all of it (``ask`` asserts the exit status of every child)."""
import os
import random
import shutil
import struct
import subprocess

import numpy as np
import pytest

import pass_builds as pb
from paos_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("axis", "kpre", "kmid", "nfft", "store", "tab", "fuse", "one_line", "central")
ELLIPSE, RECT = _lib.SHAPE_ELLIPSE, 1 - _lib.SHAPE_ELLIPSE


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("pass_program") / "pass_program_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "pass_program_main.cpp"), "-o", exe], check=True)
    return exe


def wire(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def block_rows(precision, n):
    return 8 if precision == "fp32" and n >= 2048 else 4  # csrc/host.h: block_rows<T, N>()


def text(n, batch, br, precision, passes, blocks, central=1, switches=(1,) * 8, final=0, psfmem=None, rows=None, stale=False, cols=None):
    """One program in the words of pass_program_main.cpp; passes and blocks as DeviceFields.run_passes takes them."""
    blocks = np.asarray(blocks, dtype=np.float64)
    assert blocks.shape[1:] == (batch, 5)
    out = ["program", f"dims {n} {batch} {br} {0 if precision == 'fp64' else 1} {central}", "switches " + " ".join(str(int(s)) for s in switches),
           f"final {int(final)}"]
    out.append("psfmem -1" if psfmem is None else f"psfmem {psfmem[0]} " + " ".join(wire(v) for lohi in psfmem[1] for v in lohi))
    out.append(f"entry {int(rows is not None)} {int(stale)} {int(cols is not None)}")
    for win in (rows, cols):
        if win is not None:
            out.append(" ".join(wire(v) for v in np.asarray(win, dtype=np.float64).reshape(-1)))
    out.append(f"blocks {blocks.shape[0]}")
    out.append(" ".join(wire(v) for v in blocks.reshape(-1)))
    out.append(f"passes {len(passes)}")
    for p in passes:
        lists = [p.get(s, ()) for s in ("pre", "mid", "post")]
        out.append(" ".join(str(v) for v in [p["axis"], p.get("fft1", -1), p.get("fft2", -1)] + [len(l) for l in lists] + [v for l in lists for op in l for v in op]))
    return "\n".join(out) + "\n"


def ask(program, texts):
    out = subprocess.run([program], input="".join(texts), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    plans = []
    for line in out.stdout.splitlines():
        w = line.split()
        if w[0] == "program":
            plans.append({"passes": [], "launches": [], "batched": []})
        elif w[0] == "phases":
            plans[-1]["phases"] = int(w[1])
        elif w[0] == "flags":
            plans[-1].update({k: int(v) for k, v in zip(w[1::2], w[2::2])})
        elif w[0] == "batched":
            plans[-1]["batched"] = [int(v) for v in w[1:]]
        elif w[0] == "pass":
            d = {k: int(v) for k, v in zip(w[2:20:2], w[3:20:2])}
            d.update(window=(int(w[21]), int(w[22])), items=[])
            plans[-1]["passes"].append(d)
        elif w[0] == "item":
            plans[-1]["passes"][int(w[1])]["items"].append(
                {"active": int(w[4]), "lines": (int(w[6]), int(w[7])), "fill": int(w[9]), "loads": (int(w[11]), int(w[12])), "stores": (int(w[14]), int(w[15]))})
        elif w[0] == "launch":
            plans[-1]["launches"].append({"pass": int(w[3]), "count": int(w[5]), "tables": int(w[7]), "build": tuple(int(v) for v in w[9:18]),
                                          "grid": (int(w[19]), int(w[20])), "tag": int(w[22]), "bytes": float(w[24]), "lines": float(w[26])})
        elif w[0] == "psfmem":
            plans[-1]["psfmem"] = [int(v) for v in w[1:]]
    assert len(plans) == len(texts)
    return plans


# ---- 1. the recipes -----------------------------------------------------------------------------------------------------
def recipe_text(precision, n, rc):
    """What DeviceFields.run_passes and paos_run_program hand to run_passes for the recipe's keywords."""
    kw, batch = rc.kw, rc.fields["batch"]
    stale = bool(kw.get("rows_stale")) and kw.get("live_rows") is not None
    return text(n, batch, block_rows(precision, n), precision, rc.passes, rc.blocks, central=1, final=int(kw.get("final_intensity", 0)),
                rows=kw.get("live_rows"), stale=stale, cols=kw.get("live_cols") if stale else None)


RECIPES_SEEN = {}


@pytest.mark.parametrize("precision,n", pb.FAMILIES)
def test_every_recipe_plans_its_record(program, precision, n):
    cases = [(r, pb.recipe(precision, n, r)) for r in pb.built_records(precision, n) if (precision, n, r) not in pb.UNREACHABLE]
    assert all(rc is not None for _, rc in cases), "zero recipes may be skipped"
    plans = ask(program, [recipe_text(precision, n, rc) for _, rc in cases])
    for (r, rc), plan in zip(cases, plans):
        assert plan["phases"] == 0 and plan["all_frugal"] == 1, (precision, n, r)
        want_launches = 1 if rc.fields["axes"] == 1 else 2
        assert len(plan["launches"]) == want_launches, f"{want_launches} launch(es) expected, the plan holds {plan['launches']}"
        got = plan["launches"][rc.index]["build"]
        assert got == tuple(r), f"launch {rc.index} takes the build {dict(zip(FIELDS, got))}, the recipe is for {dict(zip(FIELDS, r))}"
    RECIPES_SEEN[(precision, n)] = len(cases)
    assert len(cases) == pb.BUILT[(precision, n)] - sum(1 for key in pb.UNREACHABLE if key[:2] == (precision, n))


def test_all_748_recipes_were_planned():
    assert sum(RECIPES_SEEN.get(f, 0) for f in pb.FAMILIES) == 748, RECIPES_SEEN


# ---- 2. the planner's invariants on random programs ---------------------------------------------------------------------
class Blocks:
    def __init__(self, batch):
        self.batch, self.rows = batch, []

    def add(self, per_item):
        assert len(per_item) == self.batch
        self.rows.append([list(map(float, q)) for q in per_item])
        return len(self.rows) - 1


def random_program(rng, n, out_item):
    """1-6 row / column passes of three items, item ``out_item`` sitting out (every block disabled); apertures in either slot: an
    ellipse, a rectangle, an obscuration, one off the grid."""
    b = Blocks(3)
    on = [0.0 if it == out_item else 1.0 for it in range(3)]
    passes = []
    for _ in range(rng.randint(1, 6)):
        axis = rng.randint(0, 1)
        p = {"axis": axis, "fft1": b.add([[on[it] * (rng.random() < 0.85), rng.randint(0, 1), 0, 0, 0] for it in range(3)]), "pre": [], "mid": []}
        if rng.random() < 0.5:
            p["fft2"] = b.add([[on[it] * (rng.random() < 0.8), rng.randint(0, 1), 0, 0, 0] for it in range(3)])
        along_only = rng.random() < 0.6
        for slot, top in (("pre", 2), ("mid", 3)):
            for _ in range(rng.randint(0, top)):
                rows = []
                for it in range(3):
                    s_along, s_across = 0.5 + rng.random(), 0.0 if along_only else rng.random()
                    sx, sy = (s_along, s_across) if axis == 0 else (s_across, s_along)
                    rows.append([on[it], sx, sy, 1e-3 * rng.random(), rng.choice((-1.0, 1.0))])
                p[slot].append((rng.choice((_lib.PW_QPHASE_CENTRED, _lib.PW_QPHASE_NATURAL)), rng.choice((0, _lib.PWF_MUL2PI)), b.add(rows)))
            if rng.random() < 0.3:
                p[slot].append((_lib.PW_SIGN, rng.choice((0, _lib.PWF_X_ONLY, _lib.PWF_Y_ONLY)), b.add([[on[it], 0, 0, 0, 0] for it in range(3)])))
            if rng.random() < 0.3:
                p[slot].append((_lib.PW_SCALE, 0, b.add([[on[it], 0, 0, 0.5, 0] for it in range(3)])))
        if rng.random() < 0.6:
            kind = rng.choice(("ellipse", "rect", "obscuration", "off"))
            first, second = [], []
            for it in range(3):
                ext = [n * (0.08 + 0.12 * rng.random()) for _ in range(2)]
                centre = [n * (0.3 + 0.4 * rng.random()) for _ in range(2)]
                if kind == "off":
                    centre[rng.randint(0, 1)] = -3.0 * n
                first.append([on[it], centre[0], centre[1], ext[0], ext[1]])
                second.append([0.0, 1.0 if kind == "obscuration" else 0.0, 32.0, RECT if kind == "rect" else ELLIPSE, 0.0])
            blk = b.add(first)
            b.add(second)
            p[rng.choice(("pre", "mid"))].append((_lib.PW_MASK, 0, blk))
        passes.append(p)
    return passes, np.array(b.rows, dtype=np.float64)


def rounded(win, n, br):
    """plan_pruning's entry window: rounded outward to block heights, None where it is no window at all."""
    l, h = int(win[0]), int(win[1])
    l = 0 if l < 0 else (l // br) * br
    h = n if h > n else min(n, -(-h // br) * br)
    return (l, h) if l < h and (l > 0 or h < n) else None


def inside(a, b):
    return b[0] <= a[0] and a[1] <= b[1]


def box(axis, lines, positions):
    """(rows, columns) of a pass's range of lines x range of positions."""
    return (lines, positions) if axis == 0 else (positions, lines)


@pytest.mark.parametrize("n,br", [(64, 4), (2048, 8)])
def test_planner_invariants_on_random_programs(program, n, br):
    rng = random.Random(1000 + n)
    cases = []
    for k in range(60):
        out_item = k % 3
        passes, blocks = random_program(rng, n, out_item)
        entry = k % 4  # no windows | clean rows | stale rows | stale rows and columns
        rows = cols = None
        if entry:
            rows = [sorted(rng.sample(range(0, n + 1), 2)) for _ in range(3)]
        if entry == 3:
            cols = [sorted(rng.sample(range(0, n + 1), 2)) for _ in range(3)]
        cases.append((passes, blocks, rows, entry >= 2, cols, out_item))
    plans = ask(program, [text(n, 3, br, "fp64", p, b, rows=rows, stale=stale, cols=cols) for p, b, rows, stale, cols, _ in cases])
    fills = 0
    for (passes, blocks, rows, stale, cols, out_item), plan in zip(cases, plans):
        assert plan["phases"] == 0 and plan["all_frugal"] == 1 and plan["pruned"] == 1, "every generated pass runs on the frugal kernels"
        for it in range(3):
            act = [(p["axis"], p["items"][it]) for p in plan["passes"] if p["items"][it]["active"]]
            if it == out_item:
                assert not act, "the item that sits out"
                continue
            for axis, f in act:
                for lo, hi in (f["lines"], f["loads"], f["stores"]):
                    assert 0 <= lo < hi <= n and lo % br == 0 and hi % br == 0, f
            for (a0, f0), (a1, f1) in zip(act, act[1:]):
                stored, loaded = box(a0, f0["lines"], f0["stores"]), box(a1, f1["lines"], f1["loads"])
                assert inside(loaded[0], stored[0]) and inside(loaded[1], stored[1]), "a pass loads inside what the pass in front of it stores"
                assert inside(stored[0], loaded[0]) and inside(stored[1], loaded[1]), "a pass processes and stores what the pass behind it reads"
            if not act:
                continue
            # zeros are owed unless the entry rows are clean zeros in memory and every pass is a row pass on exactly those rows
            # that stores every position
            rows0 = rounded(rows[it], n, br) if rows is not None else None
            clean = rows0 is not None and not stale and all(a == 0 and f["lines"] == rows0 and f["stores"] == (0, n) for a, f in act)
            owed = act[-1][1]["lines"] != (0, n) and not clean
            assert [f["fill"] for _, f in act] == [0] * (len(act) - 1) + [int(owed)], "the last active pass alone carries line_fill, when zeros are owed"
            fills += owed
            # the first pass loads inside the entry box
            first_axis, first = act[0]
            cols0 = rounded(cols[it], n, br) if cols is not None and stale else None
            entry_box = (rows0 or (0, n), cols0 or (0, n))
            loaded = box(first_axis, first["lines"], first["loads"])
            assert inside(loaded[0], entry_box[0]) and inside(loaded[1], entry_box[1]), "the first pass loads inside the entry box"
        for p in plan["passes"]:  # the record window of a pass covers the live lines of every item
            if p["mask_block"] >= 0:
                assert all(inside(f["lines"], p["window"]) for f in p["items"] if f["active"])
    assert fills > 20, "the programs exercise line_fill"


# ---- 3. edge shapes -----------------------------------------------------------------------------------------------------
def simple_pass(b, axis, batch, on=None, nfft=1, along=True, aperture=None, slot="mid", phases=1):
    on = on or [1.0] * batch
    p = {"axis": axis, "fft1": b.add([[on[it], 0, 0, 0, 0] for it in range(batch)]), "pre": [], "mid": []}
    if nfft == 2:
        p["fft2"] = b.add([[on[it], 1, 0, 0, 0] for it in range(batch)])
    for _ in range(phases):
        sx, sy = ((0.9, 0.0) if axis == 0 else (0.0, 0.9)) if along else (0.9, 0.7)
        p["mid"].append((_lib.PW_QPHASE_CENTRED, 0, b.add([[on[it], sx, sy, 1e-4, 1.0] for it in range(batch)])))
    if aperture is not None:
        p[slot].append((_lib.PW_MASK, 0, aperture))
    return p


def ellipse(b, batch, n, shift=0.0):
    blk = b.add([[1.0, n / 2 + shift, n / 2 - shift, n / 10, n / 9]] * batch)
    b.add([[0.0, 0.0, 32.0, ELLIPSE, 0.0]] * batch)
    return blk


def test_entry_windows_that_must_be_zeroed_first(program):
    n, br = 64, 4
    b = Blocks(1)
    one = [simple_pass(b, 0, 1)]
    blocks1 = np.array(b.rows)
    b2 = Blocks(2)
    two = [simple_pass(b2, 0, 2, on=[1.0, 0.0])]
    blocks2 = np.array(b2.rows)
    plans = ask(program, [
        text(n, 1, br, "fp64", one, blocks1, rows=[[8, 8]], stale=True),      # empty after rounding
        text(n, 1, br, "fp64", one, blocks1, rows=[[8, 9]], stale=True),      # one block row
        text(n, 2, br, "fp64", two, blocks2, rows=[[8, 24], [8, 24]], stale=True),  # an item no pass touches
        text(n, 1, br, "fp64", one, blocks1, rows=[[8, 24]], stale=True, cols=[[12, 12]]),  # an empty column window ...
        text(n, 1, br, "fp64", one, blocks1, rows=[[8, 24]], stale=True, cols=[[13, 14]]),
        text(n, 1, br, "fp64", one, blocks1, rows=[[8, 24]], stale=True, switches=(1, 1, 1, 1, 1, 1, 1, 0)),  # the planner off
        text(n, 1, br, "fp64", one, blocks1, rows=[[8, 8]], stale=False),     # clean rows: nothing to write
    ])
    assert [p["zero_first"] for p in plans] == [1, 0, 1, 1, 0, 1, 0]
    assert plans[1]["passes"][0]["items"][0]["lines"] == (8, 12) and plans[4]["passes"][0]["items"][0]["loads"] == (12, 16)
    assert plans[0]["passes"][0]["items"][0]["lines"] == (0, n), "an empty window is no window to the planner: hence the zeros first"


def test_a_third_pass_on_the_first_ones_record_set_is_not_fused(program):
    n, br = 1024, 4
    texts = []
    for same in (True, False):
        b = Blocks(1)
        ap0 = ellipse(b, 1, n)
        ap2 = ap0 if same else ellipse(b, 1, n, shift=3.0)
        passes = [simple_pass(b, 0, 1, nfft=2, aperture=ap0), simple_pass(b, 0, 1, nfft=2), simple_pass(b, 0, 1, nfft=1, aperture=ap2)]
        texts.append(text(n, 1, br, "fp64", passes, np.array(b.rows)))
    same, other = ask(program, texts)
    assert same["passes"][0]["set"] == same["passes"][2]["set"] and [g["count"] for g in same["launches"]] == [2, 1]
    assert same["launches"][0]["build"][6] == 2 and same["launches"][1]["build"][6] == 0
    assert other["passes"][0]["set"] != other["passes"][2]["set"] and [g["count"] for g in other["launches"]] == [3]
    assert other["launches"][0]["build"][6] == 3 and other["launches"][0]["tag"] & 32
    assert other["batched"] == [0, 2] and same["batched"] == [], "two renderings go in one batch, one is rendered in place"


def test_single_table_passes(program):
    """A single pass reads tables where it works on at most half of the lines, in complex128 only."""
    texts = []
    for precision, n in (("fp64", 1024), ("fp32", 2048)):
        b = Blocks(1)
        passes = [simple_pass(b, 0, 1)]
        half, more = [[n // 4, 3 * n // 4]], [[n // 4, 3 * n // 4 + 1]]
        for rows in (None, more, half):
            texts.append(text(n, 1, block_rows(precision, n), precision, passes, np.array(b.rows), rows=rows, stale=rows is not None))
    plans = ask(program, texts)
    assert [p["launches"][0]["tables"] for p in plans] == [0, 0, 1, 0, 0, 0]
    assert [p["launches"][0]["build"][5] for p in plans] == [0, 0, 1, 0, 0, 0]
    assert plans[2]["passes"][0]["items"][0]["fill"] == 1 and plans[2]["launches"][0]["grid"] == (0, 0), "a pass that owes zeros runs on the full grid"
    b = Blocks(1)
    across = [simple_pass(b, 0, 1, along=False)]  # a phase that varies across the lines: evaluated whatever the window
    plan, = ask(program, [text(1024, 1, 4, "fp64", across, np.array(b.rows), rows=[[256, 768]], stale=True)])
    assert plan["launches"][0]["tables"] == 0
    b = Blocks(1)
    along = [simple_pass(b, 0, 1)]
    plan, = ask(program, [text(1024, 1, 4, "fp64", along, np.array(b.rows), rows=[[256, 768]], stale=True, switches=(0, 1, 1, 1, 1, 1, 1, 1))])
    assert plan["launches"][0]["tables"] == 0, "PAOS_LINE_TABLES=0"


def _central_text(window1):
    n = 4096
    rc = pb.recipe("fp64", n, pb.Record(0, 1, 1, 2, 0, 1, 1, 0, 1))
    cols = np.array(rc.kw["live_cols"], dtype=np.float64)
    cols[1] = window1
    return text(n, 2, 4, "fp64", rc.passes, rc.blocks, rows=rc.kw["live_rows"], stale=True, cols=cols)


def test_one_item_outside_the_central_half_sends_the_launch_to_the_ordinary_build(program):
    n = 4096
    inside_, touching, outside = ask(program, [_central_text((1024, 3072)), _central_text((1021, 3072)), _central_text((1024, 3076))])
    assert inside_["launches"][0]["build"] == (0, 1, 1, 2, 0, 1, 1, 0, 1)
    for plan in (touching, outside):  # (1021 rounds outward to 1020 < n / 4)
        assert plan["launches"][0]["build"] == (0, 1, 1, 2, 0, 1, 1, 0, 0)
    off, = ask(program, [_central_text((1024, 3072)).replace(f"dims {n} 2 4 0 1", f"dims {n} 2 4 0 0")])
    assert off["launches"][0]["build"][8] == 0, "a context created with the central-half builds switched off"


def test_a_table_budget_above_one_gib_stages_launch_by_launch(program):
    n, batch = 4096, 32  # two tables of 2 MiB per pass: 256 passes are 1 GiB
    b = Blocks(batch)
    p = simple_pass(b, 0, batch)
    blocks = np.array(b.rows)
    at, above, off = ask(program, [text(n, batch, 4, "fp64", [p] * 256, blocks), text(n, batch, 4, "fp64", [p] * 257, blocks),
                                   text(n, batch, 4, "fp64", [p] * 2, blocks, switches=(1, 1, 1, 1, 0, 1, 1, 1))])
    assert (at["staged_whole"], above["staged_whole"], off["staged_whole"]) == (1, 0, 0)
    assert len(above["launches"]) == 257


def test_what_the_last_pass_stores_and_the_zeros_a_psf_store_owes(program):
    n, br = 1024, 4
    b = Blocks(2)
    last = simple_pass(b, 1, 2)
    sat_out = simple_pass(b, 1, 2, on=[1.0, 0.0])
    three = simple_pass(b, 1, 2, phases=2)
    blocks = np.array(b.rows)
    rows = [[256, 512], [256, 768]]
    plans = ask(program, [
        text(n, 2, br, "fp64", [last], blocks, final=1),
        text(n, 2, br, "fp64", [last], blocks, final=2),
        text(n, 2, br, "fp64", [sat_out], blocks, final=1),   # an item sits the last pass out: the sweep follows
        text(n, 2, br, "fp64", [three], blocks, final=1),     # two phases behind the transform: no PSF-storing shape
        text(n, 2, br, "fp64", [three], blocks, final=2),     # ... but a power-summing one
        # a column pass behind stale columns: live lines [256, 512) and [256, 768); the buffer is known to hold [256, 512) of both
        text(n, 2, br, "fp64", [last], blocks, final=1, rows=[[0, n]] * 2, stale=True, cols=rows, psfmem=(1, [[256, 512], [256, 512]])),
        text(n, 2, br, "fp64", [last], blocks, final=1, rows=[[0, n]] * 2, stale=True, cols=rows, psfmem=(0, [[256, 512], [256, 512]])),
        text(n, 2, br, "fp64", [last], blocks, final=1, rows=[[0, n]] * 2, stale=True, cols=rows, psfmem=(1, [[256, 516], [256, 512]])),
    ])
    assert [p["store"] for p in plans] == [1, 2, 0, 0, 2, 1, 1, 1]
    assert [p["launches"][0]["build"][4] for p in plans] == [1, 2, 0, 0, 2, 1, 1, 1]
    items = [[(f["fill"], f["stores"]) for f in p["passes"][0]["items"]] for p in plans]
    assert items[0] == [(0, (0, n))] * 2, "nothing known and every line live: every old line is rewritten"
    assert items[5] == [(0, (0, n))] * 2, "the same axis and the old lines inside the new ones: no zeros owed"
    assert items[6] == [(1, (0, n))] * 2, "another axis: nothing known, the dead tiles write zeros"
    assert items[7] == [(1, (256, 516)), (0, (0, n))], "item 0's old lines reach beyond its new ones"
    assert plans[7]["psfmem"] == [256, 512, 256, 768] and plans[5]["launches"][0]["grid"] == (256, 768)
    assert plans[7]["launches"][0]["tag"] & 8
