"""The item grouping of the pointwise host code (paos_amd/csrc/item_groups.h) against a restatement of its rule, on the CPU:
tests/item_groups_main.cpp is compiled with the address and undefined-behaviour sanitizers and run as a child process."""
import math
import os
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = struct.unpack("<d", bytes.fromhex("010000000000f87f"))[0]  # a quiet NaN with a payload


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("item_groups") / "item_groups_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "item_groups_main.cpp"), "-o", exe], check=True)
    return exe


def bits(x):
    return struct.pack("<d", x).hex()  # what "bitwise equal" compares


def wire(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", x))[0]


def ask(program, head, rows):
    text = head + "\n" + "\n".join(" ".join(w if isinstance(w, str) else str(w) for w in row) for row in rows) + "\n"
    out = subprocess.run([program], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    return {line.split()[0]: [int(v) for v in line.split()[1:]] for line in out.stdout.splitlines()}


# ---- the rule, restated ---------------------------------------------------------------------------------------------
def same(a, b, skip=-1):
    return all(bits(x) == bits(y) for k, (x, y) in enumerate(zip(a, b)) if k != skip)


def groups(n, joins, part):
    leaders, of = [], {}
    for i in range(n):
        if part(i):
            of[i] = next((l for l in leaders if joins(l, i)), i)
            leaders += [i] if of[i] == i else []
    goff, glen, members = [0] * n, [0] * n, []
    for l in leaders:
        mine = [i for i in range(n) if of.get(i) == l]
        goff[l], glen[l] = len(members), len(mine)
        members += mine
    return goff, glen, members


def split(goff, glen, members, recs, enable, skip, share):
    goff, glen, subs, out = list(goff), list(glen), [], []
    for l in [l for l in range(len(recs)) if glen[l]]:
        left, first = members[goff[l]:goff[l] + glen[l]], len(subs) // 3
        while left:
            a = left[0]
            off = recs[a][enable] == 0.0
            sub = [b for b in left if b == a or (off and recs[b][enable] == 0.0) or
                   (not off and recs[b][enable] != 0.0 and share and same(recs[a], recs[b], skip))]
            subs += [-1 if off else a, len(out), len(sub)]
            out += sub
            left = [b for b in left if b not in sub]
        goff[l], glen[l] = first, len(subs) // 3 - first
    return subs, goff, glen, out


# ---- group_items ------------------------------------------------------------------------------------------------------
A, B, C = [1.0, 2.0, 3.0], [1.0, 2.5, 3.0], [4.0, 2.0, 3.0]
GROUP_CASES = {
    "batch 1": ([A], [1], -1),
    "all distinct": ([A, B, C, [0.0, 0.0, 0.0]], [1] * 4, -1),
    "all identical": ([A] * 5, [1] * 5, -1),
    "interleaved": ([A, B, A, B, A], [1] * 5, -1),
    "no part in front, between, behind": ([A, A, B, A, B, B, A, A], [0, 1, 1, 0, 1, 1, 1, 0], -1),
    "differ at the skipped index only": ([A, B, A, C], [1] * 4, 1),
    "differ in the sign of a zero": ([[0.0, 1.0], [-0.0, 1.0], [0.0, 1.0]], [1] * 3, -1),
    "a NaN with equal bits": ([[NAN, 1.0], [NAN, 1.0], [math.nan, 1.0]], [1] * 3, -1),
    "nobody takes part": ([A, A, B], [0] * 3, -1),
}


@pytest.mark.parametrize("name", list(GROUP_CASES))
def test_group_items(program, name):
    recs, part, skip = GROUP_CASES[name]
    n = len(recs)
    got = ask(program, f"groups {n} {len(recs[0])} {skip}", [[part[i]] + [wire(v) for v in recs[i]] for i in range(n)])
    goff, glen, members = groups(n, lambda l, i: same(recs[l], recs[i], skip), lambda i: part[i])
    assert (got["goff"], got["glen"], got["members"]) == (goff, glen, members)
    assert sorted(members) == [i for i in range(n) if part[i]]  # everybody who takes part is listed once


def test_known_groups(program):
    """The answers themselves, not only their agreement with the restatement."""
    recs, part, skip = GROUP_CASES["interleaved"]
    got = ask(program, "groups 5 3 -1", [[1] + [wire(v) for v in r] for r in recs])
    assert got == {"goff": [0, 3, 0, 0, 0], "glen": [3, 2, 0, 0, 0], "members": [0, 2, 4, 1, 3]}
    recs, part, skip = GROUP_CASES["differ in the sign of a zero"]
    got = ask(program, "groups 3 2 -1", [[1] + [wire(v) for v in r] for r in recs])
    assert got["glen"] == [2, 1, 0] and got["members"] == [0, 2, 1]
    assert bits(NAN) != bits(math.nan)  # (the third NaN of that case has other bits: a group of its own)
    recs, part, skip = GROUP_CASES["a NaN with equal bits"]
    got = ask(program, "groups 3 2 -1", [[1] + [wire(v) for v in r] for r in recs])
    assert got["glen"] == [2, 0, 1] and got["members"] == [0, 1, 2]


# ---- map_groups: zernike_apply's caller ------------------------------------------------------------------------------
# records: enable, 1 / wavelength (skipped), coefficient
MAP_CASES = {
    "two maps and a disabled item": [[1.0, 1e6, 0.5], [1.0, 2e6, 0.25], [0.0, 1e6, 0.5], [1.0, 3e6, 0.5], [1.0, 1e6, 0.25]],
    "every item disabled": [[0.0, 1e6, 0.5], [0.0, 2e6, 0.5], [0.0, 1e6, 0.25]],
}


@pytest.mark.parametrize("share", [1, 0])
@pytest.mark.parametrize("name", list(MAP_CASES))
def test_map_groups(program, name, share):
    recs = MAP_CASES[name]
    n = len(recs)
    got = ask(program, f"maps {n} 3 0 1 {share}", [[wire(v) for v in r] for r in recs])
    goff, glen, members = groups(n, lambda l, i: bool(share) and same(recs[l], recs[i], 1), lambda i: recs[i][0] != 0.0)
    assert (got["goff"], got["glen"]) == (goff, glen)
    assert got["members"] == (members or [0])  # never an empty list: one entry of padding
    if name == "every item disabled":
        assert got == {"goff": [0] * n, "glen": [0] * n, "members": [0]}


# ---- the sub-groups of start_impl's Zernike branch -------------------------------------------------------------------
# start keys: items 0, 2, 3, 5 start from one field, 1 and 4 from another; maps: X for 0 and 3, Y for 2, item 5 disabled
X, Y, OFF = [1.0, 1e6, 0.5], [1.0, 1e6, 0.75], [0.0, 1e6, 0.5]
SUB_KEYS = [7, 8, 7, 7, 8, 7]
SUB_RECS = [X, X, Y, [1.0, 2e6, 0.5], OFF, OFF]


@pytest.mark.parametrize("share", [1, 0])
def test_sub_groups(program, share):
    n = len(SUB_RECS)
    got = ask(program, f"subs {n} 3 0 1 {share}", [[SUB_KEYS[i]] + [wire(v) for v in SUB_RECS[i]] for i in range(n)])
    goff, glen, members = groups(n, lambda l, i: SUB_KEYS[l] == SUB_KEYS[i], lambda i: True)
    assert got["lead"] == [1 if glen[i] else 0 for i in range(n)]
    assert got["same"] == [next(l for l in range(n) if i in members[goff[l]:goff[l] + glen[l]]) for i in range(n)]
    subs, goff, glen, members = split(goff, glen, members, SUB_RECS, 0, 1, bool(share))
    assert (got["subs"], got["goff"], got["glen"], got["members"]) == (subs, goff, glen, members)
    if share:  # group 0: maps X (items 0, 3), Y (2) and the disabled item 5, which owns -1; group 1: X (1) and disabled (4)
        assert got["subs"] == [0, 0, 2, 2, 2, 1, -1, 3, 1, 1, 4, 1, -1, 5, 1]
        assert got["goff"][:2] == [0, 3] and got["glen"] == [3, 2, 0, 0, 0, 0] and got["members"] == [0, 3, 2, 5, 1, 4]
    else:
        assert got["glen"] == [4, 2, 0, 0, 0, 0] and got["members"] == [0, 2, 3, 5, 1, 4]


# ---- the representatives of the power sums ---------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [[1, 1, 1, 1, 1], [0, 1, 1, 0, 1], [0, 0, 0, 0, 0]])
def test_power_representatives(program, flags):
    recs = GROUP_CASES["interleaved"][0]
    got = ask(program, "reps 5 3", [[flags[i]] + [wire(v) for v in recs[i]] for i in range(5)])
    power_of = [next((j for j in range(i) if flags[j] and same(recs[j], recs[i])), i) for i in range(5)]
    assert got["power_of"] == power_of
    assert got["compute"] == [1 if flags[i] and power_of[i] == i else 0 for i in range(5)]


# ---- same_as ---------------------------------------------------------------------------------------------------------
SAME_AS = {  # list -> valid under (zernike_like: any item index, norm2: an item that stands for itself)
    "identity": ([0.0, 1.0, 2.0], True, True),
    "leaders": ([0.0, 0.0, 2.0, 2.0], True, True),
    "non-integer": ([0.0, 0.5, 2.0], False, False),
    "negative": ([0.0, -1.0, 2.0], False, False),
    "out of range": ([0.0, 3.0, 2.0], False, False),
    "NaN": ([0.0, math.nan, 2.0], False, False),
    "not self-standing": ([1.0, 2.0, 2.0], True, False),
}


@pytest.mark.parametrize("name", list(SAME_AS))
def test_same_as(program, name):
    same_as, any_index, self_standing = SAME_AS[name]
    for rule, want in ((0, any_index), (1, self_standing)):
        got = ask(program, f"sameas {len(same_as)} {rule}", [[wire(v) for v in same_as]])
        assert got["valid"] == [1 if want else 0], (name, rule)
