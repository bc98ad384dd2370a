"""The offset arithmetic of the parameter arena (paos_amd/csrc/arena_layout.h) on the CPU: tests/arena_layout_main.cpp plays
the host code's part over one slab in ordinary memory, is compiled with the address and undefined-behaviour sanitizers and
run as a child process.  Checked over random sequences of block sizes: where the blocks go, and which range a commit copies."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 256       # doubles per slab: sixteen blocks of the smallest size
ALIGN = 16
SLACK = 64      # what a reservation adds for the rounding of its blocks (kArenaSlack)
SIZES = [0, 1, 15, 16, 17, CAP - 1, CAP]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("arena_layout") / "arena_layout_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "arena_layout_main.cpp"), "-o", exe], check=True)
    return exe


def ask(program, cap, commands):
    """The program's answers, one list of words per command that prints."""
    text = f"{cap}\n" + "\n".join(commands) + "\n"
    out = subprocess.run([program], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    return [line.split() for line in out.stdout.splitlines()]


def rounded(count):
    return (count + ALIGN - 1) // ALIGN * ALIGN


class Slab:
    """What the test knows of the slab being filled: its blocks, and where the pending range starts."""

    def __init__(self, cap):
        self.cap, self.blocks, self.head, self.first_pending = cap, [], 0, None

    def fresh(self, cap=None):
        self.__init__(cap or self.cap)

    def placed(self, off, count, head):
        assert off % ALIGN == 0 and head % ALIGN == 0                       # offsets are multiples of 16 doubles
        assert off + count <= self.cap and head <= self.cap                 # no block crosses the slab's end
        assert off == self.head and head == off + rounded(count)            # blocks follow each other, rounded
        for o, c in self.blocks:
            assert off >= o + c, "blocks overlap"
        self.blocks.append((off, count))
        self.head = head
        if self.first_pending is None:
            self.first_pending = off

    def committed(self, words):
        if self.first_pending is None or self.first_pending == self.head:  # (nothing added, or empty blocks only)
            assert words == ["commit", "none"]
            self.first_pending = None
            return
        first, count = int(words[1]), int(words[2])
        assert first == self.first_pending and first + count == self.head   # exactly first offset ... head
        self.first_pending = None


@pytest.mark.parametrize("seed", range(8))
def test_blocks_pushed_one_by_one_and_in_unreserved_batches(program, seed):
    """Batches without a reservation (arena_push, the launch-by-launch paths): a block that does not fit goes to a fresh
    slab, behind the copy of what was pending in the one it leaves."""
    rng = random.Random(seed)
    commands, plan = [], []
    for _ in range(60):
        sizes = [rng.choice(SIZES) for _ in range(rng.choice([1, 1, 2, 3, 6]))]
        commands += ["batch"] + [f"add {s}" for s in sizes] + ["commit", "state"]
        plan.append(sizes)
    answers = iter(ask(program, CAP, commands))
    slab = Slab(CAP)
    for sizes in plan:
        for s in sizes:
            words = next(answers)
            assert words[0] == "add" and words[1] != "refused", words
            if words[1] == "switch":
                assert slab.head + s > CAP, "left a slab the block would have fitted"
                slab.fresh()
                words = [words[0]] + words[2:]
            slab.placed(int(words[1]), s, int(words[2]))
        slab.committed(next(answers))
        assert next(answers) == ["state", str(slab.head), str(slab.head), "0"]


@pytest.mark.parametrize("seed", range(8))
def test_reserved_batches_stay_in_one_slab(program, seed):
    """A batch that begins with the sum of its blocks never leaves its slab: room is made before the first block -- a fresh
    slab, or larger slabs when no slab holds it -- and every block is accepted where the one before it ended."""
    rng = random.Random(100 + seed)
    commands, plan = [], []
    for _ in range(40):
        sizes = [rng.choice(SIZES[:5] if rng.random() < 0.8 else SIZES) for _ in range(rng.choice([1, 2, 5, 14]))]
        commands += ["batch", f"begin {sum(rounded(s) for s in sizes)}"] + [f"add {s}" for s in sizes] + ["commit", "add 1"]
        plan.append(sizes)
    answers = iter(ask(program, CAP, commands))
    slab = Slab(CAP)
    for sizes in plan:
        total = sum(rounded(s) for s in sizes)
        words = next(answers)
        want = "grow" if total + SLACK > slab.cap else ("switch" if slab.head + total + SLACK > slab.cap else "fits")
        assert words[:2] == ["begin", want], (words, total, slab.head, slab.cap)
        if want == "grow":  # a batch larger than the slab asks for growth before its first block
            assert int(words[2]) >= total + SLACK and int(words[2]) % slab.cap == 0
        if want != "fits":
            slab.fresh(int(words[2]))
            assert int(words[3]) == 0
        for s in sizes:
            words = next(answers)
            assert words[0] == "add" and words[1] not in ("refused", "switch"), words
            slab.placed(int(words[1]), s, int(words[2]))
        slab.committed(next(answers))
        assert next(answers) == ["add", "refused", "closed"]  # the launches behind the commit may be reading


def test_known_answers(program):
    """The answers themselves: rounding, the slab's last block, an outgrown reservation, a dropped range."""
    got = ask(program, CAP, ["batch", "add 0", "add 1", "add 17", "state", "commit", "commit",
                             "batch", f"add {CAP - 1}",                      # does not fit behind 48: a fresh slab, all of it
                             "commit", "batch", "add 1", "batch", f"add {CAP}",
                             "drop", "state",
                             "batch", "begin 16", "add 16", "add 16", "add 16", "add 16", "add 16", "add 176", "add 1"])
    assert got == [["add", "0", "0"], ["add", "0", "16"], ["add", "16", "48"], ["state", "48", "0", "1"], ["commit", "0", "48"],
                   ["commit", "none"],
                   ["add", "switch", "0", str(CAP)],
                   ["commit", "0", str(CAP)], ["add", "switch", "0", "16"], ["add", "switch", "0", str(CAP)],
                   ["drop"], ["state", str(CAP), str(CAP), "0"],
                   ["begin", "switch", str(CAP), "0"], ["add", "0", "16"], ["add", "16", "32"], ["add", "32", "48"], ["add", "48", "64"],
                   ["add", "64", "80"], ["add", "80", str(CAP)], ["add", "refused", "room"]]
