#!/usr/bin/env python3
"""build_census.py LOG...: which builds of the frugal pass kernel a run launched.

Reads the "build ..." lines a library writes to stderr under PAOS_DUMP_PASSES=1 (csrc/passes.hip: launch_lowered -- the nine
fields of the build, the grid size and the precision), e.g. the stderr of a whole `pytest -m gpu -s` run -- as written, or
condensed by `grep '^build ' | sort | uniq -c` --, and reports per
family (precision, n) how many distinct records were launched, out of how many the library has a build for
(paos_frugal_built; tests/pass_builds.py: built_records) and of those a program can reach.  --missing lists the built,
reachable records the run never launched, one per line."""
import collections
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

LINE = re.compile(r"^\s*(?:(\d+)\s+)?build axis (\d+) kpre (\d+) kmid (\d+) nfft (\d+) store (\d+) tab (\d+) fuse (\d+) one_line (\d+) central (\d+) "
                  r"n (\d+) (fp64|fp32)\s*$")


def census(lines):
    """{(precision, n): Counter of records (tuples of nine ints)}"""
    seen = collections.defaultdict(collections.Counter)
    for line in lines:
        m = LINE.match(line)
        if m:
            seen[(m.group(12), int(m.group(11)))][tuple(int(v) for v in m.groups()[1:10])] += int(m.group(1) or 1)
    return seen


def main(argv):
    import pass_builds as pb

    missing = "--missing" in argv
    seen = collections.defaultdict(collections.Counter)
    for path in (a for a in argv if a != "--missing"):
        with open(path, errors="replace") as fh:
            for family, records in census(fh).items():
                seen[family].update(records)
    total = [0, 0, 0]
    for family in pb.FAMILIES:
        built = pb.built_records(*family)
        reachable = [r for r in built if (family[0], family[1], r) not in pb.UNREACHABLE]
        got = [r for r in built if tuple(r) in seen[family]]
        names = set(built)
        stray = [r for r in seen[family] if pb.Record(*r) not in names]
        by_class = collections.Counter(pb.classify(r) for r in got)
        print(f"{family[0]} {family[1]}: launched {len(got)} of {len(built)} built records ({len(reachable)} reachable), "
              f"{sum(seen[family].values())} launches; by class {dict(sorted(by_class.items()))}"
              + (f"; NOT BUILT: {stray}" if stray else ""))
        if missing:
            for r in reachable:
                if tuple(r) not in seen[family]:
                    print("  missing", " ".join(f"{k} {v}" for k, v in zip(pb.FIELDS, r)))
        total = [total[0] + len(got), total[1] + len(built), total[2] + len(reachable)]
    print(f"all families: launched {total[0]} of {total[1]} built records ({total[2]} reachable)")
    others = sorted(f for f in seen if f not in pb.FAMILIES)
    if others:
        print("lines of other families (no frugal builds there):", others)


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(sys.argv[1:])
