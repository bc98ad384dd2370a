#!/usr/bin/env python3
"""Time the transfer functions (paos_otf_*, include/paos_hip.h) at 4096^2 x 32 and 1024^2 x 256, fp64 and fp32:

  1. paos_otf_compute -- the packed real-input 2-D transform of the kept PSFs, about N line transforms per item;
  2. paos_otf_compute + paos_otf_cuts -- what a sweep pays per batch, the small copy and its synchronisation included;
  3. paos_focus_begin on the same context -- the library's own complex forward 2-D transform, 2 N line transforms per
     item: the yardstick.

1 and 3 are the sums of their two launches as the library's launch timer reports them (HIP events around each launch:
device time, no host work in between), which also says which launch a ratio is owed to; 1 and 2 are timed once more
with HIP events around the whole call (2 ends in a synchronisation).  The three alternate, `--reps` repeats after a
warm-up; medians and the spread (min, max) are reported.  Writes a Markdown record (`--out`) and prints it.

    python3 tools/otf_bench.py --out build/otf_bench.md
"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SHAPES = ((4096, 32), (1024, 256))


def spread(values):
    return f"{statistics.median(values):.3f} ({min(values):.3f} .. {max(values):.3f})"


def launches(dev, _lib, work):
    """(ms per launch, line transforms per launch) of what ``work()`` enqueues, by the library's launch timer."""
    dev.profile_begin(_lib.KERNEL_PASS_ANY)
    work()
    lines = dev.profile_line_transforms()
    ms, _ = dev.profile_end_launches()
    return ms, lines


def measure(n, batch, precision, reps, warmup):
    from focus_bench import EventTimer, hip_runtime
    from paos_amd import _lib

    dev = _lib.DeviceFields(n, batch, precision)
    try:
        rng = np.random.default_rng(n + batch)
        dev.fill(0.6 + 0.3j)
        dev.upload(0, rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
        dev.psf_keep()
        timer = EventTimer(hip_runtime(), dev.stream)
        rows = {"otf rows": [], "otf cols": [], "focus rows": [], "focus cols": [], "compute (events)": [],
                "compute + cuts (events)": []}
        lines = {}
        for rep in range(warmup + reps):
            ms_o, ln_o = launches(dev, _lib, dev.otf_compute)
            ms_f, ln_f = launches(dev, _lib, dev.focus_begin)
            dev.focus_end()
            ev_c = timer.ms(dev.otf_compute)
            ev_cc = timer.ms(lambda: (dev.otf_compute(), dev.otf_cuts()))
            assert ms_o.size == 2 and ms_f.size == 2
            if rep < warmup:
                continue
            for key, v in (("otf rows", ms_o[0]), ("otf cols", ms_o[1]), ("focus rows", ms_f[0]), ("focus cols", ms_f[1]),
                           ("compute (events)", ev_c), ("compute + cuts (events)", ev_cc)):
                rows[key].append(float(v))
            lines = {"otf": ln_o / batch, "focus": ln_f / batch}
    finally:
        dev.close()
    compute = [a + b for a, b in zip(rows["otf rows"], rows["otf cols"])]
    focus = [a + b for a, b in zip(rows["focus rows"], rows["focus cols"])]
    return rows, compute, focus, lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("build", "otf_bench.md"))
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    out = ["| shape | precision | otf_compute [ms] | rows | cols | lines/item (rows, cols) | focus_begin [ms] | rows | cols | "
           "compute / focus_begin | compute, events [ms] | compute + cuts, events [ms] |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for n, batch in SHAPES:
        for precision in ("fp64", "fp32"):
            rows, compute, focus, lines = measure(n, batch, precision, args.reps, args.warmup)
            ratio = statistics.median(compute) / statistics.median(focus)
            out.append(f"| {n}^2 x {batch} | {precision} | {spread(compute)} | {spread(rows['otf rows'])} | {spread(rows['otf cols'])} | "
                       f"{lines['otf'][0]:.0f}, {lines['otf'][1]:.0f} | {spread(focus)} | {spread(rows['focus rows'])} | "
                       f"{spread(rows['focus cols'])} | {ratio:.3f} | {spread(rows['compute (events)'])} | "
                       f"{spread(rows['compute + cuts (events)'])} |")
            print(out[-1], flush=True)
    text = (f"Medians (min .. max) of {args.reps} alternating repeats after {args.warmup} warm-up rounds; launch times by the "
            "library's launch timer, call times by HIP events on the context's stream.\n\n" + "\n".join(out) + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
