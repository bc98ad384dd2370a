#!/usr/bin/env python3
"""Time the blurred PSFs (paos_blur_apply, include/paos_hip.h) at 1024^2 x 64, 2048^2 x 16 and 4096^2 x 8, fp64, beside
paos_otf_compute on the same context:

  1. paos_blur_apply -- table upload, the column launch (spectrum x T, inverse transform along ky, row pairs re-tangled
     into the PSF buffer) and the row launch (N/2 packed lines in place), about N line transforms per item;
  2. paos_otf_compute -- the packed real-input forward transform, about N line transforms per item as well: what
     paos_blur_apply is expected to cost (an expectation, not a gate).

Both are the sums of their two launches as the library's launch timer reports them (HIP events around each launch:
device time, no host work in between) and are timed once more with HIP events around the whole call, host work and table
upload included -- paos_blur_apply twice: with the parameters of the call before (the context keeps the tables it has
evaluated) and with new sigmas (every table is evaluated again, in long double on the host).  They alternate, `--reps` repeats after a warm-up; medians and the spread (min, max) are reported, in
milliseconds per call and per item.  Writes a Markdown record (`--out`) and prints it.

    python3 tools/blur_bench.py --out build/blur_bench.md
"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SHAPES = ((1024, 64), (2048, 16), (4096, 8))
DX, DY = 1.0e-5, 1.3e-5


def spread(values, per=1.0):
    return f"{statistics.median(values) / per:.4f} ({min(values) / per:.4f} .. {max(values) / per:.4f})"


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
        sx = np.linspace(1.0, 3.0, batch) * DX
        sy = np.linspace(2.5, 0.5, batch) * DY

        def blur(stretch=1.0):
            dev.blur_apply(DX, DY, sx * stretch, sy * stretch, 2.0 * DX, 2.0 * DY)

        timer = EventTimer(hip_runtime(), dev.stream)
        rows = {"blur cols": [], "blur rows": [], "otf rows": [], "otf cols": [], "blur (events)": [], "blur, new tables (events)": [],
                "otf (events)": []}
        lines = {}
        for rep in range(warmup + reps):
            dev.psf_keep()  # (a fresh optical PSF: a blur compounds)
            ms_o, ln_o = launches(dev, _lib, dev.otf_compute)
            ms_b, ln_b = launches(dev, _lib, blur)
            dev.psf_keep()
            ev_o = timer.ms(dev.otf_compute)
            ev_b = timer.ms(blur)
            dev.psf_keep()
            dev.otf_compute()
            ev_n = timer.ms(lambda: blur(1.0 + 1.0e-3 * (rep + 1)))
            blur()  # (the tables of the next round's calls again)
            assert ms_o.size == 2 and ms_b.size == 2
            if rep < warmup:
                continue
            for key, v in (("otf rows", ms_o[0]), ("otf cols", ms_o[1]), ("blur cols", ms_b[0]), ("blur rows", ms_b[1]),
                           ("otf (events)", ev_o), ("blur (events)", ev_b), ("blur, new tables (events)", ev_n)):
                rows[key].append(float(v))
            lines = {"otf": ln_o / batch, "blur": ln_b / batch}
    finally:
        dev.close()
    blur_ms = [a + b for a, b in zip(rows["blur cols"], rows["blur rows"])]
    otf_ms = [a + b for a, b in zip(rows["otf rows"], rows["otf cols"])]
    return rows, blur_ms, otf_ms, lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("build", "blur_bench.md"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    out = ["| shape | precision | blur_apply [ms/item] | blur_apply [ms] | cols | rows | lines/item (cols, rows) | otf_compute [ms] | "
           "rows | cols | blur / otf | blur, events [ms] | blur with new tables, events [ms] | otf, events [ms] |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for n, batch in SHAPES:
        rows, blur_ms, otf_ms, lines = measure(n, batch, "fp64", args.reps, args.warmup)
        ratio = statistics.median(blur_ms) / statistics.median(otf_ms)
        out.append(f"| {n}^2 x {batch} | fp64 | {spread(blur_ms, batch)} | {spread(blur_ms)} | {spread(rows['blur cols'])} | "
                   f"{spread(rows['blur rows'])} | {lines['blur'][0]:.0f}, {lines['blur'][1]:.0f} | {spread(otf_ms)} | "
                   f"{spread(rows['otf rows'])} | {spread(rows['otf cols'])} | {ratio:.3f} | {spread(rows['blur (events)'])} | {spread(rows['blur, new tables (events)'])} | "
                   f"{spread(rows['otf (events)'])} |")
        print(out[-1], flush=True)
    text = (f"Medians (min .. max) of {args.reps} alternating repeats after {args.warmup} warm-up rounds; launch times by the "
            "library's launch timer, call times by HIP events on the context's stream.\n\n" + "\n".join(out) + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
