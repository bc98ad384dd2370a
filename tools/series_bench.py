#!/usr/bin/env python3
"""Time a pointing series of the kept PSFs (paos_series_compute / paos_series_fetch, include/paos_hip.h), fp64:

  (a) one series_compute + series_fetch at 4096^2 x 32 on a 64 x 64 detector at a pitch of 5 dx, T = 256 offsets (Gaussian
      jitter of one pitch rms), 4 boxes and a pixel response, ``frames=False``, by the host's clock around the call pair
      (the fetch synchronises) -- beside the only way the library offered before: T calls of
      ``detector_images(..., origins=...)`` on the same detector plus the box sums on the host.  The same with
      ``frames=True``, and with T = 64 and 1024 (does a frame cost the same whatever the length of the series?);
  (b) wavefronts/s of a SYN20 sweep at 4096^2 x 32 with ``outputs=(), pointing=PointingSeries(...)`` (T = 256, 4 boxes)
      beside the plain lean sweep; the two alternate on one context.

`--reps` repeats after a warm-up; medians and the spread (min .. max).  Writes a Markdown record (`--out`) and prints it.

    python3 tools/series_bench.py --out build/series_bench.md
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FIELD = {"us": 0.0, "ut": 0.0}
DX0 = 1.0e-6
BOXES = [(24, 40, 24, 40), (28, 36, 28, 36), (0, 64, 0, 64), (31, 33, 31, 33)]


def spread(values, per=1.0):
    return f"{statistics.median(values) / per:.3f} ({min(values) / per:.3f} .. {max(values) / per:.3f})"


def measure_calls(n, batch, frames_list, reps, warmup):
    from paos_amd import _lib
    from paos_amd.detector import Detector

    dev = _lib.DeviceFields(n, batch, "fp64")
    out, notes = [], []
    try:
        rng = np.random.default_rng(n + batch)
        j = np.arange(n, dtype=np.float64)
        env = np.exp(-((j - n / 2 - 3.3) ** 2) / (4.0 * (n / 64.0) ** 2))
        dev.fill(0.0)
        for i in range(min(batch, 4)):  # (a few speckled blobs; the other items stay zero: every frame reads them all the same)
            dev.upload(i, (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) * env[:, None] * env[None, :])
        dev.psf_keep()
        dxs = DX0 * np.linspace(1.0, 1.3, batch)
        det = Detector(64, 64, 5.0 * DX0)
        gains = 1.0 + 0.02 * rng.standard_normal((det.ny, det.nx))
        dev.detector_begin(det)
        for nt in frames_list:
            off = det.pitch_x * rng.standard_normal((nt, 2))
            lean, full, loop = [], [], []
            flux = ref = None
            for rep in range(warmup + reps):
                dev.sync()
                t0 = time.perf_counter()
                dev.series_compute(det, dxs, dxs, off, BOXES, response=gains)
                flux = dev.series_fetch()
                t1 = time.perf_counter()
                dev.series_compute(det, dxs, dxs, off, BOXES, response=gains, frames=True)
                dev.series_fetch()
                t2 = time.perf_counter()
                ref = np.empty((batch, nt, len(BOXES)))
                for t in range(nt):  # the loop of the parent commit: a call and a copy of every frame per time step
                    images = dev.detector_images(dxs, dxs, origins=off[t]) * gains
                    for a, (m0, m1, n0, n1) in enumerate(BOXES):
                        ref[:, t, a] = images[:, n0:n1, m0:m1].sum(axis=(1, 2))
                t3 = time.perf_counter()
                if rep >= warmup:
                    lean.append(1.0e3 * (t1 - t0))
                    full.append(1.0e3 * (t2 - t1))
                    loop.append(1.0e3 * (t3 - t2))
            scale = np.max(np.abs(ref))
            assert np.max(np.abs(flux - ref)) <= 1.0e-12 * scale, "the series and the loop disagree"
            ratio = statistics.median(loop) / statistics.median(lean)
            per_frame = 1.0e3 * statistics.median(lean) / nt
            out.append(f"| {n}^2 x {batch} | {nt} | {spread(lean)} | {per_frame:.2f} | {spread(full)} | {spread(loop)} | {ratio:.1f} |")
            print(out[-1], flush=True)
            # what the frames kernel asks of the caches: every pixel of every frame reads its window of grid pixels
            window = (5.0 * DX0 / dxs + 1.0) ** 2
            loads = float(np.sum(window)) * nt * det.nx * det.ny * 8.0
            notes.append(f"- T = {nt}: about {loads / 1e9:.1f} GB of window loads in {statistics.median(lean):.2f} ms "
                         f"({loads / statistics.median(lean) / 1e9:.2f} TB/s asked of the caches); the footprints hold "
                         f"{float(np.sum((64 * 5.0 * DX0 / dxs) ** 2)) * 8 / 1e6:.0f} MB of the {batch * n * n * 8 / 1e9:.1f} GB PSF buffer, "
                         f"all frames {batch * nt * det.nx * det.ny * 8 / 1e6:.0f} MB (the frame buffer holds at most 537 MB of them "
                         f"at a time).")
    finally:
        dev.close()
    return out, notes


def measure_sweep(n, batch, reps, warmup):
    from paos_amd import PointingSeries, _lib
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.detector import Detector
    from paos_amd.run import run_batch

    wls = [syn20_wavelength((511 * k) // max(1, batch - 1)) for k in range(batch)]
    chains = [syn20_chain() for _ in wls]
    dev = _lib.DeviceFields(n, batch, "fp64")
    try:
        first = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=(), dev=dev)
        dx = first[0][20]["dx"]
        det = Detector(64, 64, 5.0 * dx)
        off = det.pitch_x * np.random.default_rng(1).standard_normal((256, 2))
        ways = {"lean (no series)": {}, "pointing=PointingSeries(64 x 64 at 5 dx, T = 256, 4 boxes)": {"pointing": PointingSeries(det, off, apertures=BOXES)}}
        rates = {name: [] for name in ways}
        for rep in range(warmup + reps):
            for name, kw in ways.items():
                dev.sync()
                t0 = time.perf_counter()
                run_batch(1.0, wls, n, 4, FIELD, chains, outputs=(), dev=dev, **kw)
                dev.sync()
                if rep >= warmup:
                    rates[name].append(batch / (time.perf_counter() - t0))
    finally:
        dev.close()
    return [f"| {name} | {spread(vals, 1.0)} |" for name, vals in rates.items()]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("build", "series_bench.md"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, nargs="+", default=[256, 64, 1024])
    ap.add_argument("--skip-sweep", action="store_true")
    args = ap.parse_args()
    out = ["(a) one series_compute + series_fetch, 64 x 64 detector at a pitch of 5 dx, 4 boxes, a pixel response, fp64; milliseconds "
           "by the host's clock\n",
           "| shape | T | series, frames=False | per frame, us | series, frames=True | T x detector_images + host sums | loop / series |",
           "|---|---|---|---|---|---|---|"]
    rows, notes = measure_calls(4096, 32, args.frames, args.reps, args.warmup)
    out += rows + [""] + notes
    if not args.skip_sweep:
        out += ["", "(b) SYN20 sweep at 4096^2 x 32, outputs=(), one context, the two alternating; wavefronts/s\n", "| way | wavefronts/s |",
                "|---|---|"]
        out += measure_sweep(4096, 32, args.reps, args.warmup)
    text = (f"Medians (min .. max) of {args.reps} repeats after {args.warmup} warm-up rounds.\n\n" + "\n".join(out) + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
