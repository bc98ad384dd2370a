#!/usr/bin/env python3
"""Time a broadband series sum of the kept PSFs (paos_series_sum_*, include/paos_hip.h), fp64:

  (a) one series_sum_begin + series_sum_add + series_sum_flux at 4096^2 x 32 on a 64 x 64 detector at a pitch of 5 dx,
      T = 256 offsets (Gaussian jitter of one pitch rms), 4 boxes and a pixel response, by the host's clock around the
      three calls (the flux synchronises) -- beside the only way the library offered before: ``series_compute(frames=True)``
      (every frame of every item crosses to the host), ``sum_i w_i F_i`` with NumPy, the response and the box sums on the
      host.  The two alternate;
  (b) wavefronts/s of a 64-wavelength SYN20 sweep at 4096^2, ``batch=32``: ``run_broadband`` beside
      ``run_broadband_series`` with a ``PointingSeries`` (T = 256, 4 boxes); the two alternate;
  (c) the accumulate kernel alone: K adds enqueued back to back and one synchronisation, with the weights of (a) and with
      all weights zero -- the kernel then loads and stores S and skips every item, which is a plain read-modify-write of
      the same buffer by the same launch -- as bytes of S moved per second (2 T ny nx 8 bytes per add), on the detector of
      (a) and on a 1024 x 1024 detector with T = 16 (128 MiB of S: beyond the caches).

`--reps` repeats after a warm-up; medians and the spread (min .. max).  Writes a Markdown record (`--out`) and prints it.

    python3 tools/series_sum_bench.py --out build/series_sum_bench.md
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


def measure_calls(n, batch, nt, reps, warmup, adds):
    from paos_amd import _lib
    from paos_amd.detector import Detector

    dev = _lib.DeviceFields(n, batch, "fp64")
    out, kernel = [], []
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
        w = rng.uniform(0.5, 1.5, batch)
        off = det.pitch_x * rng.standard_normal((nt, 2))
        new, old = [], []
        flux = ref = None
        for rep in range(warmup + reps):
            dev.sync()
            t0 = time.perf_counter()
            dev.series_sum_begin(det, nt)
            dev.series_sum_add(dxs, dxs, w, off)
            flux = dev.series_sum_flux(BOXES, gains)
            t1 = time.perf_counter()
            frames = dev.series_compute(det, dxs, dxs, off, frames=True)  # the parent commit: every frame crosses
            total = np.tensordot(w, frames, axes=(0, 0)) * gains
            ref = np.stack([total[:, n0:n1, m0:m1].sum(axis=(1, 2)) for m0, m1, n0, n1 in BOXES], axis=1)
            t2 = time.perf_counter()
            if rep >= warmup:
                new.append(1.0e3 * (t1 - t0))
                old.append(1.0e3 * (t2 - t1))
        scale = np.max(np.abs(ref))
        assert np.max(np.abs(flux - ref)) <= 1.0e-12 * scale, "the sum and the host fold disagree"
        ratio = statistics.median(old) / statistics.median(new)
        moved = batch * nt * det.nx * det.ny * 8 / 1e6
        out.append(f"| {n}^2 x {batch} | {nt} | {spread(new)} | {spread(old)} | {ratio:.1f} | {moved:.0f} MB |")
        print(out[-1], flush=True)

        # (c) the accumulate kernel alone
        for name, d, frames_c in (("64 x 64, T = %d" % nt, det, nt), ("1024 x 1024, T = 16", Detector(1024, 1024, 0.3 * DX0), 16)):
            o = off if frames_c == nt else d.pitch_x * rng.standard_normal((frames_c, 2))
            nbytes = 2.0 * frames_c * d.nx * d.ny * 8.0
            row = [name, f"{nbytes / 1e6:.0f} MB"]
            for weights in (w, np.zeros(batch)):
                dev.series_sum_begin(d, frames_c)
                times = []
                for rep in range(warmup + reps):
                    dev.sync()
                    t0 = time.perf_counter()
                    for _ in range(adds):
                        dev.series_sum_add(dxs, dxs, weights, o)
                    dev.sync()
                    if rep >= warmup:
                        times.append((time.perf_counter() - t0) / adds)
                row += [spread(times, 1.0e-6), f"{nbytes / statistics.median(times) / 1e9:.1f}"]
            kernel.append("| " + " | ".join(row) + " |")
            print(kernel[-1], flush=True)
    finally:
        dev.close()
    return out, kernel


def measure_sweep(n, batch, count, nt, reps, warmup):
    from paos_amd import PointingSeries
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.detector import Detector, run_broadband, run_broadband_series
    from paos_amd.run import run_batch

    wls = [syn20_wavelength((511 * k) // max(1, count - 1)) for k in range(count)]
    w = np.random.default_rng(2).uniform(0.5, 1.5, count)
    chain = syn20_chain()
    dx = run_batch(1.0, wls[:1], n, 4, FIELD, [chain], outputs=())[0][20]["dx"]
    det = Detector(64, 64, 5.0 * dx)
    off = det.pitch_x * np.random.default_rng(1).standard_normal((nt, 2))
    ways = {"run_broadband (no series)": (run_broadband, {}),
            f"run_broadband_series, PointingSeries(64 x 64 at 5 dx, T = {nt}, 4 boxes)": (run_broadband_series,
                                                                                           {"pointing": PointingSeries(det, off, apertures=BOXES)})}
    rates = {name: [] for name in ways}
    images = {}
    for rep in range(warmup + reps):
        for name, (sweep, kw) in ways.items():
            t0 = time.perf_counter()
            res = sweep(1.0, wls, w, n, 4, FIELD, chain, det, batch=batch, **kw)
            if rep >= warmup:
                rates[name].append(count / (time.perf_counter() - t0))
            images[name] = res["image"]
    a, b = images.values()
    assert np.array_equal(a, b), "the image changed with a series"
    return [f"| {name} | {spread(vals, 1.0)} |" for name, vals in rates.items()]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("build", "series_sum_bench.md"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--wavelengths", type=int, default=64)
    ap.add_argument("--adds", type=int, default=20, help="adds enqueued back to back per timing of the kernel alone")
    ap.add_argument("--skip-sweep", action="store_true")
    args = ap.parse_args()
    out = ["(a) begin + add + flux, 64 x 64 detector at a pitch of 5 dx, 4 boxes, a pixel response, fp64; milliseconds by the host's "
           "clock\n",
           "| shape | T | series_sum begin + add + flux | series_compute(frames=True) + NumPy fold + host sums | old / new | frames the old way copies |",
           "|---|---|---|---|---|---|"]
    rows, kernel = measure_calls(args.n, args.batch, args.frames, args.reps, args.warmup, args.adds)
    out += rows
    out += ["", f"(c) the accumulate kernel alone: {args.adds} adds back to back, one synchronisation; microseconds per add and GB/s of S "
            "(2 T ny nx 8 bytes per add)\n",
            "| detector | bytes of S per add | add, us | GB/s | add with all weights 0 (plain read-modify-write), us | GB/s |", "|---|---|---|---|---|---|"]
    out += kernel
    if not args.skip_sweep:
        out += ["", f"(b) run_broadband and run_broadband_series, SYN20, {args.wavelengths} wavelengths at {args.n}^2, batch={args.batch}, the two alternating; "
                "wavefronts/s (the context is made inside the call)\n", "| way | wavefronts/s |", "|---|---|"]
        out += measure_sweep(args.n, args.batch, args.wavelengths, args.frames, args.reps, args.warmup)
    text = (f"Medians (min .. max) of {args.reps} repeats after {args.warmup} warm-up rounds.\n\n" + "\n".join(out) + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
