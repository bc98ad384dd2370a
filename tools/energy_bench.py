#!/usr/bin/env python3
"""Time the energy profiles of the kept PSFs (paos_ee_compute / paos_ee_fetch, include/paos_hip.h), fp64:

  (a) one paos_ee_compute plus paos_ee_fetch at 4096^2 x 32 and 2048^2 x 64 for 64, 256 and 1024 rings of one pixel about
      the centroid -- the four launches as the library's launch timer reports them (the sweep that sums, the centre, the
      binning, the scan) and the whole call pair by the host's clock, the copy and its synchronisation included -- beside
      one paos_psf_metrics call with 16 radii on the same context: the existing code doing the comparable single sweep
      (over the field, about the grid centre);
  (b) wavefronts/s of a SYN20 sweep at 4096^2 x 32 with ``outputs=(), psf_energy=EnergyProfile(256, ...)`` against the
      only other way to an encircled energy, ``outputs=(), metrics_radii_px=[16 radii]``, and against the plain lean
      sweep; the three alternate on one context.

`--reps` repeats after a warm-up; medians and the spread (min .. max).  Writes a Markdown record (`--out`) and prints it.

    python3 tools/energy_bench.py --out build/energy_bench.md
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((4096, 32), (2048, 64))
BINS = (64, 256, 1024)
FIELD = {"us": 0.0, "ut": 0.0}


def spread(values, per=1.0):
    return f"{statistics.median(values) / per:.3f} ({min(values) / per:.3f} .. {max(values) / per:.3f})"


def measure_calls(n, batch, reps, warmup):
    from paos_amd import _lib

    dev = _lib.DeviceFields(n, batch, "fp64")
    out = []
    try:
        rng = np.random.default_rng(n + batch)
        j = np.arange(n, dtype=np.float64)
        env = np.exp(-((j - n / 2 - 3.3) ** 2) / (4.0 * (n / 16.0) ** 2))
        dev.fill(0.0)
        for i in range(min(batch, 4)):  # (a few speckled blobs; the other items stay zero: the sweep reads them all the same)
            dev.upload(i, (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) * env[:, None] * env[None, :])
        dev.psf_keep()
        radii = np.arange(1, 17, dtype=np.float64) * (n / 64.0)
        for bins in BINS:
            launches, pair, metrics = [], [], []
            for rep in range(warmup + reps):
                dev.profile_begin(_lib.KERNEL_PASS_ANY)
                dev.energy_compute(bins, 1.0, 1.0, _lib.EE_CENTROID)
                ms, _ = dev.profile_end_launches()
                dev.energy_fetch()
                dev.sync()
                t0 = time.perf_counter()
                dev.energy_compute(bins, 1.0, 1.0, _lib.EE_CENTROID)
                dev.energy_fetch()
                t1 = time.perf_counter()
                dev.psf_metrics(radii)
                t2 = time.perf_counter()
                assert ms.size == 4
                if rep >= warmup:
                    launches.append(ms)
                    pair.append(1.0e3 * (t1 - t0))
                    metrics.append(1.0e3 * (t2 - t1))
            cols = list(zip(*launches))
            ratio = statistics.median(pair) / statistics.median(metrics)
            out.append(f"| {n}^2 x {batch} | {bins} | {spread(pair)} | {spread(cols[0])} | {spread(cols[1])} | {spread(cols[2])} | "
                       f"{spread(cols[3])} | {spread(metrics)} | {ratio:.2f} |")
            print(out[-1], flush=True)
    finally:
        dev.close()
    return out


def measure_sweep(n, batch, reps, warmup):
    from paos_amd import EnergyProfile, _lib
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.run import run_batch

    wls = [syn20_wavelength((511 * k) // max(1, batch - 1)) for k in range(batch)]
    chains = [syn20_chain() for _ in wls]
    radii = [float(r) for r in np.arange(1, 17) * 16.0]
    ways = {"lean": {}, "psf_energy, 256 rings": {"psf_energy": EnergyProfile(256, 1.0, unit="px", centre="centroid", fractions=(0.9,))},
            "metrics_radii_px, 16 radii": {"metrics_radii_px": radii}}
    rates = {name: [] for name in ways}
    dev = _lib.DeviceFields(n, batch, "fp64")
    try:
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
    ap.add_argument("--out", default=os.path.join("build", "energy_bench.md"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-sweep", action="store_true")
    args = ap.parse_args()
    out = ["(a) one paos_ee_compute + paos_ee_fetch, rings of one pixel about the centroid, fp64; milliseconds\n",
           "| shape | rings | compute + fetch, host clock | sums | centre | binning | scan | psf_metrics, 16 radii, host clock | ratio |",
           "|---|---|---|---|---|---|---|---|---|"]
    for n, batch in SHAPES:
        out += measure_calls(n, batch, args.reps, args.warmup)
    if not args.skip_sweep:
        out += ["", "(b) SYN20 sweep at 4096^2 x 32, outputs=(), one context, the three alternating; wavefronts/s\n", "| way | wavefronts/s |",
                "|---|---|"]
        out += measure_sweep(4096, 32, args.reps, args.warmup)
    text = (f"Medians (min .. max) of {args.reps} repeats after {args.warmup} warm-up rounds.\n\n" + "\n".join(out) + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
