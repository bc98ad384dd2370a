#!/usr/bin/env python3
"""Time the wavefront fits (paos_wavefront_fit / paos_wavefront_fetch, include/paos_hip.h), fp64:

  (a) one fit plus fetch with K = 36 at 4096^2 x 32 and 1024^2 x 256, on a disk of a quarter of the grid's width in
      radius, for both weightings -- the four kernels as the library's launch timer reports them (HIP events: moments,
      their final stage, the Gram launch, its final stage) and the whole call pair by the host's clock, the copy and its
      synchronisation included -- beside what the same answer costs without the feature: ``dev.download`` of an item's
      complex field plus the NumPy fit of tests/wavefront_np.py, timed on one item and multiplied by the batch;
      for the Gram launch the multiply-adds and the LDS bytes it needs (from the pixel count the fit returns) over its time,
      against the chip's fp64 vector peak and LDS bandwidth: which of the two bounds it;
  (b) wavefronts/s of a SYN20 sweep at 4096^2 x 32 with ``outputs=(), wavefront=WavefrontFit(36, 0.5, surfaces=(2,))`` (the
      Zernike surface, saved for the purpose) against the same sweep without it (which then runs on the lean walk) and against
      ``metrics_radii_px``, the existing keyword that also keeps the sweep on the ordinary walk; the three alternate on
      one context.

`--reps` repeats after a warm-up; medians and the spread (min .. max).  Writes a Markdown record (`--out`) and prints it.

    python3 tools/wavefront_bench.py --out build/wavefront_bench.md
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))  # the NumPy fit a user would write: tests/wavefront_np.py

SHAPES = ((4096, 32), (1024, 256))
TERMS = 36
FIELD = {"us": 0.0, "ut": 0.0}
WL = 1.0e-6
# MI355X: 256 CUs x 64 fp64 multiply-adds per clock at 2.4 GHz ("Zoomed windows": 78.6 TFLOP/s), and
# 256 B of LDS reads per clock and CU
PEAK_FLOPS = 78.6e12
PEAK_LDS = 256 * 256 * 2.4e9


def spread(values, per=1.0):
    return f"{statistics.median(values) / per:.3f} ({min(values) / per:.3f} .. {max(values) / per:.3f})"


def beam(n, radius_px, seed):
    rng = np.random.default_rng(seed)
    j = (np.arange(n) - n // 2) / float(radius_px)
    x, y = j[None, :], j[:, None]
    phase = 0.7 * x - 0.5 * y + 0.8 * (x * x - y * y) + 0.05 * rng.standard_normal((n, n))
    return (0.3 + np.exp(-(x * x + y * y))) * np.exp(1j * phase)


def measure_calls(n, batch, reps, warmup):
    import wavefront_np as wnp
    from paos_amd import _lib
    from paos_amd.wavefront import WavefrontFit, fit_from_sums
    from paos_amd.zernike import Zernike

    dx, radius_px = 1.0e-4, n / 4 + 0.3
    fit = WavefrontFit(TERMS, radius_px * dx)
    dev = _lib.DeviceFields(n, batch, "fp64")
    out = []
    try:
        u = beam(n, radius_px, n + batch)
        for i in range(batch):
            dev.upload(i, u)
        m, nn = Zernike.j2mn(TERMS, "standard")
        nmax, kdim, table, blocks, poly = fit.request([dx] * batch, [dx] * batch, [WL] * batch)
        # without the feature: every item's field to the host, and the fit there
        host = []
        for rep in range(1 if n >= 2048 else 2):  # (tens of seconds per item at 4096^2)
            t0 = time.perf_counter()
            got = dev.download(0)
            t1 = time.perf_counter()
            want = fit_from_sums(*wnp.fit_sums_np(got, m, nn, True, dx, dx, radius_px * dx), TERMS, WL)
            host.append((1.0e3 * (t1 - t0), 1.0e3 * (time.perf_counter() - t1)))
        for weight in (_lib.WF_UNIFORM, _lib.WF_INTENSITY):
            launches, pair = [], []
            for rep in range(warmup + reps):
                dev.profile_begin(_lib.KERNEL_PASS_ANY)
                dev.wavefront_fit(nmax, kdim, table, blocks, poly, weight=weight)
                ms, _ = dev.profile_end_launches()
                summary, sums = dev.wavefront_fetch()
                dev.sync()
                t0 = time.perf_counter()
                dev.wavefront_fit(nmax, kdim, table, blocks, poly, weight=weight)
                dev.wavefront_fetch()
                t1 = time.perf_counter()
                assert ms.size == 4
                if rep >= warmup:
                    launches.append(ms)
                    pair.append(1.0e3 * (t1 - t0))
            cols = list(zip(*launches))
            if weight == _lib.WF_UNIFORM:  # the two routes agree (the device's coefficients against the host's)
                dev_fit = fit_from_sums(summary[0], sums[0], TERMS, WL)
                assert np.max(np.abs(dev_fit["wf_coeff"] - want["wf_coeff"])) <= 1e-12 * np.max(np.abs(want["wf_coeff"]))
            # the Gram launch: chunks of 128 pixels that hold a pixel of the disk, (K + 1)(K + 2) / 2 pairs each, one
            # multiply-add (two with weights) and two (three) 8-byte LDS reads per pair and pixel
            npairs = (TERMS + 1) * (TERMS + 2) // 2
            chunks = summary[:, 0].sum() / 128.0 * 1.08  # (pixels of the disk; the chunks at its rim are partly outside: +8 %)
            weighted = weight == _lib.WF_INTENSITY
            flops = chunks * 128 * npairs * (3 if weighted else 2)
            lds = chunks * 128 * npairs * 8 * (3 if weighted else 2)
            t_gram = statistics.median(cols[2]) * 1.0e-3
            host_ms = batch * (statistics.median(h[0] for h in host) + statistics.median(h[1] for h in host))
            out.append(f"| {n}^2 x {batch} | {'intensity' if weighted else 'uniform'} | {spread(pair)} | {spread(cols[0])} | {spread(cols[1])} | "
                       f"{spread(cols[2])} | {spread(cols[3])} | {flops / t_gram / 1e12:.1f} ({flops / t_gram / PEAK_FLOPS:.2f}) | "
                       f"{lds / t_gram / 1e12:.1f} ({lds / t_gram / PEAK_LDS:.2f}) | "
                       f"{batch} x ({statistics.median(h[0] for h in host):.1f} + {statistics.median(h[1] for h in host):.0f}) = {host_ms:.0f} | "
                       f"{host_ms / statistics.median(pair):.0f} |")
            print(out[-1], flush=True)
    finally:
        dev.close()
    return out


def measure_sweep(n, batch, reps, warmup):
    from paos_amd import WavefrontFit, _lib
    from paos_amd.chains import syn20_chain, syn20_coefficients, syn20_wavelength
    from paos_amd.run import run_batch

    wls = [syn20_wavelength((511 * k) // max(1, batch - 1)) for k in range(batch)]
    chains = [syn20_chain(syn20_coefficients(sigma=8.0e-9)) for _ in wls]
    for chain in chains:
        chain[2]["save"] = True
    radii = [float(r) for r in np.arange(1, 17) * 16.0]
    ways = {"plain (lean walk)": {}, f"wavefront=WavefrontFit({TERMS}, 0.5, surfaces=(2,))": {"wavefront": WavefrontFit(TERMS, 0.5, surfaces=(2,))},
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
    ap.add_argument("--out", default=os.path.join("build", "wavefront_bench.md"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-sweep", action="store_true")
    ap.add_argument("--shapes", default=None, help="N:B,N:B instead of 4096:32,1024:256 (a rehearsal at small sizes)")
    args = ap.parse_args()
    shapes = SHAPES if args.shapes is None else tuple(tuple(int(v) for v in s.split(":")) for s in args.shapes.split(","))
    out = [f"(a) one paos_wavefront_fit + paos_wavefront_fetch, K = {TERMS}, disk radius N/4, fp64; milliseconds; the Gram launch's "
           "rates as TFLOP/s and LDS TB/s with their share of the chip's peak in brackets\n",
           "| shape | weights | fit + fetch, host clock | moments | their final | Gram | its final | Gram TFLOP/s | Gram LDS TB/s | "
           "download + NumPy fit, one item x batch | ratio |",
           "|---|---|---|---|---|---|---|---|---|---|---|"]
    for n, batch in shapes:
        out += measure_calls(n, batch, args.reps, args.warmup)
    if not args.skip_sweep:
        n, batch = shapes[0]
        out += ["", f"(b) SYN20 sweep at {n}^2 x {batch}, outputs=(), the Zernike surface saved, one context, the three alternating; wavefronts/s\n",
                "| way | wavefronts/s |", "|---|---|"]
        out += measure_sweep(n, batch, args.reps, args.warmup)
    text = (f"Medians (min .. max) of {args.reps} repeats after {args.warmup} warm-up rounds.\n\n" + "\n".join(out) + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
