#!/usr/bin/env python3
"""Time the detector pixel-grid kernels (paos_detector_add, include/paos_hip.h) at the headline shape, 4096^2 x 32 fp64:

  * detector_add for a 256^2 detector at pitch = 2 dx of the middle wavelength;
  * detector_add for a 4096^2 detector at pitch = dx of the longest wavelength (it covers the whole grid of every item);
  * a SYN20 walked step as bench.measure issues it, with and without a 256^2 detector behind it.

The PSFs come from one walked SYN20 step.  Each detector_add is timed over `--reps` launches between stream
synchronisations (wall clock on the host, so the 256^2 figure includes the launch cost).  The bytes model of the
full-grid case is printed next to its time: the kept PSF read once, the row-contraction scratch written and read back,
the accumulator read and written once per chunk of items.  Prints one JSON document; `--out` also writes it to a file.

    python3 tools/detector_bench.py --out build/detector_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.3  # MI355X HBM3E, datasheet
SCRATCH_CAP = 512 << 20  # PAOS_DETECTOR_SCRATCH_MIB


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from paos_amd import _lib
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.detector import Detector
    from paos_amd.run import run_batch

    n, nb = a.n, a.batch
    on_axis = {"us": 0.0, "ut": 0.0}
    chains = [syn20_chain() for _ in range(nb)]
    dev = _lib.DeviceFields(n, nb)
    out = {"n": n, "batch": nb, "precision": "fp64"}
    g = [0]

    def release(res):
        if res is not None:
            for t in {rec["power_ticket"] for r in res for rec in r.values() if "power_ticket" in rec}:
                dev.norm2_release(t)

    def step(**kw):
        wls = [syn20_wavelength((g[0] * nb + i) % 512) for i in range(nb)]
        g[0] += 1
        return run_batch(1.0, wls, n, 4, on_axis, chains, outputs=(), dev=dev, sync=False, keep_psf=True, **kw)

    try:
        res = step()
        dxs = np.array([r[20]["dx"] for r in res])
        dys = np.array([r[20]["dy"] for r in res])
        release(res)
        dev.sync()
        w = np.linspace(0.5, 1.5, nb)
        mid = nb // 2

        def time_add(det):
            dev.detector_begin(det)
            dev.detector_add(dxs, dys, w)  # warm-up: scratch allocated, code loaded
            dev.sync()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                dev.detector_add(dxs, dys, w)
            dev.sync()
            return (time.perf_counter() - t0) / a.reps * 1e3

        small = Detector(256, 256, 2.0 * dxs[mid], 2.0 * dys[mid], xc=0.3 * dxs[mid], yc=-0.2 * dys[mid])
        out["add_256_ms"] = time_add(small)
        full = Detector(n, n, float(dxs.max()), float(dys.max()))
        out["add_full_ms"] = time_add(full)
        # bytes model of the full-grid case: every item's footprint is the whole grid (the detector is as wide as the
        # widest item's grid), so rows = n for all of them
        psf_bytes = nb * n * n * 8
        scratch_bytes = 2 * nb * n * full.nx * 8  # row contraction written, read back by the column contraction
        per_item = n * full.nx * 8
        chunks = -(-nb // max(1, SCRATCH_CAP // per_item))
        image_bytes = 2 * chunks * full.nx * full.ny * 8
        moved = psf_bytes + scratch_bytes + image_bytes
        out["add_full_bytes_model"] = moved
        out["add_full_floor_bytes"] = psf_bytes
        out["add_full_floor_ms"] = psf_bytes / (HBM_TBS * 1e12) * 1e3
        out["add_full_effective_TBs"] = moved / (out["add_full_ms"] * 1e-3) / 1e12

        # the walked step with and without the detector (bench.measure's issue pattern), interleaved in blocks
        def time_steps(with_det):
            res = None
            for _ in range(2):
                release(res)
                res = step(**(dict(detector=small, detector_weights=w) if with_det else {}))
            dev.sync()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                release(res)
                res = step(**(dict(detector=small, detector_weights=w) if with_det else {}))
            dev.sync()
            release(res)
            return (time.perf_counter() - t0) / a.steps * 1e3

        plain, det = [], []
        for _ in range(3):
            plain.append(time_steps(False))
            det.append(time_steps(True))
        out["step_ms_without"] = plain
        out["step_ms_with_256"] = det
        out["step_overhead_pct"] = 100.0 * (min(det) / min(plain) - 1.0)
    finally:
        dev.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
