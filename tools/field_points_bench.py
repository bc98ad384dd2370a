#!/usr/bin/env python3
"""Time several field points per batch and detector images placed at the chief rays (Ariel FGS1, fp64):

  * detector_add placed (paos_detector_add_placed, per-item origins) against the unplaced call, 4096^2 x 32, a 256^2
    detector at pitch = 2 dx of the middle item; the PSFs come from one walked 16 f1 + 16 f2 step;
  * a mixed batch (half f1, half f2) against the single-field batches (all f1, all f2) at 4096^2 x 32 and 1024^2 x 256,
    walked as bench.measure walks a step (lean, keep_psf, no synchronisation inside a step).

Every figure is the minimum over `--rounds` interleaved rounds.  A step's wall time is taken over `--steps` steps between
stream synchronisations; its host time is the time the run_batch calls took to return (planning and enqueueing).  Prints
one JSON document; `--out` also writes it to a file.

    python3 tools/field_points_bench.py --out build/field_points_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="4096x32,1024x256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from paos_amd import _lib
    from paos_amd.detector import Detector
    from paos_amd.parse_config import parse_config
    from paos_amd.run import run_batch

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pup, par, wls, fields, chains = parse_config(os.path.join(root, "data", "lens", "Ariel_FGS-FGS1.ini"))
    last = list(chains[0].keys())[-1]
    out = {"lens": "Ariel_FGS-FGS1", "precision": "fp64", "fields": [[float(f["us"]), float(f["ut"])] for f in fields[:2]]}

    def release(dev, res):
        if res is not None:
            for t in {rec["power_ticket"] for r in res for rec in r.values() if "power_ticket" in rec}:
                dev.norm2_release(t)

    def batch_of(nb, kind):
        wl = [1e-6 * wls[i % len(wls)] for i in range(nb)]
        ch = [chains[i % len(wls)] for i in range(nb)]
        if kind == "mixed":
            fl = [fields[0]] * (nb // 2) + [fields[1]] * (nb - nb // 2)
        else:
            fl = fields[0] if kind == "f1" else fields[1]
        return wl, fl, ch

    for shape in a.shapes.split(","):
        n, nb = (int(x) for x in shape.split("x"))
        dev = _lib.DeviceFields(n, nb)
        try:
            if n == 4096 and nb == 32:
                wl, fl, ch = batch_of(nb, "mixed")
                res = run_batch(pup, wl, n, par["zoom"], fl, ch, outputs=(), dev=dev, keep_psf=True)
                dxs = np.array([r[last]["dx"] for r in res])
                dys = np.array([r[last]["dy"] for r in res])
                w = np.linspace(0.5, 1.5, nb)
                org = np.array([[0.0, 0.0]] * (nb // 2) + [[0.0, 0.3 * dys[nb // 2]]] * (nb - nb // 2))
                mid = nb // 2
                det = Detector(256, 256, 2.0 * dxs[mid], 2.0 * dys[mid], xc=0.3 * dxs[mid], yc=-0.2 * dys[mid])
                dev.detector_begin(det)

                def time_add(origins):
                    dev.detector_add(dxs, dys, w, origins=origins)
                    dev.sync()
                    t0 = time.perf_counter()
                    for _ in range(a.reps):
                        dev.detector_add(dxs, dys, w, origins=origins)
                    dev.sync()
                    return (time.perf_counter() - t0) / a.reps * 1e3

                plain, placed = [], []
                for _ in range(a.rounds):
                    plain.append(time_add(None))
                    placed.append(time_add(org))
                out["add_256_ms_unplaced"] = plain
                out["add_256_ms_placed"] = placed
                out["add_256_placed_overhead_pct"] = 100.0 * (min(placed) / min(plain) - 1.0)

            def time_steps(kind):
                wl, fl, ch = batch_of(nb, kind)
                res = None
                for _ in range(2):
                    release(dev, res)
                    res = run_batch(pup, wl, n, par["zoom"], fl, ch, outputs=(), dev=dev, sync=False, keep_psf=True)
                dev.sync()
                host = 0.0
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    release(dev, res)
                    h0 = time.perf_counter()
                    res = run_batch(pup, wl, n, par["zoom"], fl, ch, outputs=(), dev=dev, sync=False, keep_psf=True)
                    host += time.perf_counter() - h0
                dev.sync()
                release(dev, res)
                wall = (time.perf_counter() - t0) / a.steps * 1e3
                return wall, host / a.steps * 1e3

            rec = {}
            for kind in ("f1", "f2", "mixed"):
                rec[kind] = {"step_ms": [], "host_ms": []}
            for _ in range(a.rounds):
                for kind in ("f1", "f2", "mixed"):
                    wall, host = time_steps(kind)
                    rec[kind]["step_ms"].append(wall)
                    rec[kind]["host_ms"].append(host)
            for kind in rec:
                rec[kind]["us_per_wavefront"] = 1e3 * min(rec[kind]["step_ms"]) / nb
            single = 0.5 * (rec["f1"]["us_per_wavefront"] + rec["f2"]["us_per_wavefront"])
            rec["mixed_vs_single_mean_pct"] = 100.0 * (rec["mixed"]["us_per_wavefront"] / single - 1.0)
            rec["mixed_host_vs_f1_host"] = min(rec["mixed"]["host_ms"]) / min(rec["f1"]["host_ms"])
            out[f"{n}x{nb}"] = rec
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
