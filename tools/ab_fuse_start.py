"""A/B of the fused first-field write on one context, in one process: blocks of walked SYN20 steps (the benchmark's call:
4096^2 complex128, 32 wavefronts per step) alternate between the fused start (paos_start_zernike_box) and the pair of calls
(paos_start_box + paos_zernike_like, what PAOS_FUSE_START=0 runs).  Prints ms per step of every block and the two medians.

    python tools/ab_fuse_start.py [--grid 4096] [--batch 32] [--steps 50] [--blocks 4]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=4)
    args = ap.parse_args()

    import paos_amd.run as prun
    from paos_amd import _lib
    from paos_amd.chains import syn20_chain, syn20_wavelength

    n, nb = args.grid, args.batch
    chains = [syn20_chain() for _ in range(nb)]
    dev = _lib.DeviceFields(n, nb)
    g = 0

    def step():
        nonlocal g
        wls = [syn20_wavelength((g * nb + i) % 512) for i in range(nb)]
        g += 1
        res = prun.run_batch(1.0, wls, n, 4, {"us": 0.0, "ut": 0.0}, chains, outputs=(), dev=dev, sync=False, keep_psf=True)
        for t in {rec["power_ticket"] for r in res for rec in r.values() if "power_ticket" in rec}:
            dev.norm2_release(t)

    try:
        for _ in range(5):
            step()
        dev.sync()
        ms = {True: [], False: []}
        for b in range(2 * args.blocks):
            prun.FUSE_START = b % 2 == 0
            step()  # (the first step behind a switch is not timed)
            dev.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            dev.sync()
            ms[prun.FUSE_START].append((time.perf_counter() - t0) * 1e3 / args.steps)
            print(f"block {b}: {'fused' if prun.FUSE_START else 'pair '} {ms[prun.FUSE_START][-1]:.4f} ms/step", flush=True)
        print(f"median fused {statistics.median(ms[True]):.4f} ms/step, pair {statistics.median(ms[False]):.4f} ms/step "
              f"({nb} wavefronts per step at {n}^2)")
    finally:
        prun.FUSE_START = True
        dev.close()


if __name__ == "__main__":
    main()
