#!/usr/bin/env python3
"""Which kernels a library launches, case by case -- two libraries that launch the same kernels in the same order give equal lists.

  python tools/launch_names.py run GRID PRECISION
      one lean walked SYN20 sweep step (its last pass stores the PSFs) and one full run that saves a surface (the last pass
      sums the power of the field it stores), four wavefronts each.  Run it under a kernel trace, once per library
      (PAOS_LIB selects one) and case; PAOS_SEPARABLE / PAOS_LINE_TABLES / PAOS_FUSE_PAIRS / PAOS_CENTRAL_HALF = 0 send it down
      the operator-by-operator, evaluating, unfused and ordinary-build arms.  With PAOS_DUMP_PASSES=1 stderr names the build
      of every pass launch (FrugalBuild).
  python tools/launch_names.py names TRACE.csv
      the kernel names of a rocprofv3 --kernel-trace CSV in the order in which they started, one per line."""
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(n, precision):
    from paos_amd import _lib
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.run import run_batch

    wls = [syn20_wavelength(k) for k in range(4)]
    chains = [syn20_chain() for _ in wls]
    field = {"us": 0.0, "ut": 0.0}
    dev = _lib.DeviceFields(n, len(wls), precision)
    try:
        run_batch(1.0, wls, n, 4, field, chains, precision=precision, outputs=(), dev=dev, keep_psf=True)
        dev.sync()
        print(f"lean step done: {n}^2 {precision}", flush=True)
        res = run_batch(1.0, wls, n, 4, field, chains, precision=precision, outputs=("psf",), dev=dev)
        dev.sync()
        print(f"full run done: {n}^2 {precision}, surfaces saved: {sorted(res[0])}", flush=True)
    finally:
        dev.close()


def names(path):
    with open(path, newline="") as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        print(r["Kernel_Name"])


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "run":
        run(int(sys.argv[2]), sys.argv[3])
    elif len(sys.argv) == 3 and sys.argv[1] == "names":
        names(sys.argv[2])
    else:
        sys.exit(__doc__)
