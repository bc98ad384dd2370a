#!/usr/bin/env python3
"""Time a zoomed PSF window (paos_zoom_compute, include/paos_hip.h) at the headline shape: 4096^2 x 32 complex128,
M = 256, s = 4.

  1. one `zoom_compute` (both contractions), and the TFLOP/s it reaches on 4 N N M + 4 N M M flops per item;
  2. one `paos_focus_plane` on the same context in the same run -- the nearest existing product;
  3. the host route for ONE item: download `wfo` and contract it with NumPy (`Wy @ u @ Wx.T`, the weights already made).

1 and 2 are timed with HIP events on the context's stream, alternating, `--reps` repeats after a warm-up; medians and
the spread (quartiles, min, max) are reported.  3 is timed with the host clock.  The fields are the last-surface fields
of one ordinary SYN20 walk of the batch.  Progress goes to stderr; writes a Markdown record (`--out`) and prints it.

    python3 tools/zoom_bench.py --out build/zoom_bench.md
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from focus_bench import EventTimer, fmt, hip_runtime, spread  # noqa: E402


def weight_matrix(lib, n, m, s, c):
    """The dense (m, n) weights of one axis from the library's own phase table (paos_zoom_weights)."""
    from paos_amd import _lib

    ci = int(np.floor(c))
    tab = np.empty((s, n))
    carry = np.empty(s, dtype=np.intc)
    rc = lib.paos_zoom_weights(n, s, float(c - ci), tab.ctypes.data_as(_lib._dbl_p),
                               carry.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    if rc != 0:
        raise RuntimeError("paos_zoom_weights failed")
    j = np.arange(n)
    out = np.empty((m, n))
    for q in range(m):
        a, b = divmod(q - m // 2, s)
        out[q] = tab[b, (ci + a + int(carry[b]) - j) % n]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--oversample", type=int, default=4)
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", default="fp64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")

    from paos_amd import _lib
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.run import run_batch

    t_start = time.perf_counter()

    def progress(what):
        print(f"[{time.perf_counter() - t_start:7.1f} s] {what}", file=sys.stderr, flush=True)

    n, nb, m, s = a.n, a.batch, a.size, a.oversample
    dev = _lib.DeviceFields(n, nb, a.precision)
    timer = EventTimer(hip_runtime(), dev.stream)
    lines = []
    try:
        progress("context created")
        wls = [syn20_wavelength((7 * i) % 512) for i in range(nb)]
        # the ordinary walk stores the field of the last surface (focus_planes = the nominal plane alone)
        res = run_batch(1.0, wls, n, 4, {"us": 0.0, "ut": 0.0}, [syn20_chain() for _ in range(nb)], outputs=(), dev=dev,
                        focus_planes=[0.0], precision=a.precision)
        dev.sync()
        progress("walked")
        dxs, dys = [r[20]["dx"] for r in res], [r[20]["dy"] for r in res]
        dz = 0.25 * min(n * min(dx, dy) ** 2 / wl for dx, dy, wl in zip(dxs, dys, wls))
        blocks = np.ascontiguousarray([[1.0, 1.0 / (n * dxs[i]), 1.0 / (n * dys[i]), np.pi * wls[i] * dz, -1.0]
                                       for i in range(nb)])
        # (a focus plane overwrites the field; the planes of a planar wavefront stay PSF-like, so the windows timed
        # afterwards see fields of the same kind)
        dev.focus_begin()
        for _ in range(a.warmup):
            dev.zoom_compute(m, s)
            dev.focus_plane(blocks)
        dev.sync()
        progress("warm")
        t_zoom, t_plane = [], []
        for _ in range(a.reps):  # alternating, same context, same run
            t_zoom.append(timer.ms(lambda: dev.zoom_compute(m, s)))
            t_plane.append(timer.ms(lambda: dev.focus_plane(blocks)))
        dev.focus_end()
        progress("timed")
        s_zoom, s_plane = spread(t_zoom), spread(t_plane)
        flops = nb * (4.0 * n * n * m + 4.0 * n * m * m)
        tflops = flops / (s_zoom["median"] * 1e-3) / 1e12

        # the host route for one item (the weights are made beforehand and not timed)
        wy = weight_matrix(dev._lib, n, m, s, n // 2)
        wx = weight_matrix(dev._lib, n, m, s, n // 2)
        t_down, t_host = [], []
        for _ in range(5):
            t0 = time.perf_counter()
            u = dev.download(0)
            t1 = time.perf_counter()
            tr, ti = wy @ np.ascontiguousarray(u.real), wy @ np.ascontiguousarray(u.imag)  # (contiguous: the BLAS path)
            wr, wi = tr @ wx.T, ti @ wx.T
            host_psf = wr * wr + wi * wi
            t2 = time.perf_counter()
            t_down.append((t1 - t0) * 1e3)
            t_host.append((t2 - t1) * 1e3)
            del u
            progress("host route")
        dev.zoom_compute(m, s)
        got = dev.zoom_fetch(0, "psf")
        err = float(np.max(np.abs(got - host_psf)) / np.max(host_psf))
        s_down, s_host = spread(t_down), spread(t_host)
        per_item = s_zoom["median"] / nb
        host_item = s_down["median"] + s_host["median"]
        lines += [
            "# Zoomed PSF windows: time per `zoom_compute`",
            "",
            f"`tools/zoom_bench.py`: {n}^2 x {nb} {a.precision}, M = {m}, s = {s}, SYN20 last-surface fields, {dev.build_info()}.",
            f"1 and 2: HIP events on the context's stream, alternating in one run, after {a.warmup} warm-up rounds.  3: host "
            f"clock, OMP_NUM_THREADS = {os.environ.get('OMP_NUM_THREADS', 'unset')}.",
            "",
            "| what | time |",
            "|---|---|",
            f"| 1. `zoom_compute`, {nb} items (stage Y + stage X) | {fmt(s_zoom)} |",
            f"| 2. `paos_focus_plane`, same context, same run | {fmt(s_plane)} |",
            f"| 3a. host route, one item: download `wfo` ({16 * n * n / 2**20:.0f} MiB) | {fmt(s_down)} |",
            f"| 3b. host route, one item: `Wy @ u @ Wx.T` in NumPy | {fmt(s_host)} |",
            "",
            f"`zoom_compute`: {per_item:.3f} ms per item, {tflops:.1f} TFLOP/s on {flops / 1e9:.1f} GFLOP "
            f"(4 N N M + 4 N M M per item).",
            f"Host route: {host_item:.1f} ms per item -- the device route is "
            f"{'faster' if per_item < host_item else 'NOT faster'}, x{host_item / per_item:.0f}.",
            f"Device window against the NumPy contraction of the downloaded field: {err:.2e} of the peak.",
        ]
    finally:
        timer.close()
        dev.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
