#!/usr/bin/env python3
"""Time a through-focus stack (paos_focus_*, include/paos_hip.h) at the headline shape: SYN20, 4096^2 x 32 complex128,
K = 9 planes.

  1. one plane: focus_plane + psf_keep;
  2. paos_ptp + psf_keep on the same context in the same run -- what a caller without the fan-out composes per plane,
     once a copy that restores the last-surface field is added (the in-place copy yardstick is reported next to it);
  3. one nominal walk: the lean one bench.py times, and the ordinary one a stack rides on;
  and the K-plane stack (focus_begin + K planes) against K full walks.

1 and 2 are timed with HIP events on the context's stream, alternating, `--reps` repeats after a warm-up; medians and
the spread (quartiles, min, max) are reported.  The walks are timed with the host clock around work that ends in a
stream synchronisation.  Writes a Markdown record (`--out`) and prints it.

    python3 tools/focus_bench.py --out build/focus_bench.md
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def hip_runtime():
    """The HIP runtime the library is linked against, as this process has it loaded."""
    with open("/proc/self/maps") as fh:
        paths = sorted({line.split()[-1] for line in fh if "libamdhip64" in line})
    if not paths:
        raise RuntimeError("libamdhip64 is not loaded (load the library first)")
    hip = ctypes.CDLL(paths[0])
    hip.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
    hip.hipEventDestroy.argtypes = [ctypes.c_void_p]
    return hip


class EventTimer:
    def __init__(self, hip, stream):
        self.hip, self.stream = hip, stream
        self.a, self.b = ctypes.c_void_p(), ctypes.c_void_p()
        for e in (self.a, self.b):
            if hip.hipEventCreate(ctypes.byref(e)) != 0:
                raise RuntimeError("hipEventCreate failed")

    def ms(self, work):
        """Device time of what ``work()`` enqueues on the stream."""
        hip = self.hip
        if hip.hipEventRecord(self.a, self.stream) != 0:
            raise RuntimeError("hipEventRecord failed")
        work()
        if hip.hipEventRecord(self.b, self.stream) != 0 or hip.hipEventSynchronize(self.b) != 0:
            raise RuntimeError("hipEventRecord / hipEventSynchronize failed")
        out = ctypes.c_float(0.0)
        if hip.hipEventElapsedTime(ctypes.byref(out), self.a, self.b) != 0:
            raise RuntimeError("hipEventElapsedTime failed")
        return float(out.value)

    def close(self):
        for e in (self.a, self.b):
            self.hip.hipEventDestroy(e)


def spread(v):
    v = np.sort(np.asarray(v, dtype=np.float64))
    return {"median": float(np.median(v)), "q1": float(np.percentile(v, 25)), "q3": float(np.percentile(v, 75)),
            "min": float(v[0]), "max": float(v[-1]), "n": int(v.size)}


def fmt(s):
    return f"{s['median']:.3f} ms (quartiles {s['q1']:.3f} .. {s['q3']:.3f}, range {s['min']:.3f} .. {s['max']:.3f}, n = {s['n']})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--planes", type=int, default=9)
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--walks", type=int, default=6)
    ap.add_argument("--precision", default="fp64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")

    from paos_amd import _lib
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.run import run_batch

    n, nb, kp = a.n, a.batch, a.planes
    on_axis = {"us": 0.0, "ut": 0.0}
    chains = [syn20_chain() for _ in range(nb)]
    wls = [syn20_wavelength((7 * i) % 512) for i in range(nb)]
    dev = _lib.DeviceFields(n, nb, a.precision)
    hip = hip_runtime()
    timer = EventTimer(hip, dev.stream)
    lines = []
    try:
        def lean_walk():
            res = run_batch(1.0, wls, n, 4, on_axis, chains, outputs=(), dev=dev, sync=False, keep_psf=True,
                            precision=a.precision)
            for t in {id(rec["power_ticket"]): rec["power_ticket"] for r in res for rec in r.values()
                      if "power_ticket" in rec}.values():
                t.release()
            dev.sync()
            return res

        def ordinary_walk():
            # what a stack rides on: the field of the last surface is stored (focus_planes = the nominal plane alone)
            res = run_batch(1.0, wls, n, 4, on_axis, chains, outputs=(), dev=dev, keep_psf=True, focus_planes=[0.0],
                            precision=a.precision)
            dev.sync()
            return res

        def wall(fn, count):
            out = []
            for _ in range(count):
                t0 = time.perf_counter()
                fn()
                out.append((time.perf_counter() - t0) * 1e3)
            return out

        lean_walk()
        ordinary_walk()
        t_lean, t_ord = [], []
        for _ in range(a.walks):  # alternating
            t_lean += wall(lean_walk, 1)
            t_ord += wall(ordinary_walk, 1)
        res = ordinary_walk()  # the field now holds the last surface
        rec = res[0][20]
        dxs = [r[20]["dx"] for r in res]
        dys = [r[20]["dy"] for r in res]
        zr_free = min(n * min(dx, dy) ** 2 / wl for dx, dy, wl in zip(dxs, dys, wls))  # the sampling limit N d^2 / wl
        step = min(2.0e-4, 0.9 * zr_free) / (kp // 2 + 1)
        dzs = [step * (k - kp // 2) for k in range(kp)]
        dzs = [dz if dz != 0.0 else 0.5 * step for dz in dzs]  # every timed plane is a computed one

        def blocks(dz):
            return [[1.0, 1.0 / (n * dxs[i]), 1.0 / (n * dys[i]), np.pi * wls[i] * dz, -1.0] for i in range(nb)]

        all_blocks = [np.ascontiguousarray(blocks(dz)) for dz in dzs]

        def plane(k):
            dev.focus_plane(all_blocks[k])
            dev.psf_keep()

        def ptp(k):
            dev.ptp(all_blocks[k])
            dev.psf_keep()

        dev.focus_begin()
        for k in range(a.warmup):
            plane(k % kp)
            ptp(k % kp)
        dev.sync()
        t_plane, t_ptp = [], []
        for r in range(a.reps):  # alternating, same context, same run
            k = r % kp
            t_plane.append(timer.ms(lambda: plane(k)))
            t_ptp.append(timer.ms(lambda: ptp(k)))
        dev.focus_end()
        copy_ms, copy_bytes = dev.copy_yardstick(10)

        # the K-plane stack as run_batch issues it (begin + K planes + psf_keep each), on the last-surface field
        ordinary_walk()
        t_stack = []
        for r in range(max(5, a.reps // 4)):
            def stack():
                dev.focus_begin()
                for k in range(kp):
                    plane(k)
            t_stack.append(timer.ms(stack))
            dev.focus_end()

        s_plane, s_ptp, s_stack = spread(t_plane), spread(t_ptp), spread(t_stack)
        s_lean, s_ord = spread(t_lean), spread(t_ord)
        noise = max(s_plane["q3"] - s_plane["q1"], s_ptp["q3"] - s_ptp["q1"])
        diff = s_ptp["median"] - s_plane["median"]
        lines += [
            "# Through-focus stack: time per plane",
            "",
            f"`tools/focus_bench.py`: SYN20, {n}^2 x {nb} {a.precision}, K = {kp} planes, {dev.build_info()}.",
            "Planes and ptp: HIP events on the context's stream, alternating in one run, after "
            f"{a.warmup} warm-up rounds.  Walks: host clock around a run that ends in a stream synchronisation, alternating.",
            "",
            "| what | time |",
            "|---|---|",
            f"| 1. one plane: `focus_plane` + `psf_keep` | {fmt(s_plane)} |",
            f"| 2. `paos_ptp` + `psf_keep`, same context, same run | {fmt(s_ptp)} |",
            f"| (the copy that restores the field before each `paos_ptp`, not included in 2: in-place copy yardstick, "
            f"{copy_bytes / 2**30:.2f} GiB) | {copy_ms:.3f} ms |",
            f"| 3a. one nominal walk, lean (what `bench.py` times; the field is not stored) | {fmt(s_lean)} |",
            f"| 3b. one nominal walk, ordinary (stores the last-surface field; what a stack rides on) | {fmt(s_ord)} |",
            f"| K-plane stack: `focus_begin` + {kp} x (`focus_plane` + `psf_keep`) | {fmt(s_stack)} |",
            f"| K full walks (K x 3b) | {kp * s_ord['median']:.1f} ms |",
            "",
            f"A plane is {'below' if diff > 0 else 'NOT below'} `paos_ptp` + `psf_keep`: {diff:+.3f} ms "
            f"({100.0 * diff / s_ptp['median']:+.1f} % of 2), against a run-to-run spread (largest interquartile range of "
            f"the two) of {noise:.3f} ms{'' if diff > noise else ' -- NOT more than the spread'}.",
            f"One walk plus a {kp}-plane stack: {s_ord['median'] + s_stack['median']:.1f} ms, against {kp} walks "
            f"{kp * s_ord['median']:.1f} ms: x{kp * s_ord['median'] / (s_ord['median'] + s_stack['median']):.2f}.",
            f"Defocus values timed: {', '.join(f'{dz:+.2e}' for dz in dzs)} m (sampling limit N d^2 / wl of the batch: "
            f"{zr_free:.2e} m); dx = {rec['dx']:.3e} m at the last surface.",
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
