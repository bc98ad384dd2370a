"""The starts of tests/test_gpu_start_partials.py and the call they go through, shared by the test and by the fresh process
it starts for PAOS_START_POWER_MEMO=0 (read once per process)."""
import hashlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NB = 1024, 3  # the smallest grid of the production pass kernels, batch 3


def starts():
    """{name: (constant, aperture blocks, stop flags, row windows, column windows)}.  'first': one start group (three items,
    one aperture); each of the others changes ONE thing the kept sums depend on.  'two groups': item 2 has an aperture and
    windows of its own, so two items lead a sum (lead = 1, 0, 1)."""
    from paos_amd.aperture import EllipticalAperture

    h = N // 2

    def ap(a, b):
        return EllipticalAperture((N / 2, N / 2), a, b, 0.0).block(obscuration=False)

    def box(half):
        return [[h - half, h + half + 1]] * NB

    big, small = ap(120.0, 120.0), ap(90.5, 70.25)
    first = (1.0, [big] * NB, [1.0] * NB, box(123), box(123))
    return {
        "first": first,
        "rows": (1.0, [big] * NB, [1.0] * NB, box(110), box(123)),          # the window cuts the disk: another power
        "cols": (1.0, [big] * NB, [1.0] * NB, box(110), box(97)),
        # [h - 98, h + 99) rounds outward to the same whole blocks of four columns as [h - 97, h + 98): found again, rightly
        "cols that round alike": (1.0, [big] * NB, [1.0] * NB, box(110), [[h - 98, h + 99]] * NB),
        "aperture": (1.0, [small] * NB, [1.0] * NB, box(110), box(97)),
        "two groups": (1.0, [big, big, small], [1.0] * NB, box(123)[:2] + [[h - 73, h + 74]], box(123)[:2] + [[h - 93, h + 94]]),
        "flags": (1.0, [big, big, small], [1.0, 0.0, 1.0], box(123)[:2] + [[h - 73, h + 74]], box(123)[:2] + [[h - 93, h + 94]]),
        "constant": (0.5 + 0.25j, [big, big, small], [1.0, 0.0, 1.0], box(123)[:2] + [[h - 73, h + 74]], box(123)[:2] + [[h - 93, h + 94]]),
    }


# the order on the one context: the same start twice, then one change at a time, then the first again
SEQUENCE = ("first", "first", "rows", "cols", "cols that round alike", "aperture", "two groups", "flags", "constant", "first")


def zernike_args():
    """One wfe map for items 0 and 1 (two wavelengths), another for item 2."""
    from paos_amd.run import _Plans, _zernike_tables, zernike_tables

    m, nn, norm = zernike_tables(15, "standard", True)
    rng = np.random.default_rng(17)
    c0, c2 = rng.normal(0.0, 30e-9, 15), rng.normal(0.0, 30e-9, 15)

    def zplan(coef, wl):
        return {"aperture": None, "stop": False, "phase_map": None,
                "zernike": dict(m=m, n=nn, norm=norm, Z=coef, dx=1.0 / 240.0, dy=1.0 / 240.0, radius=0.5, wl=wl, origin="x", pupil=None)}

    plans = _Plans([zplan(c0, 1.0e-6), zplan(c0, 1.3e-6), zplan(c2, 1.0e-6)])
    zs, nmax, kdim, table, build = _zernike_tables(plans)
    return nmax, kdim, table, build([z["Z"] for z in zs])


def fused_start(dev, start, zargs):
    """paos_start_zernike_box with a power ticket on a field full of NaN: ([field per item], powers)."""
    from paos_amd import _lib

    value, blocks, stops, rows, cols = start
    for i in range(NB):
        dev.upload(i, np.full((N, N), complex(np.nan, np.nan)))
    ticket = dev.start_zernike(value, _lib.SHAPE_ELLIPSE, blocks, stops, rows, cols, *zargs, power=True)
    power = np.array(dev.norm2_fetch(ticket))
    return [dev.download(i, _lib.WHAT_FIELD) for i in range(NB)], power


def digest(result):
    """Every NaN counts as the same NaN: the pixels outside the box, which no call has written."""
    fields, power = result

    def canon(v):
        a = np.ascontiguousarray(v).view(np.float64)
        return np.where(np.isnan(a), np.nan, a).tobytes()

    return {"fields": [hashlib.sha256(canon(f)).hexdigest() for f in fields], "power": [float(p).hex() for p in power]}


def switched_worker(out, switch):
    """In a fresh process, with ``switch`` (read once per process) at 0: the first start, twice on one context.  Puts
    ("ok", [digests, digests]) or ("fail", message) on ``out``."""
    try:
        os.environ[switch] = "0"
        from paos_amd import _lib

        dev = _lib.DeviceFields(N, NB)
        try:
            zargs = zernike_args()
            out.put(("ok", [digest(fused_start(dev, starts()["first"], zargs)) for _ in range(2)]))
        finally:
            dev.close()
    except Exception as exc:  # noqa: BLE001 -- the parent reports it
        out.put(("fail", repr(exc)))
