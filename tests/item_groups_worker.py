"""The batch of tests/test_gpu_item_groups.py and the calls it goes through, shared by the test and by the fresh processes the
test starts for the switches the library reads once per process (PAOS_SHARE_START, PAOS_SHARE_WFE)."""
import hashlib

import numpy as np

N = 64  # the smallest grid: which items share cannot depend on the grid size
VALUE = 1.0 + 0.5j


def scenario():
    """Six items.  Aperture records: A for items 0, 2, 4, B for 1 and 3, C for 5; the stop flags differ inside A and B, so the
    groups of identical start fields are {0, 2}, {4}, {1}, {3}, {5}.  Zernike records: map P for items 0 and 2 (at two
    wavelengths: one map, and both hold copies of one start field), map Q for 1, 3, 4 (3 at another wavelength), item 5
    switched off."""
    from paos_amd.aperture import EllipticalAperture
    from paos_amd.run import _Plans, _zernike_tables, zernike_tables

    h = N // 2
    geo = {"A": (20.0, 20.0), "B": (15.5, 12.25), "C": (10.0, 18.0)}  # semi-axes along x, y in pixels
    which = ["A", "B", "A", "B", "A", "C"]
    blocks = np.array([EllipticalAperture((N / 2, N / 2), *geo[k], 0.0).block(obscuration=False) for k in which])
    rows = np.array([[h - int(geo[k][1]) - 3, h + int(geo[k][1]) + 4] for k in which], dtype=np.float64)
    cols = np.array([[h - int(geo[k][0]) - 3, h + int(geo[k][0]) + 4] for k in which], dtype=np.float64)
    m, nn, norm = zernike_tables(15, "standard", True)
    rng = np.random.default_rng(16)
    p, q = rng.normal(0.0, 30e-9, 15), rng.normal(0.0, 30e-9, 15)

    def zplan(coef, wl, radius):
        return {"aperture": None, "stop": False, "phase_map": None,
                "zernike": dict(m=m, n=nn, norm=norm, Z=coef, dx=1.0 / 40.0, dy=1.0 / 40.0, radius=radius, wl=wl, origin="x",
                                pupil=None)}

    plans = _Plans([zplan(p, 1.0e-6, 0.5), zplan(q, 1.0e-6, 0.3), zplan(p, 1.3e-6, 0.5), zplan(q, 1.1e-6, 0.3),
                    zplan(q, 1.0e-6, 0.3), {"aperture": None, "stop": False, "phase_map": None, "zernike": None}])
    zs, nmax, kdim, table, build = _zernike_tables(plans)
    zb = build([z["Z"] if z is not None else None for z in zs])
    assert zb[5, 0] == 0.0 and zb[0, 0] != 0.0  # (item 5's record is switched off)
    return dict(blocks=blocks, stops=np.array([1.0, 1.0, 1.0, 0.0, 0.0, 1.0]), rows=rows, cols=cols, nmax=nmax, kdim=kdim,
                table=table, zb=zb, same_as=[0, 1, 0, 3, 4, 5])


def run_calls(items, precision="fp64"):
    """The calls under test on a context that holds ``items`` of the scenario (all six, or one alone), each on a field full of
    NaN: {name: [per item: field or power]}."""
    from paos_amd import _lib

    sc = scenario()
    nb = len(items)
    blocks, stops, rows, cols, zb = (sc[k][items] for k in ("blocks", "stops", "rows", "cols", "zb"))
    at = {it: k for k, it in enumerate(items)}
    like = [at.get(sc["same_as"][it], k) for k, it in enumerate(items)]  # (alone, an item stands for itself)
    zargs = (sc["nmax"], sc["kdim"], sc["table"], zb)
    dev = _lib.DeviceFields(N, nb, precision=precision)
    out = {}

    def poison():
        for i in range(nb):
            dev.upload(i, np.full((N, N), complex(np.nan, np.nan)))

    def fields():
        return [dev.download(i, _lib.WHAT_FIELD) for i in range(nb)]

    try:
        poison()
        dev.start(VALUE, _lib.SHAPE_ELLIPSE, blocks, stops, write_rows=rows)
        out["start_rows"] = fields()
        poison()
        dev.start(VALUE, _lib.SHAPE_ELLIPSE, blocks, stops, write_rows=rows, write_cols=cols)
        out["start_box"] = fields()
        ticket = dev.norm2_enqueue(rows, same_as=like, live_cols=cols)
        out["start_power"] = list(dev.norm2_fetch(ticket))
        dev.zernike(*zargs, same_as=like)
        out["zernike_like"] = fields()
        poison()
        dev.start(VALUE, _lib.SHAPE_ELLIPSE, blocks, stops, write_rows=rows, write_cols=cols)
        dev.zernike(*zargs)
        out["zernike"] = fields()
        poison()
        ticket = dev.start_zernike(VALUE, _lib.SHAPE_ELLIPSE, blocks, stops, rows, cols, *zargs, power=True)
        out["fused"] = fields()
        out["fused_power"] = list(dev.norm2_fetch(ticket))
    finally:
        dev.close()
    return out


def digests(results):
    """{name: [sha256 of each item's bytes]}: what crosses the process boundary.  (Every NaN counts as the same NaN: the
    pixels no call has written.)"""
    def canon(v):
        a = np.ascontiguousarray(v).view(np.float64)
        return np.where(np.isnan(a), np.nan, a).tobytes()

    return {name: [hashlib.sha256(canon(v)).hexdigest() for v in per_item] for name, per_item in results.items()}


def switched_worker(out, switch):
    """In a fresh process: the whole batch with ``switch`` (an environment variable the library reads once) set to 0.  Puts
    ("ok", digests) or ("fail", message) on ``out``."""
    import os

    try:
        os.environ[switch] = "0"
        out.put(("ok", digests(run_calls(list(range(6))))))
    except Exception as exc:  # noqa: BLE001 -- the parent reports it
        out.put(("fail", repr(exc)))
