#!/usr/bin/env python3
"""Everything the walk asks of the device, as text (python tools/walk_trace.py OUT.txt [SCENARIO ...]): a refactoring of
paos_amd/run.py that changes nothing writes the same file, byte for byte, as the commit before it.

Only the public API is used -- ``run``, ``run_batch`` and the NumPy model of the device (tests/fakes.py: ModelDevice) -- so
this very file runs on any commit.  The model device is wrapped in a recorder that writes one line per device method call:
the name, then a digest of every argument (arrays by dtype, shape and bytes; floats by ``float.hex``; a nested sequence
of numbers as the float64 array the library makes of it, so a list and an array of the same numbers agree).  Every
returned record follows: scalars, powers, arrays, the numbers of the aperture handles, the ray-transfer matrices.  The
legacy NumPy generator is seeded before each scenario (the PSD draws).  No GPU is needed."""
import hashlib
import os
import sys
from numbers import Integral, Real

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from fakes import ModelDevice  # noqa: E402
from paos_amd import _lib  # noqa: E402
from paos_amd import run as prun  # noqa: E402
from paos_amd.abcd import ABCD  # noqa: E402
from paos_amd.chains import syn20_chain, syn20_orthonorm_chain, syn20_wavelength  # noqa: E402
from paos_amd.parse_config import parse_config  # noqa: E402

LENS = os.path.join(ROOT, "data", "lens")
TIE = 94906267.0 * 2.0 ** -40  # a slope whose square is a tie between two doubles (tests/test_field_points.py)
OUT = []


def _array(a):
    a = np.ascontiguousarray(a)
    return f"{a.dtype.str}{list(a.shape)}:{hashlib.sha1(a.tobytes()).hexdigest()[:16]}"


def digest(x):
    if x is None or isinstance(x, (str, bytes)):
        return repr(x)
    if isinstance(x, (bool, np.bool_)):
        return "T" if x else "F"
    if isinstance(x, Integral):
        return f"i{int(x)}"
    if isinstance(x, Real):
        return float(x).hex()
    if isinstance(x, complex):
        return f"({x.real.hex()},{x.imag.hex()})"
    if isinstance(x, np.ma.MaskedArray):
        return f"ma({_array(np.ma.getdata(x))},{_array(np.ma.getmaskarray(x))})"
    if isinstance(x, np.ndarray):
        return _array(x)
    if isinstance(x, dict):
        return "{" + ",".join(f"{k!r}:{digest(v)}" for k, v in sorted(x.items(), key=lambda kv: repr(kv[0]))) + "}"
    if isinstance(x, (list, tuple)):
        if len(x) and not any(v is None or isinstance(v, (str, bytes, dict)) for v in x):
            try:
                a = np.asarray(x)
            except ValueError:
                a = None
            if a is not None and a.dtype.kind in "biuf":
                return _array(a.astype(np.float64))
        return "[" + ",".join(digest(v) for v in x) + "]"
    if isinstance(x, ABCD):
        return "ABCD" + _array(np.asarray(x(), dtype=np.float64))
    name = type(x).__name__
    if name in ("EllipticalAperture", "RectangularAperture"):
        sizes = (x.a, x.b) if name == "EllipticalAperture" else (x.w, x.h)
        return f"{name}({digest(list(x.positions))},{digest(sizes[0])},{digest(sizes[1])},{digest(x.theta)})"
    if name == "Detector":
        return "Detector" + digest(vars(x))
    raise TypeError(f"walk_trace cannot digest a {name}")


class Recorder:
    """A ModelDevice whose every method call is written down."""

    def __init__(self, n, batch=1, precision="fp64", device=0):
        self.__dict__["_dev"] = ModelDevice(n, batch, precision, device)
        OUT.append(f"  device {n} x {batch} {precision}")

    def __getattr__(self, name):
        attr = getattr(self._dev, name)
        if not callable(attr):
            return attr

        def call(*args, **kw):
            OUT.append(f"  {name}(" + ", ".join([digest(a) for a in args] + [f"{k}={digest(v)}" for k, v in sorted(kw.items())]) + ")")
            return attr(*args, **kw)

        return call

    def __setattr__(self, name, value):
        setattr(self._dev, name, value)


def records(results):
    for i, res in enumerate(results if isinstance(results, list) else [results]):
        for num in res:
            for key in sorted(res[num]):
                OUT.append(f"  -> item {i} surface {num} {key} = {digest(res[num][key])}")


def scenario(title):
    np.random.seed(20261019)
    prun.forget_maps()
    OUT.append(f"== {title}")


def attempt(what, call):
    """A call that the product may refuse: the refusal is part of the trace."""
    mark = len(OUT)
    try:
        records(call())
    except Exception as exc:  # noqa: BLE001
        del OUT[mark:]
        OUT.append(f"  {what}: refused, {type(exc).__name__}")


def batch(title, pup, wls, n, zoom, field, chains, **kw):
    scenario(title)
    attempt("run_batch", lambda: prun.run_batch(pup, wls, n, zoom, field, chains, dev=Recorder(n, len(chains)), **kw))


def single(title, pup, wl, n, zoom, field, chain):
    scenario(title)
    keep = _lib.DeviceFields
    _lib.DeviceFields = Recorder
    try:
        attempt("run", lambda: prun.run(pup, wl, n, zoom, field, chain))
    finally:
        prun.release_contexts()
        _lib.DeviceFields = keep


LEAN, ORDINARY = dict(outputs=(), keep_psf=True), dict(outputs=("psf",))
AXIS = {"us": 0.0, "ut": 0.0}


def syn20():
    for n in (256, 1024):
        for tag, kw in (("lean", LEAN), ("ordinary", ORDINARY)):
            batch(f"SYN20 x 4 wavelengths {n} {tag}", 1.0, [syn20_wavelength(k) for k in (0, 100, 300, 511)], n, 4, AXIS,
                  [syn20_chain() for _ in range(4)], **kw)


def lens_files():
    for name in sorted(os.listdir(LENS)):
        if not name.endswith(".ini"):
            continue
        scenario(f"lens file {name}: parse")
        try:
            pup, par, wls, fields, chains = parse_config(os.path.join(LENS, name))
        except Exception as exc:  # noqa: BLE001
            OUT.append(f"  parse_config: refused, {type(exc).__name__}")
            continue
        pick = [0, len(wls) - 1]
        for tag, kw in (("lean", LEAN), ("ordinary", ORDINARY)):
            batch(f"lens file {name} 2 wavelengths 256 {tag}", pup, [1e-6 * wls[k] for k in pick], 256, par["zoom"], fields[0],
                  [chains[k] for k in pick], **kw)
        single(f"lens file {name} run() 256", pup, 1e-6 * wls[0], 256, par["zoom"], fields[0], chains[0])
        if "PSD" in name:  # (the PSD band of the file needs the file's own sampling)
            n = int(par["grid_size"])
            batch(f"lens file {name} 2 wavelengths {n} ordinary", pup, [1e-6 * wls[k] for k in pick], n, par["zoom"], fields[0],
                  [chains[k] for k in pick], **ORDINARY)


def grid_sag():
    """test_Grid_Sag.ini names a sag file that is not shipped: it is parsed with a smooth bump written next to a copy."""
    import configparser
    import tempfile

    cfg = configparser.ConfigParser()
    cfg.read(os.path.join(LENS, "test_Grid_Sag.ini"))
    y, x = np.mgrid[-32:32, -32:32] / 32.0
    with tempfile.TemporaryDirectory() as tmp:
        np.save(os.path.join(tmp, "sag.npy"), {"data": 0.05 * np.exp(-4.0 * (x * x + 2.0 * y * y)), "nx": 64, "ny": 64,
                                               "delx": 1.0e-2, "dely": 1.0e-2, "xdec": 3.0, "ydec": -2.0}, allow_pickle=True)
        for sec in cfg.sections():
            if sec.startswith("lens_") and cfg[sec].get("SurfaceType") == "Grid Sag":
                cfg[sec]["Par8"] = os.path.join(tmp, "sag.npy")
        with open(os.path.join(tmp, "gs.ini"), "w") as fh:
            cfg.write(fh)
        pup, par, wls, fields, chains = parse_config(os.path.join(tmp, "gs.ini"))
    pick = [0, len(wls) - 1]
    for tag, kw in (("lean", LEAN), ("ordinary", ORDINARY)):
        batch(f"Grid Sag lens file 2 wavelengths 256 {tag}", pup, [1e-6 * wls[k] for k in pick], 256, par["zoom"], fields[0],
              [chains[k] for k in pick], **kw)
    batch("Grid Sag lens file one wavelength twice 256 (a shared map)", pup, [1e-6 * wls[0]] * 2, 256, par["zoom"], fields[0],
          [chains[0]] * 2, **ORDINARY)
    single("Grid Sag lens file run() 256", pup, 1e-6 * wls[0], 256, par["zoom"], fields[0], chains[0])


def field_points():
    pup, par, wls, fields, chains = parse_config(os.path.join(LENS, "periscope.ini"))
    fl = [fields[0], fields[1], {"us": 3.0e-4, "ut": -5.0e-4}, {"us": TIE, "ut": -TIE}, AXIS]
    for tag, kw in (("lean", LEAN), ("ordinary", ORDINARY)):
        batch(f"periscope five field points 1024 {tag}", pup, [1e-6 * wls[0]] * 5, 1024, par["zoom"], fl, [chains[0]] * 5, **kw)


def _with_apertures(per_item):
    """SYN20 chains whose first aperture differs from item to item: ``per_item[i]`` edits item i's aperture dict (None
    takes the entry away)."""
    chains = []
    for edit in per_item:
        chain = syn20_chain()
        key = next(k for k, it in chain.items() if it.get("aperture") is not None)
        hit = [k for k, it in chain.items() if it.get("aperture") is not None][2]
        for k in (key, hit):
            item = dict(chain[k])
            if edit is None:
                item.pop("aperture")
            else:
                item["aperture"] = dict(item["aperture"], **edit)
            chain[k] = item
        chains.append(chain)
    return chains


def partly_on():
    edits = [{}, {"xrad": float("nan")}, {"shape": "rectangular"}, {"type": "obscuration", "xrad": 0.1, "yrad": 0.1}, None,
             {"shape": "rectangular", "xc": 0.02, "yc": float("nan")}]
    wls = [syn20_wavelength(7 * k) for k in range(len(edits))]
    fl = [AXIS, AXIS, {"us": 5e-5, "ut": 0.0}, AXIS, {"us": TIE, "ut": -TIE}, AXIS]
    for n in (256, 1024):
        for tag, kw in (("lean", LEAN), ("ordinary", ORDINARY)):
            batch(f"partly-on mixed-shape batch {n} {tag}", 1.0, wls, n, 4, AXIS, _with_apertures(edits), **kw)
            batch(f"partly-on mixed-shape batch off axis {n} {tag}", 1.0, wls, n, 4, fl, _with_apertures(edits), **kw)
    # every item on, two shapes; one shape with one item's box off the grid (the reference's TypeError)
    batch("two shapes, all on 1024 lean", 1.0, wls[:2], 1024, 4, AXIS, _with_apertures([{}, {"shape": "rectangular"}]), **LEAN)
    batch("an aperture that misses the grid", 1.0, wls[:2], 256, 4, AXIS, _with_apertures([{}, {"xc": 50.0}]), **LEAN)
    batch("a shape nobody renders", 1.0, wls[:2], 256, 4, AXIS, _with_apertures([{}, {"shape": "circular"}]), **LEAN)


def mixed_kinds():
    """Items that differ in kind at one surface: Standard, Zernike, Coordinate Break."""
    chains = []
    for kind in ("Zernike", "Standard", "Coordinate Break", "Zernike"):
        chain = syn20_chain()
        key = next(k for k, it in chain.items() if it["type"] == "Zernike")
        if kind == "Standard":
            chain[key] = dict(chain[key], type="Standard")
        elif kind == "Coordinate Break":
            chain[key] = dict(chain[key], type="Coordinate Break", xdec=1e-5, ydec=float("nan"), xrot=2e-5, yrot=-1.5e-5)
        chains.append(chain)
    wls = [syn20_wavelength(k) for k in (0, 5, 9, 200)]
    for tag, kw in (("lean", LEAN), ("ordinary", ORDINARY)):
        batch(f"mixed kinds at one surface 256 {tag}", 1.0, wls, 256, 4, AXIS, chains, **kw)


def zorthonorm():
    chain = syn20_orthonorm_chain()
    chain[2] = dict(chain[2], save=True)
    batch("Zorthonorm batch 256", 1.0, [1.0e-6, 1.2e-6], 256, 4, AXIS, [chain, chain], **ORDINARY)
    single("Zorthonorm run() 256", 1.0, 1.0e-6, 256, 4, AXIS, chain)
    bare = dict(chain)
    bare[2] = {k: v for k, v in chain[2].items() if k != "aperture"}
    single("Zorthonorm without an aperture", 1.0, 1.0e-6, 256, 4, AXIS, bare)


def psd():
    def chain():
        out = {}
        for item in syn20_chain().values():
            num = len(out) + 1
            out[num] = dict(item, num=num)
            if item["name"] == "Z1":
                num = len(out) + 1
                out[num] = dict(A=12.0, B=1.0, C=2.2, fknee=3.0, fmin=0.5, fmax=6.0, SR=2.0, units="nm", num=num, type="PSD",
                                name="SCREEN", is_stop=False, save=True, ABCDt=ABCD(thickness=0.0, curvature=0.0),
                                ABCDs=ABCD(thickness=0.0, curvature=0.0))
        return out

    from paos_amd import phase_maps

    keep = phase_maps.PSD_ON_DEVICE_FROM
    try:
        for tag, first in (("on the device", 256), ("on the host", 1 << 20)):
            phase_maps.PSD_ON_DEVICE_FROM = first
            batch(f"PSD surface, batch of 3, 256, screens {tag}", 1.0, [1.0e-6, 1.1e-6, 1.3e-6], 256, 4, AXIS,
                  [chain() for _ in range(3)], **ORDINARY)
            single(f"PSD surface run() 256, screen {tag}", 1.0, 1.0e-6, 256, 4, AXIS, chain())
    finally:
        phase_maps.PSD_ON_DEVICE_FROM = keep


SCENARIOS = dict(syn20=syn20, lens_files=lens_files, grid_sag=grid_sag, field_points=field_points, partly_on=partly_on, mixed_kinds=mixed_kinds,
                 zorthonorm=zorthonorm, psd=psd)

if __name__ == "__main__":
    for name in sys.argv[2:] or SCENARIOS:
        SCENARIOS[name]()
    text = "\n".join(OUT) + "\n"
    with open(sys.argv[1], "w") as fh:
        fh.write(text)
    print(f"{len(OUT)} lines, {sum(1 for line in OUT if line.startswith('=='))} scenarios, sha256 "
          f"{hashlib.sha256(text.encode()).hexdigest()}")
