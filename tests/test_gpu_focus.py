"""Through-focus stacks on the GPU (paos_focus_begin / paos_focus_plane / paos_focus_end, run_batch(focus_planes=...)):
planes against the NumPy restatement (tests/focus_np.py) and the oracle, the bit-for-bit invariants, the consumers per
plane, the count of line transforms, and misuse of the C calls."""
import copy
import os

import numpy as np
import pytest

import detector_np
import focus_np
from conftest import l2_rel_err, rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = os.path.join(ROOT, "data", "lens")
FIELD = {"us": 0.0, "ut": 0.0}
# the project's parity gates: max-norm and L2-relative
GATE = {"fp64": 1.0e-10, "fp32": 2.0e-5}


def _case(name, n):
    from paos_amd.chains import parse_config_variant, syn20_chain, syn20_wavelength

    if name == "SYN20":
        wls = [syn20_wavelength(k) for k in ((0, 511) if n >= 4096 else (0, 200, 511))]
        return 1.0, 4, FIELD, wls, [syn20_chain() for _ in wls]
    pup, par, wls, fields, chains = parse_config_variant(os.path.join(LENS, "Ariel_AIRS-CH0.ini"), [1.95, 3.9])
    return pup, par["zoom"], fields[0], [1e-6 * w for w in wls], chains


def _planes(ends, n, count):
    """Defocus values from the oracle's pilot beams: within every item's sampling limit N d^2 / wl, on both sides of
    the nominal plane (which is one of them), the largest one about 2 zr of the first item away."""
    limit = min(n * min(w.dx, w.dy) ** 2 / w.wl for w in ends)
    step = min(0.9 * min(w.zr for w in ends), 0.45 * limit)
    return [step, 0.0, -2.0 * step, 0.37 * step][:count]


@pytest.mark.parametrize("name,n,precision", [("SYN20", 256, "fp64"), ("SYN20", 1024, "fp64"), ("SYN20", 4096, "fp64"),
                                              ("Ariel_AIRS-CH0", 1024, "fp64"), ("SYN20", 256, "fp32"),
                                              ("SYN20", 1024, "fp32")])
def test_planes_against_restatement_and_oracle(name, n, precision):
    """Field and power of every plane of a mixed-wavelength batch against ``RefWFO.ptp`` on the oracle's field behind the
    last surface (complex128) and against the restatement on the nominal field the device returned, at the parity gate
    of the context's precision.  Largest errors seen on an MI355X are printed (pytest -s)."""
    from paos_amd.run import run_batch

    pup, zoom, field, wls, chains = _case(name, n)
    num = chains[0][list(chains[0].keys())[-1]]["num"]
    ends = [focus_np.oracle_end_state(pup, wl, n, zoom, field, ch)[1] for wl, ch in zip(wls, chains)]
    planes = _planes(ends, n, 3 if n >= 4096 else 4)
    gate = GATE[precision]
    res = run_batch(pup, wls, n, zoom, field, chains, outputs=("wfo",), precision=precision, focus_planes=planes)
    worst = [0.0, 0.0, 0.0, 0.0]
    for i, end in enumerate(ends):
        nominal = res[i][num]["wfo"]
        stack = res[i][num]["focus"]
        assert [p["dz"] for p in stack] == planes
        for p in stack:
            if p["dz"] == 0.0:
                assert np.array_equal(p["wfo"], nominal)
                continue
            ref = copy.deepcopy(end)
            ref.ptp(p["dz"])
            restated = focus_np.plane(nominal, end.wl, end.dx, end.dy, p["dz"])
            want_power = float(np.sum(np.abs(ref._wfo) ** 2))
            errs = [rel_err(p["wfo"], ref._wfo), l2_rel_err(p["wfo"], ref._wfo), rel_err(p["wfo"], restated),
                    abs(p["power"] - want_power) / want_power]
            worst = [max(a, b) for a, b in zip(worst, errs)]
            print(f"focus {name} {n}^2 {precision} item {i} dz {p['dz']:+.3e}: oracle max {errs[0]:.2e} L2 {errs[1]:.2e}, "
                  f"restatement max {errs[2]:.2e}, power {errs[3]:.2e}")
            assert all(e < gate for e in errs), (i, p["dz"], errs, gate)
            assert p["z"] == ref.z and p["wz"] == ref.wz and p["distancetofocus"] == ref.distancetofocus
    print(f"focus {name} {n}^2 {precision}: worst oracle max {worst[0]:.2e} L2 {worst[1]:.2e} restatement {worst[2]:.2e} "
          f"power {worst[3]:.2e} (gate {gate:.0e})")


@pytest.mark.parametrize("n", [256, 1024])
def test_nominal_records_do_not_change(n):
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.run import run_batch

    wls = [syn20_wavelength(k) for k in (3, 400)]
    chains = [syn20_chain() for _ in wls]
    kw = dict(outputs=("wfo", "psf"), metrics_radii_px=[2.0, 9.5])
    plain = run_batch(1.0, wls, n, 4, FIELD, chains, **kw)
    res = run_batch(1.0, wls, n, 4, FIELD, chains, focus_planes=[5.0e-5, 0.0, -1.0e-4], **kw)
    for a, b in zip(plain, res):
        assert sorted(a) == sorted(b)
        for key, rec in a.items():
            for k, v in rec.items():
                if isinstance(v, np.ndarray):
                    assert np.array_equal(b[key][k], v), (key, k)
                elif k == "metrics":
                    assert all(np.array_equal(np.asarray(v[m]), np.asarray(b[key][k][m])) for m in v), key
                elif k not in ("ABCDt", "ABCDs", "aperture"):
                    assert b[key][k] == v, (key, k)
        assert np.array_equal(b[20]["focus"][1]["wfo"], a[20]["wfo"]) and np.array_equal(b[20]["focus"][1]["psf"], a[20]["psf"])


def _fields(n, batch, boxed):
    rng = np.random.default_rng(20260 + n)
    out = []
    for i in range(batch):
        u = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        if boxed:  # a live box, as behind a field stop: exact zeros outside
            lo, hi = n // 2 - n // 10 - i, n // 2 + n // 10 + 2 * i
            m = np.zeros((n, n))
            m[lo:hi, lo + 1:hi + 3] = 1.0
            u = u * m
        out.append(u)
    return out


def _blocks(n, batch, dz, dx=2.5e-6, dy=3.1e-6):
    return [[1.0, 1.0 / (n * dx), 1.0 / (n * dy), np.pi * (1.0e-6 * (1 + 0.1 * i)) * dz, -1.0] for i in range(batch)]


@pytest.mark.parametrize("n,precision,boxed", [(256, "fp64", False), (1024, "fp64", True), (2048, "fp32", True),
                                               (64, "fp32", False)])
def test_invariants_bit_for_bit(n, precision, boxed):
    """focus_begin leaves the field as it was; a plane does not depend on the planes computed before it, nor on
    whether pruning is on; and it is paos_ptp's plane at the parity gate."""
    from paos_amd import _lib

    batch = 2
    fields = _fields(n, batch, boxed)
    dzs = [4.0e-5, -7.0e-5, 1.1e-4]
    dev = _lib.DeviceFields(n, batch, precision)
    try:
        for i, u in enumerate(fields):
            dev.upload(i, u)
        before = [dev.download(i) for i in range(batch)]
        dev.focus_begin()
        assert all(np.array_equal(dev.download(i), before[i]) for i in range(batch))
        dev.focus_plane(_blocks(n, batch, dzs[0]))
        first = [dev.download(i) for i in range(batch)]
        for dz in dzs[1:]:
            dev.focus_plane(_blocks(n, batch, dz))
        dev.focus_plane(_blocks(n, batch, dzs[0]))
        assert all(np.array_equal(dev.download(i), first[i]) for i in range(batch)), "a plane depends on its predecessors"
        dev.focus_end()
        # pruning off: the same bits
        dev.set_pruning(False)
        for i, u in enumerate(fields):
            dev.upload(i, u)
        dev.focus_begin()
        dev.focus_plane(_blocks(n, batch, dzs[0]))
        assert all(np.array_equal(dev.download(i), first[i]) for i in range(batch)), "pruning changes a plane"
        dev.focus_end()
        dev.set_pruning(True)
        # paos_ptp on the same field
        for i, u in enumerate(fields):
            dev.upload(i, u)
        dev.ptp(_blocks(n, batch, dzs[0]))
        for i in range(batch):
            got = dev.download(i)
            assert rel_err(first[i], got) < GATE[precision] and l2_rel_err(first[i], got) < GATE[precision]
            want = focus_np.plane(before[i], 1.0e-6 * (1 + 0.1 * i), 2.5e-6, 3.1e-6, dzs[0])
            assert rel_err(first[i], want) < GATE[precision] and l2_rel_err(first[i], want) < GATE[precision]
    finally:
        dev.close()


def test_consumers_work_on_the_plane():
    """metrics and detector image of every plane against NumPy on the plane's fetched PSF."""
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.detector import Detector
    from paos_amd.run import run_batch

    n, wls = 512, [syn20_wavelength(k) for k in (0, 300)]
    chains = [syn20_chain() for _ in wls]
    radii = [1.5, 6.0, 40.0]
    planes = [1.0e-4, 0.0, -6.0e-5]
    probe = run_batch(1.0, wls[:1], n, 4, FIELD, chains[:1], outputs=())[0][20]
    det = Detector(33, 21, 1.7 * probe["dx"], 2.3 * probe["dy"], xc=0.31 * probe["dx"], yc=-0.62 * probe["dy"])
    res = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=("psf",), metrics_radii_px=radii, detector=det,
                    focus_planes=planes)
    yy, xx = np.mgrid[0:n, 0:n]
    d2 = (xx - n / 2) ** 2 + (yy - n / 2) ** 2
    for i in range(len(wls)):
        rec = res[i][20]
        for p in rec["focus"]:
            psf, m = p["psf"], p["metrics"]
            assert abs(m["power"] - psf.sum()) < 1e-11 * psf.sum() and abs(p["power"] - psf.sum()) < 1e-11 * psf.sum()
            assert abs(m["peak"] - psf.max()) < 1e-12 * psf.max()
            for r, ee in zip(radii, m["encircled"]):
                assert abs(ee - psf[d2 <= r * r].sum()) < 1e-10 * psf.sum(), (i, p["dz"], r)
            want = detector_np.rebin(psf, det, rec["dx"], rec["dy"])
            assert want.max() > 0.0
            assert rel_err(p["detector"], want) < 1e-13 and l2_rel_err(p["detector"], want) < 1e-13, (i, p["dz"])
        assert np.array_equal(rec["focus"][1]["detector"], rec["detector"])


def test_the_forward_transform_runs_once():
    """paos_profile_line_transforms: a K-plane stack runs at most 2N + K 2N line transforms per item, K calls of
    paos_ptp run 4N K (1024^2 complex128: the grid whose ptp reports its line counts)."""
    from paos_amd import _lib

    n, batch, k = 1024, 2, 3
    dev = _lib.DeviceFields(n, batch, "fp64")
    try:
        for i, u in enumerate(_fields(n, batch, False)):
            dev.upload(i, u)
        dev.profile_begin(_lib.KERNEL_PASS_ANY)
        dev.focus_begin()
        for j in range(k):
            dev.focus_plane(_blocks(n, batch, 3.0e-5 * (j + 1)))
        stack = dev.profile_line_transforms()
        dev.profile_end_launches()
        dev.focus_end()
        dev.profile_begin(_lib.KERNEL_PASS_ANY)
        for j in range(k):
            dev.ptp(_blocks(n, batch, 3.0e-5 * (j + 1)))
        ptp = dev.profile_line_transforms()
        dev.profile_end_launches()
    finally:
        dev.close()
    print(f"line transforms per item: stack {stack.sum() / batch:.0f} in {stack.size} launches, "
          f"{k} x ptp {ptp.sum() / batch:.0f} in {ptp.size} launches")
    assert stack.size == 2 + 2 * k and 0 < stack.sum() <= batch * (2 * n + k * 2 * n)
    assert ptp.sum() == batch * 4 * n * k


def test_misuse_is_refused_and_the_context_stays_usable():
    import ctypes

    from paos_amd import _lib

    n, batch = 128, 2
    dev = _lib.DeviceFields(n, batch, "fp64")
    lib, ctx = dev._lib, dev._ctx
    dp = ctypes.POINTER(ctypes.c_double)

    def raw(blocks):
        return np.ascontiguousarray(blocks, dtype=np.float64)

    try:
        fields = _fields(n, batch, False)
        for i, u in enumerate(fields):
            dev.upload(i, u)
        good = raw(_blocks(n, batch, 5.0e-5))
        assert lib.paos_focus_plane(ctx, good.ctypes.data_as(dp)) == 1 and b"begin" in lib.paos_last_error(ctx)
        assert lib.paos_focus_end(ctx) == 1
        assert lib.paos_focus_begin(ctx) == 0
        assert lib.paos_focus_begin(ctx) == 1 and b"already" in lib.paos_last_error(ctx)
        assert lib.paos_focus_plane(ctx, None) == 1
        for bad in (float("nan"), float("inf")):
            b = good.copy()
            b[1, 3] = bad
            assert lib.paos_focus_plane(ctx, b.ctypes.data_as(dp)) == 1 and b"item 1" in lib.paos_last_error(ctx)
        # nothing of the above touched the field; the stack still works
        assert all(np.array_equal(dev.download(i), fields[i]) for i in range(batch))
        dev.focus_plane(good)
        for i in range(batch):
            want = focus_np.plane(fields[i], 1.0e-6 * (1 + 0.1 * i), 2.5e-6, 3.1e-6, 5.0e-5)
            assert rel_err(dev.download(i), want) < 1e-10
        dev.focus_end()
        assert lib.paos_focus_begin(ctx) == 0 and lib.paos_focus_end(ctx) == 0
    finally:
        dev.close()
