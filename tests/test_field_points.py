"""Several field points per batch (run_batch / run_broadband / run_sharded with one field per chain) and detector
images placed at each item's chief ray, on the CPU: the batch planner's array arithmetic against the scalar planner of
tests/plan_np.py for off-axis items, per-item fields on the NumPy model of the device against the oracle, the chief-ray origins against
paos_amd.raytrace, the placed restatement against brute-force supersampling, and the argument checks."""
import copy
import os

import numpy as np
import pytest

import detector_np
import detector_placed_np
from conftest import l2_rel_err, rel_err
from detector_placed_np import DetectorModelDevice
from fakes import ModelDevice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = os.path.join(ROOT, "data", "lens")
SYNTH = {"us": 3.0e-4, "ut": -5.0e-4}
# a slope whose square is a tie between two doubles: C pow and a multiplication may round it differently
TIE = 94906267.0 * 2.0 ** -40


def _lens(name):
    from paos_amd.parse_config import parse_config

    return parse_config(os.path.join(LENS, name + ".ini"))


def _compare_plans(fast, slow, nb):
    import plan_np
    from paos_amd import run as prun

    assert fast.ap is not None and fast.ap.on.all()
    blocks, _ = fast.ap.blocks()
    for i in range(nb):
        h, o = slow[i]
        assert list(blocks[i]) == h.block(obscuration=o), i
        fh, fo = fast.aperture(i), bool(fast.ap.obsc[i])
        assert type(fh) is type(h) and fo == o
    n = 1024
    la, lb = [[0, n] for _ in range(nb)], [[0, n] for _ in range(nb)]
    prun._live_rows_after(fast, la, n)
    plan_np.live_rows_after(slow, lb, n)
    assert la == lb
    assert prun._live_cols_of(fast, n) == plan_np.live_cols_of(slow, n)


@pytest.mark.parametrize("with_break", [False, True])
def test_batch_planner_array_path_equals_the_per_item_planner_off_axis(with_break):
    """_plan_surface with the walk's ray arrays: mixed on- and off-axis items (missing centres fall back on the chief ray,
    radii shrink with the slopes) are planned with array arithmetic, and every number equals the scalar planner's
    (tests/plan_np.py); a coordinate break in front moves the rays of every item exactly as the scalar planner moves
    them."""
    import plan_np
    from paos_amd import run as prun
    from paos_amd.abcd import ABCD

    n, nb = 1024, 10
    rng = np.random.default_rng(5)
    fields = [{"us": 0.0, "ut": 0.0}, {"us": 0.0, "ut": 1.2e-5}, SYNTH, {"us": TIE, "ut": -TIE}, {"us": -2e-3, "ut": 0.0}]
    fields = [fields[i % len(fields)] for i in range(nb)]
    slow_rays = [plan_np.Ray(f) for f in fields]
    rays = prun._Rays(fields)
    dxs = [4.0 / n * (1 + 0.01 * i) for i in range(nb)]
    dys = [4.0 / n * (1 + 0.02 * i) for i in range(nb)]
    wls = [1e-6] * nb
    abcd = ABCD(thickness=0.3, curvature=0.7)
    surfaces = []
    if with_break:
        surfaces.append([{"type": "Coordinate Break", "is_stop": False, "save": False, "xdec": 1e-3, "ydec": float("nan"),
                          "xrot": 2.0, "yrot": -1.5, "ABCDt": ABCD(), "ABCDs": ABCD()} for _ in range(nb)])
    for shape in ("elliptical", "rectangular"):
        items = []
        for i in range(nb):
            ap = {"shape": shape, "type": "aperture" if i % 3 else "obscuration",
                  "xc": float("nan") if i % 2 else float(rng.normal(0, 0.01)),
                  "yc": float("nan") if i % 4 == 1 else float(rng.normal(0, 0.01)),
                  "xrad": float(rng.uniform(0.2, 0.6)), "yrad": float(rng.uniform(0.2, 0.6))}
            items.append({"type": "Standard", "is_stop": bool(i % 2), "save": False, "aperture": ap,
                          "ABCDt": abcd, "ABCDs": abcd})
        surfaces.append(items)
    for items in surfaces:
        fast = prun._plan_surface(items, n, dxs, dys, wls, lambda i: 0.5, rays)
        slow = [plan_np.plan_aperture(r, it, n, dxs[i], dys[i]) for i, (r, it) in enumerate(zip(slow_rays, items))]
        for i, r in enumerate(slow_rays):
            assert rays.vt[i].tolist() == r.vt.tolist() and rays.vs[i].tolist() == r.vs.tolist(), i
            assert bool(rays.still[i]) == r.still
        if items[0]["type"] != "Coordinate Break":
            _compare_plans(fast, slow, nb)
        # the ray update of the walk: one stacked A @ v == the per-item products
        col = [it["ABCDt"] for it in items]
        rays.advance(col, col)
        for r in slow_rays:
            if not r.still:
                r.advance(col[0], col[0])
        for i, r in enumerate(slow_rays):
            assert rays.vt[i].tolist() == r.vt.tolist() and rays.vs[i].tolist() == r.vs.tolist(), i
    assert not rays.all_still()


def _per_item_against_oracle(name, n, field_list, wl_list):
    from oracle.run_np import run as oracle_run
    from paos_amd.run import run_batch

    pup, par, wls, fields, chains = _lens(name)
    nb = len(field_list)
    chain_of = {wl: chains[wls.index(wl)] for wl in set(wl_list)}
    batch_chains = [chain_of[wl] for wl in wl_list]
    res = run_batch(pup, [1e-6 * wl for wl in wl_list], n, par["zoom"], field_list, batch_chains, outputs=("psf", "wfo"),
                    dev=ModelDevice(n, nb))
    last = list(batch_chains[0].keys())[-1]
    for i in range(nb):
        ref = oracle_run(pup, 1e-6 * wl_list[i], n, par["zoom"], field_list[i], batch_chains[i], light=True)
        assert sorted(ref) == sorted(res[i])
        for num in ref:
            for k in ("dx", "dy", "wz", "distancetofocus", "fratio"):
                assert res[i][num][k] == ref[num][k], (i, num, k)
        e = rel_err(res[i][last]["wfo"], ref[last]["wfo"])
        assert e < 1e-10, (i, e)
        # the same item in a batch of its own field point: the same numbers
        alone = run_batch(pup, [1e-6 * wl_list[i]], n, par["zoom"], field_list[i], [batch_chains[i]], outputs=("psf",),
                          dev=ModelDevice(n, 1))
        assert np.array_equal(alone[0][last]["psf"], res[i][last]["psf"]), i
    return res, fields


@pytest.mark.parametrize("name", ["periscope", "Ariel_FGS-FGS1"])
def test_run_batch_per_item_fields_against_the_oracle(name):
    """f1 and f2 of the lens file (periscope: coordinate breaks that tilt the line of sight) and a synthetic field point,
    interleaved in one batch on the model device: every item agrees with the oracle run at its own field point."""
    _, _, wls, fields, _ = _lens(name)
    fl = [fields[0], fields[1], SYNTH, fields[1]]
    wl = [wls[0], wls[-1], wls[0], wls[0]]
    _per_item_against_oracle(name, 64, fl, wl)


def test_chief_ray_origins_follow_the_raytrace():
    """detector_origin="chief_ray": the (x0, y0) handed to the placed detector call are the chief ray's position at the
    last surface -- the raytrace's ray behind the surface in front of it (the last surface is no coordinate break) -- and
    the images are the placed restatement of the kept PSFs."""
    from paos_amd.detector import Detector
    from paos_amd.raytrace import trace
    from paos_amd.run import run_batch

    for name in ("Ariel_FGS-FGS1", "periscope"):
        pup, par, wls, fields, chains = _lens(name)
        fl = [fields[0], fields[1], SYNTH]
        n = 64
        chain = chains[0]
        last = list(chain.keys())[-1]
        assert chain[last]["type"] != "Coordinate Break"
        dev = DetectorModelDevice(n, 3)
        res = run_batch(pup, [1e-6 * wls[0]] * 3, n, par["zoom"], fl, [chain] * 3, outputs=(), dev=dev,
                        detector=Detector(16, 12, 1e-6), detector_origin="chief_ray")
        origins = dev.origins_seen[-1]
        for i, f in enumerate(fl):
            rays = list(trace(f, chain))
            _, _, vt, vs = rays[-2]
            assert origins[i].tolist() == [float(vs[0]), float(vt[0])], (name, i)
            want = detector_placed_np.rebin_placed(dev.psf_fetch(i), dev.detector, res[i][last]["dx"], res[i][last]["dy"],
                                                   *origins[i])
            assert np.array_equal(res[i][last]["detector"], want)
        assert origins[1][1] != origins[0][1]  # (f2 lands elsewhere than f1)


def test_placed_restatement_against_supersampling():
    from paos_amd.detector import Detector

    rng = np.random.default_rng(3)
    n = 16
    psf = rng.uniform(0.0, 1.0, (n, n))
    dx, dy = 1.0, 0.5
    det = Detector(11, 9, 0.75, 0.375, xc=0.25, yc=-0.125)
    for x0, y0 in ((0.0, 0.0), (0.25, -0.5), (-3.0, 1.375), (5.5, 2.25), (40.0, 0.0)):
        got = detector_placed_np.rebin_placed(psf, det, dx, dy, x0, y0)
        want = detector_placed_np.supersampled(psf, det, dx, dy, x0, y0, 8)
        assert np.allclose(got, want, rtol=1e-13, atol=1e-14), (x0, y0)
        if x0 == 40.0:
            assert not got.any()
    # zero offsets: the unplaced restatement, bit for bit
    for d in (det, Detector(37, 29, 1.7e-6, 1.3e-6, xc=0.31e-6, yc=-0.77e-6)):
        assert np.array_equal(detector_placed_np.rebin_placed(psf, d, 1e-6, 1.1e-6, 0.0, 0.0),
                              detector_np.rebin(psf, d, 1e-6, 1.1e-6))
    # an offset moves the image: a shift by whole detector pixels is a shift of the array
    a = detector_placed_np.rebin_placed(psf, det, dx, dy, 0.0, 0.0)
    b = detector_placed_np.rebin_placed(psf, det, dx, dy, 2 * 0.75, -1 * 0.375)
    assert np.allclose(b[:-1, 2:], a[1:, :-2], rtol=1e-13, atol=1e-15)


def test_argument_checks():
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.detector import Detector, run_broadband
    from paos_amd.run import run_batch

    chain = syn20_chain()
    wls = [syn20_wavelength(0)] * 2
    on = {"us": 0.0, "ut": 0.0}

    def rb(**kw):
        args = dict(field=[on, on], dev=ModelDevice(64, 2), outputs=())
        args.update(kw)
        field = args.pop("field")
        return run_batch(1.0, wls, 64, 4, field, [chain] * 2, **args)

    for bad in ([on], [on, on, on], [on, {"us": float("nan"), "ut": 0.0}], [on, {"us": 0.0, "ut": float("inf")}],
                [on, {"us": 0.0}], [on, "f1"], {"us": float("nan"), "ut": 0.0}, "f1", None):
        with pytest.raises(ValueError):
            rb(field=bad)
    det = Detector(8, 8, 1e-6)
    with pytest.raises(ValueError):
        rb(detector_origin="chief_ray")  # without a detector
    for bad in ("axis", np.zeros((3, 2)), np.zeros(2), [[0.0, 0.0], [float("nan"), 0.0]]):
        with pytest.raises(ValueError):
            rb(detector=det, detector_origin=bad, dev=DetectorModelDevice(64, 2))
    with pytest.raises(ValueError):
        run_broadband(1.0, wls, [1.0, 1.0], 64, 4, [on], chain, det)
    with pytest.raises(ValueError):
        run_broadband(1.0, wls, [1.0, 1.0], 64, 4, on, chain, det, detector_origin=np.zeros((3, 2)))
    # a single dict and a list of that dict: the same walk
    a = rb(field=on, outputs=("psf",))
    b = rb(field=[on, on], outputs=("psf",))
    assert all(np.array_equal(a[i][20]["psf"], b[i][20]["psf"]) for i in range(2))


def test_detector_placed_model_run_batch_weights():
    """run_batch with detector weights and per-item origins: the accumulated image is the item-by-item sum of the placed
    restatement, and a (B, 2) array is used as given."""
    from paos_amd.detector import Detector
    from paos_amd.run import run_batch

    pup, par, wls, fields, chains = _lens("Ariel_FGS-FGS1")
    n, nb = 64, 3
    fl = [fields[0], fields[1], SYNTH]
    dev = DetectorModelDevice(n, nb)
    det = Detector(20, 18, 2e-6, 2e-6, xc=1e-6)
    org = np.array([[0.0, 0.0], [3e-6, -1e-6], [-2.5e-6, 4e-6]])
    w = [0.5, 1.0, 2.0]
    res = run_batch(pup, [1e-6 * wls[0]] * nb, n, par["zoom"], fl, [chains[0]] * nb, outputs=(), dev=dev, keep_psf=True,
                    detector=det, detector_weights=w, detector_origin=org)
    last = list(chains[0].keys())[-1]
    want = detector_np.accumulate([detector_placed_np.rebin_placed(dev.psf_fetch(i), det, res[i][last]["dx"],
                                                                   res[i][last]["dy"], *org[i]) for i in range(nb)], w)
    assert np.array_equal(dev.detector_fetch(), want) and want.any()
    assert np.array_equal(dev.origins_seen[-1], org)


def _sharded_fields_worker(rank, world, key, out):
    import sys

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from fakes import ModelDevice
    from paos_amd.comm import Comm
    from paos_amd.dist import run_sharded
    from paos_amd.parse_config import parse_config

    comm = Comm(world, rank, 0, "socket", key=key, timeout=120)
    try:
        pup, par, wls, fields, chains = parse_config(os.path.join(LENS, "Ariel_FGS-FGS1.ini"))
        total = 5
        fl = [fields[k % 2] if k != 3 else SYNTH for k in range(total)]
        res = run_sharded(pup, [1e-6 * wls[0]] * total if rank == 0 else None, 64, par["zoom"],
                          fl if rank == 0 else None, [chains[0]] * total if rank == 0 else None, batch=2,
                          outputs=("psf",), make_device=lambda n, nb: ModelDevice(n, nb), comm=comm)
        last = list(chains[0].keys())[-1]
        out.put((rank, [(i, float(r[last]["power"])) for i, r in res],
                 {i: r[last]["psf"] for i, r in res if "psf" in r[last]}))
    finally:
        comm.close()


def test_run_sharded_per_item_fields_two_ranks():
    """run_sharded with one field per wavefront over the 2-rank TCP transport: the fields travel with the work and are
    sliced with the shards; every PSF equals run_batch's at the same field point."""
    from paos_amd.run import run_batch
    from test_abi_and_dist import _spawn

    results = _spawn(_sharded_fields_worker, 2)
    (_, all0, psf0), (_, all1, psf1) = results
    assert all0 == all1 and [i for i, _ in all0] == [0, 1, 2, 3, 4]
    assert sorted(psf0) == [0, 1, 2] and sorted(psf1) == [3, 4]
    pup, par, wls, fields, chains = _lens("Ariel_FGS-FGS1")
    last = list(chains[0].keys())[-1]
    psfs = {**psf0, **psf1}
    for k in range(5):
        f = fields[k % 2] if k != 3 else SYNTH
        want = run_batch(pup, [1e-6 * wls[0]], 64, par["zoom"], f, [chains[0]], outputs=("psf",), dev=ModelDevice(64, 1))
        assert np.array_equal(psfs[k], want[0][last]["psf"]), k
    assert not np.array_equal(psfs[0], psfs[1])


@pytest.mark.parametrize("name", ["Ariel_FGS-FGS1", "Ariel_AIRS-CH0"])
def test_lean_kept_psf_is_the_last_surface_psf(name):
    """A lean walk that keeps its PSFs stores them at the last surface -- also when only inert surfaces follow a surface
    that still propagates (FGS1: the last mirror 32 mm in front of the image plane, whose field is not the PSF)."""
    from oracle.run_np import run as oracle_run
    from paos_amd.run import run_batch

    pup, par, wls, fields, chains = _lens(name)
    n = 64
    last = list(chains[0].keys())[-1]
    for f in (fields[0], fields[1]):
        dev = ModelDevice(n, 1)
        run_batch(pup, [1e-6 * wls[0]], n, par["zoom"], f, [chains[0]], outputs=(), dev=dev, keep_psf=True)
        ref = oracle_run(pup, 1e-6 * wls[0], n, par["zoom"], f, chains[0], light=True)[last]
        assert rel_err(dev.psf_fetch(0), np.abs(ref["wfo"]) ** 2) < 1e-10
