"""Host logic without a GPU: the planner, the pass compiler and the batched run loop are
driven against a NumPy model of the device contract (tests/fakes.py) and compared with the
reference's golden vectors and the oracle."""
import copy
import os

import numpy as np
import pytest

from conftest import load_golden, rel_err
from fakes import ModelDevice
from oracle.run_np import run as oracle_run
from paos_amd import _lib
from paos_amd.chains import inject_wfe, read_wfe_table, syn20_chain, syn20_wavelength
from paos_amd.parse_config import parse_config
from paos_amd.planner import PilotBeam, jacobi_recurrence
from paos_amd.run import _Item, _walk

DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data")
FIELD = {"us": 0.0, "ut": 0.0}


def beam_scalars(b):
    return np.array([b.wl, b.z, b.w0, b.zw0, b.zr, b.dx, b.dy, b.C, b.fratio, b.wz, b.distancetofocus])


def test_pilot_beam_matches_reference_scalars():
    """PilotBeam vs the before/after scalars recorded from the reference's WFO."""
    g = load_golden("primitives.npz")
    for anam in (False, True):
        sfx = "_anam" if anam else ""

        def fresh():
            b = PilotBeam(1.0, 3.0e-6, 64, 4)
            if anam:
                b.magnification(1.25, 0.8)
            return b

        for fl in (10.0, -3.0, 0.4):
            b = fresh()
            assert np.array_equal(beam_scalars(b), g[f"lens_{fl}{sfx}_before"])
            b.lens(fl)
            assert np.array_equal(beam_scalars(b), g[f"lens_{fl}{sfx}_after"])
        for dz in (0.5, -0.25, 1.0e-8):
            b = fresh()
            b.ptp(dz)
            assert np.array_equal(beam_scalars(b), g[f"ptp_{dz}{sfx}_after"])
        for fl in (10.0, -7.0):
            b = fresh()
            b.lens(fl)
            blk, inv = b.stw(b.zw0 - b.z)
            assert np.array_equal(beam_scalars(b), g[f"stw_{fl}{sfx}_after"])
            assert inv == (g[f"stw_{fl}{sfx}_dz"] < 0) and blk[0] == 1.0
        for dz in (2.0, -1.5):
            b = fresh()
            blk, inv = b.wts(dz)
            assert np.array_equal(beam_scalars(b), g[f"wts_{dz}{sfx}_after"]) and inv == (dz < 0)
    b = PilotBeam(1.0, 3.0e-6, 64, 4)
    assert b.ptp(1e-10) is None and b.z == 0.0  # below wl/1000: reference returns early
    b.lens(10.0)
    with pytest.raises(ValueError):
        b.ptp(1.0)
    with pytest.raises(ValueError):
        PilotBeam(1.0, 3.0e-6, 64, 4).stw(1.0)
    for tag, (fl, dist) in {"II": (None, 1.0), "OI": (10.0, 10.0), "IO": (None, 4.0e6), "OO": (10.0, 20.0)}.items():
        b = PilotBeam(1.0, 3.0e-6, 64, 4)
        if fl:
            b.lens(fl)
        steps = b.propagate(dist)
        assert b.propagator == tag
        # IO from the waist itself: the leading ptp(0) is below wl/1000 and is skipped (wfo.py:454)
        assert [s[0] for s in steps] == {"II": ["ptp"], "OI": ["stw", "ptp"], "IO": ["wts"], "OO": ["stw", "wts"]}[tag]
        assert np.array_equal(beam_scalars(b), g["propagate_" + tag + "_after"])


def _model_run(spec, n, chains=None, wls=None):
    chains = chains or [spec["chain"]]
    wls = wls or [spec["wl"]]
    dev = ModelDevice(n, len(chains))
    states = [_Item(spec["pup"], wl, n, spec["zoom"], spec["field"]) for wl in wls]
    saved = {}

    def on_saved(key, items, plans, wfe):
        for i, (it, pl) in enumerate(zip(items, plans)):
            if it["save"]:
                saved.setdefault(i, {})[it["num"]] = dict(pl["scalars"], wfo=dev.download(i), wfe=wfe)

    stats = {}
    _walk(dev, states, chains, on_saved, stats=stats, fresh=1.0 + 0.0j)
    return saved, dev, stats


def _spec(name):
    if name == "SYN20":
        return dict(pup=1.0, wl=1.0e-6, zoom=4, field=FIELD, chain=syn20_chain())
    pup, par, wls, fields, chains = parse_config(os.path.join(DATA, "lens", name + ".ini"))
    return dict(pup=pup, wl=1.0e-6 * wls[0], zoom=par["zoom"], field=fields[0], chain=chains[0])


@pytest.mark.parametrize("name", ["SYN20", "Hubble_simple", "Excite_TEL", "Ariel_AIRS-CH0", "Ariel_FGS-FGS1"])
def test_fused_pass_programs_reproduce_reference(name):
    """Planner + pass compiler + NumPy model of the pass semantics == the reference's run()
    outputs: validates the operator fusion and axis alternation logic on the CPU."""
    spec = _spec(name)
    gs = load_golden(f"scalars_{name}.npz")
    chain = copy.deepcopy(spec["chain"])
    for item in chain.values():
        item["save"] = True
    saved, _, _ = _model_run(dict(spec, chain=chain), 64)
    for row, k in zip(gs["table"], gs["nums"]):
        s = saved[0][k]
        got = [s["wl"], s["dx"], s["dy"], s["wz"], s["distancetofocus"], s["fratio"]]
        assert np.array_equal(got, row), (name, k)
    assert [saved[0][k]["propagator"] for k in gs["nums"]] == list(gs["propagator"])

    gr = load_golden(f"run_{name}.npz")
    n = int(gr["gridsize"])
    saved, dev, stats = _model_run(spec, n)
    for k in gr["nums"]:
        assert rel_err(saved[0][k]["wfo"], gr[f"S{k:02d}_wfo"]) < 1e-12, (name, k)
    assert stats["fused_passes"] == dev.pass_count


def test_syn20_pass_budget():
    """SURVEY 8d counts 43 2-D FFTs for SYN20 (16 ptp, 6 stw, 5 wts); fused they take 29 HBM
    passes + 7 stand-alone aperture passes (unfused: 70 transform + 11 lens + 7 aperture), or
    24 passes in all when the apertures ride on passes too (PAOS_FUSE_APERTURES=1).  Round 3: each of the five
    relays has two ptp in a row at its focus (OI then IO: ptp(+1.6 nm), ptp(-1.6 nm)); since fft2(ifft2(X)) = X
    the second joins the first one's middle pass, and since H(-d) H(d) = 1 the pair goes altogether and the stw in
    front meets the wts behind in one pass: four passes less per relay, 49 -> 29 and 44 -> 24."""
    import paos_amd.run as prun

    prun.FUSE_APERTURES = False
    try:
        _, dev, stats = _model_run(_spec("SYN20"), 64)
    finally:
        prun.FUSE_APERTURES = "auto"
    assert stats["fused_passes"] == dev.pass_count == 29
    kinds = [name for name, _ in dev.log]
    # the first surface (ones -> aperture -> stop) is one "start" launch
    assert kinds.count("start") == 1 and kinds.count("aperture") == 6 and kinds.count("make_stop") == 0
    assert kinds.count("zernike") == 1 and kinds.count("fill") == 0
    assert -1 not in [d for name, d in dev.log if name == "pass"]  # every lens rides on a transform
    prun.FUSE_APERTURES = True
    try:
        saved, dev, stats = _model_run(_spec("SYN20"), 64)
    finally:
        prun.FUSE_APERTURES = "auto"
    kinds = [name for name, _ in dev.log]
    assert kinds.count("aperture") == 0 and kinds.count("start") == 1 and stats["fused_passes"] == 24
    gr = load_golden("run_SYN20.npz")
    saved, _, _ = _model_run(_spec("SYN20"), 128)
    prun.FUSE_APERTURES = True
    try:
        fused, _, _ = _model_run(_spec("SYN20"), 128)
    finally:
        prun.FUSE_APERTURES = "auto"
    for k in gr["nums"]:
        assert rel_err(fused[0][k]["wfo"], gr[f"S{k:02d}_wfo"]) < 1e-12
        assert rel_err(fused[0][k]["wfo"], saved[0][k]["wfo"]) < 1e-13


def _two_regime_chain():
    """lens f = 10 m, stop 0.5 mm short of focus, then on to focus: the first hop is OO at
    1 um (2 zr = 0.25 mm) but OI at 10 um (2 zr = 2.5 mm)."""
    from paos_amd.abcd import ABCD

    def item(num, kind, name, thickness=0.0, curvature=0.0, **extra):
        d = {"num": num, "type": kind, "name": name, "is_stop": False, "save": False,
             "ABCDt": ABCD(thickness=thickness, curvature=curvature),
             "ABCDs": ABCD(thickness=thickness, curvature=curvature)}
        d.update(extra)
        return d

    pupil = {"shape": "elliptical", "type": "aperture", "xrad": 0.5, "yrad": 0.5, "xc": 0.0, "yc": 0.0}
    return {1: item(1, "Standard", "STOP", is_stop=True, aperture=pupil),
            2: item(2, "Paraxial Lens", "L", thickness=10.0 - 5.0e-4, curvature=0.1),
            3: item(3, "Standard", "NEAR", thickness=5.0e-4, save=True),
            4: item(4, "Standard", "IMAGE_PLANE", save=True)}


def test_batched_walk_matches_itemwise_oracle():
    """Batches whose items disagree share one pass sequence: different wavelengths and WFE
    draws through SYN20, and a chain whose propagator regime flips with wavelength (one
    item runs stw+wts where the other runs stw+ptp in the same launches)."""
    _, _, _, table = read_wfe_table(os.path.join(DATA, "wfe", "wfe_realization_SN20210914.csv"))
    wls = [syn20_wavelength(0), syn20_wavelength(300), 7.0e-6]
    chains = [inject_wfe(syn20_chain(), table[:, k]) for k in range(3)]
    spec = dict(pup=1.0, zoom=4, field=FIELD)
    saved, _, _ = _model_run(spec, 64, chains=chains, wls=wls)
    for i in range(3):
        ref = oracle_run(1.0, wls[i], 64, 4, FIELD, chains[i], light=True)
        for k in ref:
            assert rel_err(saved[i][k]["wfo"], ref[k]["wfo"]) < 1e-12, (i, k)
            assert saved[i][k]["dx"] == ref[k]["dx"] and saved[i][k]["propagator"] == ref[k]["propagator"]

    wls = [1.0e-6, 1.0e-5]
    chains = [_two_regime_chain(), _two_regime_chain()]
    saved, _, _ = _model_run(spec, 64, chains=chains, wls=wls)
    props = []
    for i in range(2):
        ref = oracle_run(1.0, wls[i], 64, 4, FIELD, chains[i], light=True)
        props.append(ref[3]["propagator"])
        for k in ref:
            assert rel_err(saved[i][k]["wfo"], ref[k]["wfo"]) < 1e-12, (i, k)
            assert saved[i][k]["propagator"] == ref[k]["propagator"] and saved[i][k]["dx"] == ref[k]["dx"]
    assert props == ["OO", "OI"]


def test_jacobi_recurrence_matches_scipy():
    from scipy.special import eval_jacobi

    tab = jacobi_recurrence(12)
    x = np.linspace(-1, 1, 41)
    for a in range(13):
        pkm1, pk = np.zeros_like(x), np.ones_like(x)
        for k in range(0, (12 - a) // 2 + 1):
            if k > 0:
                A, B, C = tab[a, k]
                pkm1, pk = pk, (A * x + B) * pk - C * pkm1
            assert np.max(np.abs(pk - eval_jacobi(k, a, 0.0, x))) < 1e-12 * max(1.0, np.max(np.abs(pk)))


def test_run_passes_rejects_oversized_slots():
    from paos_amd.passes import PassCompiler

    comp = PassCompiler(1, 64)
    blk = [[1.0, 1e-3, 1e-3, 0.5, -1.0]]
    for _ in range(9):  # many lenses in a row overflow one pass slot -> extra stand-alone passes
        comp.lens(blk)
    comp.ptp([[1.0, 1.0, 1.0, 1e-3, -1.0]])
    passes, blocks = comp.program()
    assert all(len(p.get(s, ())) <= _lib.MAX_PW for p in passes for s in ("pre", "mid", "post"))
    assert sum(1 for p in passes if p["axis"] == -1) >= 1
    assert blocks.shape[1:] == (1, 5)


def test_zorthonorm_host_logic_reproduces_reference():
    """Zorthonorm (run.py:133-141, PolyOrthoNorm zernike.py:320-402) through the product's host
    logic -- Gram sums -> covariance -> M = inv(chol) -> transformed coefficients -> ordinary
    expansion inside the pupil -- equals the reference's run() output."""
    from paos_amd.chains import syn20_orthonorm_chain

    g = load_golden("orthonorm.npz")
    for n in (64, 128):
        chain = syn20_orthonorm_chain()
        chain[2]["save"] = True
        saved, dev, _ = _model_run(dict(pup=1.0, wl=1.0e-6, zoom=4, field=FIELD, chain=chain), n)
        wfe = saved[0][2]["wfe"]
        assert np.array_equal(np.isnan(wfe), g[f"run{n}_S02_wfe_mask"])
        assert rel_err(np.nan_to_num(wfe), g[f"run{n}_S02_wfe"]) < 1e-12
        assert rel_err(saved[0][2]["wfo"], g[f"run{n}_S02_wfo"]) < 1e-12
        assert rel_err(saved[0][20]["wfo"], g[f"run{n}_S20_wfo"]) < 1e-12
        assert ("pupil_aperture", _lib.SHAPE_ELLIPSE) in dev.log and ("zernike_gram", 36) in dev.log


def test_orthonorm_matrix_matches_reference():
    from paos_amd.planner import gram_polynomials, orthonorm_matrix
    from paos_amd.zernike import Zernike, norm_factors

    g = load_golden("orthonorm.npz")
    for ordering in ("noll", "ansi"):
        m, nn = Zernike.j2mn(15, ordering)
        norm = norm_factors(m, nn, True)
        # covariance -> M from the reference's own covariance (its masked means times the pixel count)
        cov = g[f"poly_{ordering}_cov"]
        iu = np.triu_indices(15)
        count = float((~g["poly_mask"] & (g["poly_rho"] <= 1.0)).sum())
        M = orthonorm_matrix(cov[iu] * count, count, 15)
        assert np.allclose(M, g[f"poly_{ordering}_M"], rtol=1e-9, atol=1e-12)
        assert gram_polynomials(m, nn, norm).shape == (15, 4)


@pytest.mark.parametrize("name", ["Ariel_AIRS-CH1", "Ariel_FGS-FGS2", "Ariel_FGS-NIRSpec", "Ariel_FGS-VISPhot",
                                  "lens_file_TA_Ground", "lens_file_TA_OGSE_Ground", "lens_file_template",
                                  "periscope"])
def test_remaining_lens_files_through_the_pass_compiler(name):
    g = load_golden("run_more_chains.npz")
    pup, par, wls, fields, chains = parse_config(os.path.join(DATA, "lens", name + ".ini"))
    for tag, iw in (("first", 0), ("last", len(wls) - 1)):
        key = f"{name}_{tag}"
        spec = dict(pup=pup, wl=1.0e-6 * wls[iw], zoom=par["zoom"], field=fields[0], chain=chains[iw])
        saved, _, _ = _model_run(spec, 64)
        nums = sorted(saved[0].keys())
        assert np.array_equal(nums, g[key + "_nums"])
        table = np.array([[saved[0][k][f] for f in ("wl", "dx", "dy", "wz", "distancetofocus", "fratio")]
                          for k in nums])
        assert np.array_equal(table, g[key + "_table"]), key
        assert [saved[0][k]["propagator"] for k in nums] == list(g[key + "_propagator"])
        assert rel_err(saved[0][nums[-1]]["wfo"], g[key + "_wfo"]) < 1e-12, key


def test_package_exports_resolve_lazily():
    import importlib

    import paos_amd

    for name in paos_amd.__all__:
        assert getattr(paos_amd, name) is not None, name
    assert callable(paos_amd.run_batch) and callable(paos_amd.run_sharded)
    assert callable(importlib.import_module("paos_amd.run").run)
    with pytest.raises(AttributeError):
        paos_amd.no_such_thing


def test_lean_walk_skips_dead_rows_and_ends_on_the_psf():
    """run_batch that hands back no arrays (outputs=(), the benchmark's mode): the first field write leaves the
    rows outside the aperture's box unwritten (the model device fills them with NaN, so any read would show), the
    power of the first surface is summed over the live rows, and the last pass stores |u|^2 instead of the field.
    Powers and PSFs equal those of the ordinary walk and of the oracle."""
    from fakes import ModelDevice
    from oracle.run_np import run as oracle_run
    from paos_amd.chains import syn20_chain, syn20_wavelength
    import paos_amd.run as prun
    from paos_amd.run import run_batch

    wls = [syn20_wavelength(0), syn20_wavelength(300)]
    chains = [syn20_chain(), syn20_chain()]
    field = {"us": 0.0, "ut": 0.0}
    prun.FUSE_APERTURES = True  # as at the production sizes: the field stop rides on the last pass
    try:
        _lean_walk_checks(ModelDevice, oracle_run, run_batch, syn20_chain, wls, chains, field)
    finally:
        prun.FUSE_APERTURES = "auto"


def _lean_walk_checks(ModelDevice, oracle_run, run_batch, syn20_chain, wls, chains, field):
    plain_dev = ModelDevice(128, 2)
    plain = run_batch(1.0, wls, 128, 4, field, chains, outputs=("psf",), dev=plain_dev, keep_psf=True)
    dev = ModelDevice(128, 2)
    lean = run_batch(1.0, wls, 128, 4, field, chains, outputs=(), dev=dev, keep_psf=True)
    kinds = [name for name, _ in dev.log]
    assert kinds.count("psf_store") == 1 and kinds.count("psf_keep") == 0
    assert "zero_outside_rows" not in kinds  # the first pass program consumed the rows that stood for zeros
    assert np.isnan(dev.u).all()  # the field was given up for its PSF
    for i in range(2):
        for k in (1, 20):
            assert np.isfinite(lean[i][k]["power"])
            assert abs(lean[i][k]["power"] - plain[i][k]["power"]) <= 1e-13 * plain[i][k]["power"]
        assert np.allclose(dev.psf_fetch(i), plain[i][20]["psf"], rtol=0, atol=1e-13 * plain[i][20]["psf"].max())
    ref = oracle_run(1.0, wls[1], 128, 4, field, syn20_chain(), light=True)
    psf = ref[20]["amplitude"] ** 2
    assert np.max(np.abs(dev.psf_fetch(1) - psf)) < 1e-11 * psf.max()
    # power=False: the fused store's ticket is handed back, nothing else changes
    dev2 = ModelDevice(128, 2)
    run_batch(1.0, wls, 128, 4, field, chains, outputs=(), dev=dev2, keep_psf=True, power=False)
    assert np.array_equal(dev2.psf_fetch(0), dev.psf_fetch(0))
    # a chain whose second surface is a stop: the rows that stand for zeros are cleared before the sum reads them
    chain = syn20_chain()
    chain[2] = dict(chain[2], is_stop=True)
    dev3 = ModelDevice(128, 1)
    got = run_batch(1.0, wls[:1], 128, 4, field, [chain], outputs=(), dev=dev3, keep_psf=True)
    assert [name for name, _ in dev3.log].count("zero_outside_rows") == 1
    want = run_batch(1.0, wls[:1], 128, 4, field, [chain], outputs=("psf",), dev=ModelDevice(128, 1), keep_psf=True)
    assert abs(got[0][20]["power"] - want[0][20]["power"]) <= 1e-13 * want[0][20]["power"]


def test_consecutive_ptp_merge_into_one_middle_pass():
    """ptp . ptp = F^-1 (H2 H1) F: the pass compiler drops the inverse / forward transform pair between two
    ptp that follow each other directly.  Against the oracle's two separate ptp (wfo.py:445-472) on a random
    field, with items that take both, only the first, only the second, or neither; a lens or an aperture in
    between keeps them apart; a fourth ptp in a row starts a new group (three phases per pass at most)."""
    from fakes import ModelDevice
    from oracle.pop_numpy import RefWFO
    from paos_amd import _lib
    from paos_amd.passes import PassCompiler
    from paos_amd.planner import PilotBeam

    n, nb = 64, 4
    rng = np.random.default_rng(11)
    u0 = rng.standard_normal((nb, n, n)) + 1j * rng.standard_normal((nb, n, n))
    takes = [(True, True), (True, False), (False, True), (False, False)]
    dz = (0.7, 1.9)
    beams = [PilotBeam(1.0, 1.0e-6 * (1 + 0.1 * i), n, 4) for i in range(nb)]
    dev = ModelDevice(n, nb)
    dev.u[:] = u0
    comp = PassCompiler(nb, n)
    for k in range(2):
        comp.ptp([beams[i].ptp(dz[k]) if takes[i][k] else None for i in range(nb)])
    assert len(comp.passes) == 3 and sum(op[0] == _lib.PW_QPHASE_NATURAL for op in comp.passes[1]["mid"]) == 2
    comp.flush(dev)
    for i in range(nb):
        w = RefWFO(1.0, 1.0e-6 * (1 + 0.1 * i), n, 4)
        w._wfo = u0[i].copy()
        for k in range(2):
            if takes[i][k]:
                w.ptp(dz[k])
        assert rel_err(dev.u[i], w._wfo) < 1e-13, i
    # ptp(+d) then ptp(-d): the pair is the identity and leaves no pass behind -- for every item or not at all
    comp = PassCompiler(nb, n)
    comp.stw([beams[i].ptp(0.3) for i in range(nb)], [False] * nb)  # (any block will do for the structure)
    before = len(comp.passes)
    fwd = [beams[i].ptp(2.0e-9 * (i + 1)) if i != 3 else None for i in range(nb)]
    back = [beams[i].ptp(-2.0e-9 * (i + 1)) if i != 3 else None for i in range(nb)]
    assert all(b is None or b[3] == -f[3] for f, b in zip(fwd, back))
    comp.ptp(fwd)
    assert len(comp.passes) == before + 2
    comp.ptp(back)
    assert len(comp.passes) == before and comp.open is comp.passes[-1] and comp.open["fft2"] == -1
    comp.ptp(fwd)
    odd = [list(b) if b is not None else None for b in back]
    odd[1][3] *= 1.0000001  # one item whose second step is not the exact inverse: the pair stays, merged
    comp.ptp(odd)
    assert len(comp.passes) == before + 2
    assert sum(op[0] == _lib.PW_QPHASE_NATURAL for op in comp.passes[-2]["mid"]) == 2
    dev = ModelDevice(n, nb)
    dev.u[:] = u0
    comp = PassCompiler(nb, n)
    comp.ptp(fwd)
    comp.ptp(back)
    assert not comp.pending() or not comp.program()[0]
    # something between two ptp: no merge
    comp = PassCompiler(1, n)
    comp.ptp([beams[0].ptp(1.0)])
    comp.lens([[1.0, beams[0].dx, beams[0].dy, 0.5 / 1.0e-6 * 0.1, -1.0]])
    comp.ptp([beams[0].ptp(1.0)])
    assert len(comp.program()[0]) == 5
    # four in a row: 3 + 1
    comp = PassCompiler(1, n)
    for _ in range(4):
        comp.ptp([beams[0].ptp(0.5)])
    prog = comp.program()[0]
    assert len(prog) == 5
    assert [sum(op[0] == _lib.PW_QPHASE_NATURAL for op in p["mid"]) for p in prog] == [0, 3, 0, 1, 0]


def test_ptp_algebra_switch():
    """PAOS_PTP_ALGEBRA=0 / passes.PTP_ALGEBRA = False: every ptp of the reference runs as its own three passes
    (SYN20: 44 with the apertures riding) -- same fields to rounding as the 24-pass program."""
    import paos_amd.passes as ppasses
    import paos_amd.run as prun

    prun.FUSE_APERTURES = True
    try:
        fast, _, stats_fast = _model_run(_spec("SYN20"), 128)
        ppasses.PTP_ALGEBRA = False
        try:
            plain, _, stats_plain = _model_run(_spec("SYN20"), 128)
        finally:
            ppasses.PTP_ALGEBRA = True
    finally:
        prun.FUSE_APERTURES = "auto"
    assert stats_fast["fused_passes"] == 24 and stats_plain["fused_passes"] == 44
    for k in fast[0]:
        assert rel_err(fast[0][k]["wfo"], plain[0][k]["wfo"]) < 1e-13


@pytest.mark.parametrize("name,fewer", [("Ariel_FGS-FGS1", 8), ("Ariel_FGS-FGS2", None), ("Ariel_AIRS-CH0", 0),
                                        ("Excite_TEL", None), ("Hubble_simple", None)])
def test_a_wts_and_the_stw_that_undoes_it_cancel(name, fewer):
    """Two outside-to-outside hops in a row with nothing between them (the flat windows of the Ariel FGS channels):
    the wts that ends the first and the stw that starts the second are each other's inverse and go (passes.py:
    _single / _undoes).  Needs a stretch without saved surfaces, i.e. ``light_output``: the image plane of the
    fused program against the chain with the identities off, and -- through the other tests of this file, which
    pin that configuration to the reference -- against the reference."""
    import paos_amd.passes as ppasses
    import paos_amd.run as prun

    spec = _spec(name)
    chain = copy.deepcopy(spec["chain"])
    for item in chain.values():
        item["save"] = item["name"] == "IMAGE_PLANE"
    spec = dict(spec, chain=chain)
    prun.FUSE_APERTURES = True
    try:
        fast, _, stats_fast = _model_run(spec, 128)
        ppasses.PTP_ALGEBRA = False
        try:
            plain, _, stats_plain = _model_run(spec, 128)
        finally:
            ppasses.PTP_ALGEBRA = True
    finally:
        prun.FUSE_APERTURES = "auto"
    (k,) = fast[0]
    assert rel_err(fast[0][k]["wfo"], plain[0][k]["wfo"]) < 1e-11, name
    if fewer is not None:
        assert stats_plain["fused_passes"] - stats_fast["fused_passes"] >= fewer, (stats_plain, stats_fast)
    print(name, stats_plain["fused_passes"], "->", stats_fast["fused_passes"],
          "image-plane difference", rel_err(fast[0][k]["wfo"], plain[0][k]["wfo"]))


def test_undoes_needs_opposite_directions_equal_items_and_cancelling_phases():
    from paos_amd.passes import PassCompiler

    comp = PassCompiler(2, 256)
    # dz = 0.5 m, lambda = 1 um, dx at the critical sampling of the chirp (dx^2 = lambda dz / N: the corner phase is
    # pi N / 2 = 402 rad, its coefficient's rounding noise ~1e-13 rad -- an undersampled 1 mm grid would carry 2e5 rad
    # and 2e-11 rad of noise, above UNDO_MAX_RESIDUAL: such a pair keeps both operators, which is always correct)
    dx = (1e-6 * 0.5 / 256) ** 0.5
    wts = np.array([[1.0, dx, dx, np.pi / (0.5 * 1e-6), 1.0]] * 2)
    dxn = 1e-6 * 0.5 / (256 * dx)
    fs = 1.0 / (256 * dxn)
    stw = np.array([[1.0, fs, fs, np.pi * 1e-6 * -0.5, 1.0]] * 2)
    fwd, inv = np.zeros(2), np.ones(2)
    assert comp._undoes(wts, fwd, stw, inv)
    assert not comp._undoes(wts, fwd, stw, fwd)                      # same direction: a coordinate flip, not the identity
    assert not comp._undoes(wts, np.array([0.0, 1.0]), stw, inv)     # one item disagrees
    off = stw.copy(); off[1, 0] = 0.0
    assert not comp._undoes(wts, fwd, off, inv)                      # not the same items
    far = stw.copy(); far[:, 3] *= 1.001
    assert not comp._undoes(wts, fwd, far, inv)                      # another distance: radians of residual phase
    # through the operator interface: wts then stw cancel, a lens between them keeps both
    comp.stw(stw * [1, 1, 1, -1, 1], fwd)
    n0 = len(comp.passes)
    comp.wts(wts, fwd)
    comp.stw(stw, inv)
    assert len(comp.passes) == n0 and comp.open is comp.passes[-1]
    comp.wts(wts, fwd)
    comp.lens(np.array([[1.0, dx, dx, 0.25, 1.0]] * 2))
    comp.stw(stw, inv)
    assert len(comp.passes) == n0 + 2


def test_undoes_threshold_sits_a_decade_inside_the_parity_gate():
    """VERDICT r03 "weak" 2: the residual phase a dropped wts -> stw pair may leave is bounded by the field gate the
    parity tests assert (1e-10) / 10.  A pair whose corner residual is 1e-10 rad must NOT cancel, one at
    1e-13 rad (rounding noise of separately rounded coefficients) must."""
    import paos_amd.passes as ppasses
    from paos_amd.passes import PassCompiler

    assert ppasses.UNDO_MAX_RESIDUAL <= 1.0e-11 and ppasses.UNDO_MAX_RESIDUAL <= ppasses.PARITY_GATE / 10.0
    n = 256
    comp = PassCompiler(1, n)
    wts = np.array([[1.0, 1e-3, 1e-3, np.pi / (0.5 * 1e-6), 1.0]])
    dxn = 1e-6 * 0.5 / (n * 1e-3)
    fs = 1.0 / (n * dxn)
    fwd, inv = np.zeros(1), np.ones(1)
    half = (n / 2.0) ** 2

    def stw_with_residual(target):
        """stw block whose coefficient leaves ``target`` rad at the corner against ``wts`` (x and y alike)."""
        cw = wts[0, 3] * wts[0, 4] * wts[0, 1] ** 2          # per-pixel^2 coefficient of the wts phase
        c = (target / (2.0 * half) - cw) / fs ** 2            # ... so that (cw + c fs^2) * 2 half = target
        blk = np.array([[1.0, fs, fs, c, 1.0]])
        got = 2.0 * abs(blk[0, 3] * blk[0, 4] * blk[0, 1] ** 2 + cw) * half
        return blk, got

    corner = abs(wts[0, 3] * wts[0, 1] ** 2) * 2.0 * half      # ~2e5 rad: ulp ~ 3e-11, so targets are met to ~1e-11
    assert corner > 1e3
    above, got_above = stw_with_residual(1.0e-10 * 4.0)        # well above the threshold whatever the rounding
    assert got_above > ppasses.UNDO_MAX_RESIDUAL
    assert not comp._undoes(wts, fwd, above, inv)
    # exactly representable cancellation (residual 0) and an explicit 1e-13 through the max_residual argument's default
    exact = np.array([[1.0, wts[0, 1], wts[0, 2], -wts[0, 3], 1.0]])
    assert comp._undoes(wts, fwd, exact, inv)
    # a small-phase pair, where 1e-13 and 1e-10 are far above the coefficient's ulp: both sides of the threshold
    small = np.array([[1.0, 1e-3, 1e-3, 1.0, 1.0]])           # corner phase 2 * 128^2 * 1e-6 = 0.033 rad
    cw = small[0, 3] * small[0, 1] ** 2
    for target, cancels in ((1.0e-13, True), (5.0e-12, True), (1.0e-10, False), (1.0e-9 * 0.5, False)):
        c = target / (2.0 * half) - cw
        blk = np.array([[1.0, 1.0, 1.0, c, 1.0]])
        resid = 2.0 * abs(c + cw) * half
        assert abs(resid - target) < 1e-3 * target, (resid, target)
        assert comp._undoes(small, fwd, blk, inv) is cancels, (target, resid)
    # through the operator interface: the 1e-13 pair leaves nothing; the 1e-10 pair loses its transforms (exact
    # inverses whatever the phases do) but its residual phase is KEPT as a diagonal operator -- nothing above the
    # threshold is dropped; a pair that leaves 1e-5 rad is no inverse pair and keeps both operators (two more passes)
    for target, extra, kept in ((1.0e-13, 0, 0), (1.0e-10, 0, 1), (1.0e-5, 2, 0)):
        comp = PassCompiler(1, n)
        comp.stw(np.array([[1.0, 1.0, 1.0, -0.5, 1.0]]), fwd)
        n0 = len(comp.passes)
        comp.wts(small, fwd)
        comp.stw(np.array([[1.0, 1.0, 1.0, target / (2.0 * half) - cw, 1.0]]), inv)
        assert len(comp.passes) == n0 + extra, (target, len(comp.passes), n0)
        if extra == 0:
            assert len(comp.tail) == kept, (target, comp.tail)
            if kept:
                blk = comp.blocks[comp.tail[0][2]][0]
                left = blk[4] * blk[3] * (blk[1] ** 2 + blk[2] ** 2) * half  # phase at the corner
                assert abs(left - target) < 1e-3 * target, (left, target)


def _short_chain(surfaces):
    """The first ``surfaces`` of a STOP | flat (thickness 0) ... | IMAGE_PLANE prescription: no hop ever exceeds
    lambda / 1000, so no pass program runs between the start field and the saved last surface."""
    from paos_amd.abcd import ABCD

    chain = {1: {"num": 1, "type": "Standard", "name": "STOP", "is_stop": True, "save": True,
                 "aperture": {"shape": "elliptical", "type": "aperture", "xrad": 0.5, "yrad": 0.5, "xc": 0.0, "yc": 0.0},
                 "ABCDt": ABCD(thickness=0.0, curvature=0.0), "ABCDs": ABCD(thickness=0.0, curvature=0.0)}}
    for num in range(2, surfaces + 1):
        chain[num] = {"num": num, "type": "Standard", "name": "IMAGE_PLANE" if num == surfaces else f"FLAT{num}",
                      "is_stop": False, "save": num == surfaces,
                      "ABCDt": ABCD(thickness=0.0, curvature=0.0), "ABCDs": ABCD(thickness=0.0, curvature=0.0)}
    return chain


@pytest.mark.parametrize("surfaces", [1, 3])
def test_lean_walk_that_keeps_the_psf_without_any_pass_program(surfaces):
    """a lean walk (outputs=(), keep_psf=True) whose saved last surface is reached before any
    pass program has consumed the rows that merely stand for zeros -- a single-surface chain, or a chain of hops
    shorter than lambda / 1000 -- takes |u|^2 of the whole field (psf_keep / psf_keep_power).  The model device holds
    NaN in those rows: power and PSF must be finite and equal to the ordinary walk's."""
    from paos_amd.run import run_batch

    n, wl, field = 128, 1.0e-6, {"us": 0.0, "ut": 0.0}
    chain = _short_chain(surfaces)
    last = surfaces
    want_dev = ModelDevice(n, 1)
    want = run_batch(1.0, [wl], n, 4, field, [chain], outputs=("psf",), dev=want_dev, keep_psf=True)
    for power in (True, False):
        dev = ModelDevice(n, 1)
        got = run_batch(1.0, [wl], n, 4, field, [chain], outputs=(), dev=dev, keep_psf=True, power=power)
        kinds = [name for name, _ in dev.log]
        assert "zero_outside_rows" in kinds, kinds  # the rows were stale (lean start) and had to become zeros
        psf = dev.psf_fetch(0)
        assert np.isfinite(psf).all()
        assert np.array_equal(psf, want[0][last]["psf"])
        if power:
            assert np.isfinite(got[0][last]["power"])
            assert abs(got[0][last]["power"] - want[0][last]["power"]) <= 1e-13 * want[0][last]["power"]
            assert abs(got[0][last]["power"] - 1.0) < 1e-12  # behind the stop the power is 1


def _random_chain(rng, surfaces):
    """A random prescription of lenses, gaps, (re-)imaging relays, nanometre hops past a focus and flat windows,
    with apertures sprinkled in: every operator order the planner can produce (II / OI / IO / OO, skipped hops,
    ptp pairs that cancel or merge, wts -> stw pairs that undo each other) shows up over a few draws."""
    from paos_amd.abcd import ABCD

    def surf(num, kind, name, thickness=0.0, curvature=0.0, **extra):
        item = {"num": num, "type": kind, "name": name, "is_stop": False, "save": False,
                "ABCDt": ABCD(thickness=thickness, curvature=curvature), "ABCDs": ABCD(thickness=thickness, curvature=curvature)}
        item.update(extra)
        return item

    pupil = {"shape": "elliptical", "type": "aperture", "xrad": 0.5, "yrad": 0.5, "xc": 0.0, "yc": 0.0}
    chain = {1: surf(1, "Standard", "STOP", is_stop=True, save=True, aperture=pupil)}
    f = 10.0
    while len(chain) < surfaces - 1:
        num = len(chain) + 1
        kind = rng.integers(0, 6)
        if kind == 0:    # focusing lens, propagate to (a hair past) its focus
            chain[num] = surf(num, "Paraxial Lens", f"L{num}", thickness=f + float(rng.choice([0.0, 1.6e-9, -1.6e-9, 3.0e-4])), curvature=1.0 / f)
        elif kind == 1:  # free space
            chain[num] = surf(num, "Standard", f"D{num}", thickness=float(rng.choice([f, 0.1, 2.0e-9, 0.0, -1.6e-9])))
        elif kind == 2:  # flat window: two outside-to-outside hops in a row come out of these
            chain[num] = surf(num, "Standard", f"W{num}", thickness=float(rng.choice([0.5, 1.0, 0.25])))
        elif kind == 3:  # collimating lens with an aperture
            chain[num] = surf(num, "Paraxial Lens", f"C{num}", thickness=0.1, curvature=1.0 / f, aperture=pupil)
        elif kind == 4:  # weak lens
            chain[num] = surf(num, "Paraxial Lens", f"Q{num}", thickness=float(rng.choice([0.3, 3.0])), curvature=1.0 / float(rng.choice([40.0, -25.0])))
        else:            # a saved flat
            chain[num] = surf(num, "Standard", f"S{num}", thickness=0.0, save=bool(rng.integers(0, 2)))
    num = len(chain) + 1
    chain[num] = surf(num, "Standard", "IMAGE_PLANE", save=True)
    return chain


@pytest.mark.parametrize("seed", range(12))
def test_ptp_algebra_on_and_off_agree_on_random_chains(seed):
    """the compiler's three rewrites (consecutive ptp share a middle pass, ptp(+d) ptp(-d) cancel, a
    wts and the stw that undoes it cancel) pinned beyond SYN20-like chains: random prescriptions, two wavelengths per
    batch (so items may disagree about which hops they take), compiled with PTP_ALGEBRA on and off, run on the NumPy
    model of the device, every saved surface equal to ~1e-12."""
    import paos_amd.passes as ppasses
    import paos_amd.run as prun

    rng = np.random.default_rng(1000 + seed)
    chain = _random_chain(rng, int(rng.integers(6, 14)))
    wls = [1.0e-6, float(rng.choice([1.0e-6, 1.7e-6, 2.3e-6]))]
    spec = dict(pup=1.0, wl=wls[0], zoom=4, field=FIELD, chain=chain)
    prun.FUSE_APERTURES = bool(rng.integers(0, 2)) or "auto"
    try:
        try:
            fast, _, st_fast = _model_run(spec, 64, chains=[chain, chain], wls=wls)
        except (ValueError, AssertionError, TypeError) as exc:
            pytest.skip(f"the planner refuses this draw like the reference would ({type(exc).__name__}: {exc})")
        ppasses.PTP_ALGEBRA = False
        try:
            plain, _, st_plain = _model_run(spec, 64, chains=[chain, chain], wls=wls)
        finally:
            ppasses.PTP_ALGEBRA = True
    finally:
        prun.FUSE_APERTURES = "auto"
    assert st_fast["fused_passes"] <= st_plain["fused_passes"]
    for i in fast:
        assert sorted(fast[i]) == sorted(plain[i])
        for k in fast[i]:
            a, b = fast[i][k]["wfo"], plain[i][k]["wfo"]
            assert np.isfinite(a).all() and np.isfinite(b).all()
            assert rel_err(a, b) < 1e-11, (seed, i, k, rel_err(a, b), st_fast, st_plain)


def test_a_near_inverse_wts_stw_pair_keeps_its_residual_phase():
    """The numbers behind the rewrite: wts then stw whose phases leave 5e-8 rad at the corner along x and -2e-8 along
    y, on a random field, against the two operators run one after the other (PTP_ALGEBRA off): equal to rounding,
    with two passes less; dropping the residual instead would show at 1e-8."""
    import paos_amd.passes as ppasses
    from paos_amd.passes import PassCompiler

    n, nb = 64, 2
    half = (n / 2.0) ** 2
    rng = np.random.default_rng(5)
    u0 = rng.standard_normal((nb, n, n)) + 1j * rng.standard_normal((nb, n, n))
    cw = 3.0e-3
    wts = np.array([[1.0, 1.0, 1.0, cw, 1.0]] * nb)
    stw = np.array([[1.0, np.sqrt(1.0 - 5.0e-8 / (cw * half)), np.sqrt(1.0 + 2.0e-8 / (cw * half)), cw, -1.0]] * nb)
    fwd, inv = np.zeros(nb), np.ones(nb)
    out = {}
    for algebra in (True, False):
        ppasses.PTP_ALGEBRA = algebra
        try:
            dev = ModelDevice(n, nb)
            dev.u[:] = u0
            comp = PassCompiler(nb, n)
            comp.wts(wts, fwd)
            comp.stw(stw, inv)
            out[algebra] = (comp.flush(dev), dev.u.copy())
        finally:
            ppasses.PTP_ALGEBRA = True
    assert out[True][0] < out[False][0], (out[True][0], out[False][0])
    assert rel_err(out[True][1], out[False][1]) < 1e-13
    assert rel_err(u0, out[False][1]) > 1e-9  # ... and the residual is really there


def test_power_of_a_saved_surface_rides_on_the_pass_that_stores_it():
    """Round 4: where a saved surface's field is exactly what its pass program stored (no stop, Zernike, phase map or
    stand-alone aperture on the surface), the last pass sums |u|^2 on the way (paos_run_program: final_intensity = 2)
    and no separate reduction reads the field back.  On the model device: SYN20 with every relay surface saved -- the
    powers equal those of the ordinary reductions, and the fused path was really taken."""
    import paos_amd.run as prun
    from paos_amd.run import run_batch

    wls = [1.0e-6, 1.4e-6]
    chain = syn20_chain()
    for k, it in chain.items():
        if it["name"].endswith("b") or it["name"].endswith("c"):
            chain[k] = dict(it, save=True)
    prun.FUSE_APERTURES = True
    try:
        dev = ModelDevice(128, 2)
        got = run_batch(1.0, wls, 128, 4, FIELD, [chain, chain], outputs=(), dev=dev, keep_psf=True)
        kinds = [name for name, _ in dev.log]
        assert kinds.count("power_on_store") >= 8, kinds.count("power_on_store")
        want = run_batch(1.0, wls, 128, 4, FIELD, [chain, chain], outputs=("wfo",), dev=ModelDevice(128, 2), keep_psf=True)
    finally:
        prun.FUSE_APERTURES = "auto"
    for i in range(2):
        assert sorted(got[i]) == sorted(want[i])
        for k in want[i]:
            direct = float(np.sum(np.abs(want[i][k]["wfo"]) ** 2))
            assert abs(got[i][k]["power"] - direct) <= 1e-12 * direct, (i, k, got[i][k]["power"], direct)
            assert abs(want[i][k]["power"] - direct) <= 1e-12 * direct


@pytest.mark.parametrize("name", ["Excite_TEL", "Ariel_AIRS-CH0", "Ariel_FGS-FGS1"])
def test_a_stop_behind_a_pass_program_takes_its_power_from_the_program(name):
    """Round 4: the stop of a real prescription sits on a mirror the beam has propagated to; the pass program that
    brings it there sums |u|^2 on its way out (final_intensity = 2) and make_stop only scales
    (paos_stop_scale_last_power).  Fields and powers equal those of the ordinary make_stop; the power reported behind
    the stop is P (1 / sqrt P)^2."""
    import paos_amd.run as prun
    from paos_amd.run import run_batch

    spec = _spec(name)
    out = {}
    for fused in (True, False):
        prun.STOP_FROM_PROGRAM = fused
        prun.FUSE_APERTURES = True  # as at the production sizes: the mirror's aperture rides on the pass that reaches it
        try:
            dev = ModelDevice(64, 2)
            out[fused] = (run_batch(spec["pup"], [spec["wl"], 1.1 * spec["wl"]], 64, spec["zoom"], spec["field"], [spec["chain"]] * 2,
                                    outputs=("wfo",), dev=dev), [k for k, d in dev.log if k == "make_stop" and d == "power_known"])
        finally:
            prun.STOP_FROM_PROGRAM = True
            prun.FUSE_APERTURES = "auto"
    # the fused path is taken exactly where a stop follows a program: Excite_TEL's M1 behind the obstruction and 0.74 m of
    # free space; the Ariel channels open with coordinate breaks, which no longer spend the start field (_inert), so their
    # M1 -- aperture + stop -- is written in one go by the start kernels
    assert len(out[True][1]) == (1 if name == "Excite_TEL" else 0) and len(out[False][1]) == 0
    for i in range(2):
        for k in out[False][0][i]:
            a, b = out[True][0][i][k], out[False][0][i][k]
            assert rel_err(a["wfo"], b["wfo"]) < 1e-14, (name, i, k)
            assert abs(a["power"] - b["power"]) <= 1e-13 * b["power"], (name, i, k, a["power"], b["power"])


def test_the_image_plane_right_behind_a_saved_slit_shares_its_pass():
    """Round 4: Excite_TEL ends "slit (saved, aperture) | IMAGE_PLANE (saved, zero thickness)": nothing touches the field
    behind the slit, so in a lean walk that keeps its PSFs the pass program that reaches the slit stores |u|^2 for the
    image plane as well (one psf_store, no psf_keep sweep, no separate reduction for the slit), and both surfaces
    report that pass's power.  Equal to the ordinary walk; PAOS_INERT_TAIL=0 gives the round-3 behaviour."""
    import paos_amd.run as prun
    from paos_amd.run import run_batch

    spec = _spec("Excite_TEL")
    wls = [spec["wl"], 1.2 * spec["wl"]]
    args = (spec["pup"], wls, 64, spec["zoom"], spec["field"], [spec["chain"]] * 2)
    prun.FUSE_APERTURES = True
    try:
        want = run_batch(*args, outputs=("psf",), dev=ModelDevice(64, 2), keep_psf=True)
        dev = ModelDevice(64, 2)
        got = run_batch(*args, outputs=(), dev=dev, keep_psf=True)
        prun.INERT_TAIL = False
        try:
            dev_old = ModelDevice(64, 2)
            old = run_batch(*args, outputs=(), dev=dev_old, keep_psf=True)
        finally:
            prun.INERT_TAIL = True
    finally:
        prun.FUSE_APERTURES = "auto"
    kinds, kinds_old = [k for k, _ in dev.log], [k for k, _ in dev_old.log]
    assert kinds.count("psf_store") == 1 and kinds.count("psf_keep") == 0 and kinds.count("psf_keep_power") == 0, kinds
    assert kinds_old.count("psf_store") == 0  # round 3: the slit's program stores the field, the image plane sweeps it again
    last, slit = max(want[0]), sorted(want[0])[-2]
    for i in range(2):
        assert np.allclose(dev.psf_fetch(i), want[i][last]["psf"], rtol=0, atol=1e-13 * want[i][last]["psf"].max())
        for k in (slit, last):
            assert abs(got[i][k]["power"] - want[i][k]["power"]) <= 1e-12 * want[i][k]["power"], (i, k)
            assert abs(old[i][k]["power"] - want[i][k]["power"]) <= 1e-12 * want[i][k]["power"], (i, k)
        assert got[i][slit]["power"] == got[i][last]["power"]


def test_power_tickets_of_an_unsynchronised_run_can_be_fetched_per_record():
    """with ``sync=False`` a saved slit and the image plane behind it are answered by ONE reduction (the
    pass that stored the PSF), and a surface whose stop scales by its program's power reports a DERIVED power.  Every
    record gets a ``PowerTicket``: each may be fetched (through the handle or through ``dev.norm2_fetch``), in any
    order, more than once; the library's slot is read exactly once (the model device, like the library, refuses a
    second fetch of a slot); a derived power is formed at fetch time -- run_batch itself never waits."""
    import paos_amd.run as prun
    from paos_amd.run import PowerTicket, run_batch

    spec = _spec("Excite_TEL")
    wls = [spec["wl"], 1.2 * spec["wl"]]
    chain = {k: dict(v, save=True) for k, v in spec["chain"].items()}  # every surface saved: the stop's power is derived
    args = (spec["pup"], wls, 64, spec["zoom"], spec["field"], [chain] * 2)
    prun.FUSE_APERTURES = True
    try:
        want = run_batch(*args, outputs=(), dev=ModelDevice(64, 2), keep_psf=True)
        dev = ModelDevice(64, 2)
        fetches = []
        real_fetch = dev.norm2_fetch
        dev.norm2_fetch = lambda t: (fetches.append(t) if not hasattr(t, "fetch") else None, real_fetch(t))[1]
        got = run_batch(*args, outputs=(), dev=dev, keep_psf=True, sync=False)
    finally:
        prun.FUSE_APERTURES = "auto"
    assert fetches == [], "run_batch(sync=False) fetched a power itself"
    last, slit = max(want[0]), sorted(want[0])[-2]
    assert got[0][slit]["power_ticket"]._red is got[0][last]["power_ticket"]._red  # two handles on ONE reduction
    derived = [k for k in got[0] if isinstance(got[0][k].get("power_ticket"), PowerTicket) and got[0][k]["power_ticket"]._post]
    assert derived, "no surface reported a power derived from its program's reduction"
    for order in (sorted(got[0]), sorted(got[0], reverse=True)):  # any order, twice over
        for k in order:
            for i in range(2):
                rec = got[i][k]
                assert "power" not in rec and isinstance(rec["power_ticket"], PowerTicket)
                a, b = rec["power_ticket"].fetch()[i], dev.norm2_fetch(rec["power_ticket"])[i]
                assert a == b and abs(a - want[i][k]["power"]) <= 1e-12 * want[i][k]["power"], (i, k, a, want[i][k]["power"])
    assert len(fetches) == len(set(fetches)), "a slot was read twice"
    assert not dev._ring, "a slot leaked"
    # given back unread: release is idempotent across the records that share a reduction, and a later fetch says so
    dev2 = ModelDevice(64, 2)
    prun.FUSE_APERTURES = True
    try:
        res = run_batch(*args, outputs=(), dev=dev2, keep_psf=True, sync=False)
    finally:
        prun.FUSE_APERTURES = "auto"
    for t in {rec["power_ticket"] for r in res for rec in r.values()}:
        dev2.norm2_release(t)
        t.release()
    assert not dev2._ring
    with pytest.raises(RuntimeError):
        res[0][last]["power_ticket"].fetch()


def test_many_saved_surfaces_wrap_the_ticket_ring_without_stale_powers():
    """a mid-walk drain must not serve a later surface the cached value of a slot that has been handed
    out again.  A chain with more saved surfaces than ticket slots, on the model's ring (64 slots, reissued as soon as
    they are free): every power equals the directly summed one."""
    from paos_amd.abcd import ABCD
    from paos_amd.run import run_batch

    chain = {}
    base = syn20_chain()
    first = base[min(base)]
    chain[1] = dict(first, num=1, save=True)
    for k in range(2, 2 + 2 * _lib.NORM_SLOTS + 5):  # flat, saved surfaces a short hop apart: each is one reduction
        chain[k] = {"num": k, "type": "Standard", "name": f"P{k}", "is_stop": False, "save": True,
                    "ABCDt": ABCD(thickness=1.0e-3 * (1 + k % 3), curvature=0.0), "ABCDs": ABCD(thickness=1.0e-3 * (1 + k % 3), curvature=0.0)}
    got = run_batch(1.0, [1.0e-6, 1.3e-6], 64, 4, FIELD, [chain, chain], outputs=("wfo",), dev=ModelDevice(64, 2))
    for i in range(2):
        for k, rec in got[i].items():
            direct = float(np.sum(np.abs(rec["wfo"]) ** 2))
            assert abs(rec["power"] - direct) <= 1e-12 * direct, (i, k)


def test_lean_walk_writes_the_first_field_inside_its_aperture_box_only():
    """Round 5: the lean start writes only the rows AND the columns inside the first aperture's bounding
    box (paos_start_box); the model device poisons everything else with NaN.  The power of the saved first surface is
    summed over the box, the first pass program is told the columns stand for zeros, a second saved surface in front of any
    program still reports the right power, a stop in front of any program makes the box real zeros first -- and the results
    equal those of whole-row starts (PAOS_START_BOX=0) and of the ordinary walk."""
    from fakes import ModelDevice
    import paos_amd.run as prun
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.run import run_batch

    wls = [syn20_wavelength(0), syn20_wavelength(300)]
    field = {"us": 0.0, "ut": 0.0}

    class Spy(ModelDevice):
        def start(self, value, shape, blocks, stop=None, write_rows=None, write_cols=None):
            self.log.append(("start_windows", (write_rows, write_cols)))
            super().start(value, shape, blocks, stop, write_rows=write_rows, write_cols=write_cols)
            if write_cols is not None:  # the poison is really there
                lo, hi = (int(write_cols[0][0]) // 4) * 4, -(-int(write_cols[0][1]) // 4) * 4
                assert np.isnan(self.u[0][:, :lo]).all() and np.isnan(self.u[0][:, hi:]).all() and lo > 0 and hi < self.n

        def run_passes(self, passes, blocks, live_rows=None, rows_stale=False, final_intensity=False, live_cols=None):
            self.log.append(("program_windows", (rows_stale, live_cols is not None)))
            return super().run_passes(passes, blocks, live_rows=live_rows, rows_stale=rows_stale, final_intensity=final_intensity,
                                      live_cols=live_cols)

    prun.FUSE_APERTURES = True
    try:
        chains = [syn20_chain(), syn20_chain()]
        plain = run_batch(1.0, wls, 128, 4, field, chains, outputs=("psf",), dev=ModelDevice(128, 2), keep_psf=True)
        dev = Spy(128, 2)
        box = run_batch(1.0, wls, 128, 4, field, chains, outputs=(), dev=dev, keep_psf=True)
        rows, cols = [d for k, d in dev.log if k == "start_windows"][0]
        assert rows is not None and cols is not None and all(0 < lo < hi < 128 for lo, hi in cols)
        assert [d for k, d in dev.log if k == "program_windows"][0] == (True, True)
        prun.START_BOX = False
        try:
            dev_rows = Spy(128, 2)
            whole = run_batch(1.0, wls, 128, 4, field, chains, outputs=(), dev=dev_rows, keep_psf=True)
        finally:
            prun.START_BOX = True
        assert [d for k, d in dev_rows.log if k == "start_windows"][0][1] is None
        for i in range(2):
            for k in (1, 20):
                # (on the GPU the two sums are the same bit for bit -- tests/test_gpu_r5.py; NumPy's pairwise sum over
                # another window rounds differently)
                assert abs(box[i][k]["power"] - whole[i][k]["power"]) <= 4e-16 * whole[i][k]["power"]
                assert abs(box[i][k]["power"] - plain[i][k]["power"]) <= 1e-13 * plain[i][k]["power"]
            assert np.allclose(dev.psf_fetch(i), dev_rows.psf_fetch(i), rtol=0, atol=1e-15 * dev_rows.psf_fetch(i).max())
        # a second saved surface before any program runs (S02, the Zernike surface, saved): summed over the box as well
        chain2 = syn20_chain()
        chain2[2] = dict(chain2[2], save=True)
        dev2 = Spy(128, 1)
        got = run_batch(1.0, wls[:1], 128, 4, field, [chain2], outputs=(), dev=dev2, keep_psf=True)
        want = run_batch(1.0, wls[:1], 128, 4, field, [chain2], outputs=("psf",), dev=ModelDevice(128, 1), keep_psf=True)
        for k in want[0]:
            assert np.isfinite(got[0][k]["power"]) and abs(got[0][k]["power"] - want[0][k]["power"]) <= 1e-13 * want[0][k]["power"], k
        # a stop on the second surface: the box becomes real zeros (rows and columns) before the sum reads the field
        chain3 = syn20_chain()
        chain3[2] = dict(chain3[2], is_stop=True)
        dev3 = Spy(128, 1)
        got = run_batch(1.0, wls[:1], 128, 4, field, [chain3], outputs=(), dev=dev3, keep_psf=True)
        assert [k for k, _ in dev3.log].count("zero_outside_rows") == 1
        want = run_batch(1.0, wls[:1], 128, 4, field, [chain3], outputs=("psf",), dev=ModelDevice(128, 1), keep_psf=True)
        assert abs(got[0][20]["power"] - want[0][20]["power"]) <= 1e-13 * want[0][20]["power"]
    finally:
        prun.FUSE_APERTURES = "auto"


def test_a_shared_grid_sag_map_is_built_once_and_applied_to_all_its_items():
    """Round 5: one measured-surface array on a Grid Sag surface of every item of a batch -- a
    wavelength sweep, a Monte-Carlo batch -- is turned into ITS map once (``_sag_map_once``: same array object, same
    geometry) and applied with one ``phase_map_items`` call; an array edited in place is rebuilt; items with their own
    arrays keep the per-item path.  Fields equal those of the reference formula item by item."""
    import paos_amd.run as prun
    from paos_amd.abcd import ABCD
    from paos_amd.run import run_batch

    n = 64
    rng = np.random.default_rng(5)
    sag = rng.standard_normal((n, n)) * 30.0e-9
    step = 4.0 / n

    def chain_with(screen):
        base = syn20_chain()
        out = {}
        for key, item in base.items():
            num = len(out) + 1
            out[num] = dict(item, num=num)
            if item["name"] == "Z1":
                num = len(out) + 1
                out[num] = {"num": num, "type": "Grid Sag", "name": "SCREEN", "is_stop": False, "save": True,
                            "grid_sag": screen, "nx": n, "ny": n, "delx": step, "dely": step, "xdec": 0, "ydec": 0,
                            "ABCDt": ABCD(thickness=0.0, curvature=0.0), "ABCDs": ABCD(thickness=0.0, curvature=0.0)}
        return out

    wls = [1.0e-6, 1.2e-6, 1.5e-6]
    calls = []
    real = prun.grid_sag_map
    prun.grid_sag_map = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        shared = chain_with(sag)
        dev = ModelDevice(n, 3)
        got = run_batch(1.0, wls, n, 4, FIELD, [shared] * 3, outputs=("wfo",), dev=dev)
        assert len(calls) == 1 and ("phase_map_items", 3) in dev.log and not any(k == "phase_map" for k, _ in dev.log)
        run_batch(1.0, wls, n, 4, FIELD, [shared] * 3, outputs=(), dev=ModelDevice(n, 3))
        assert len(calls) == 1  # the next batch finds the map
        sag[3, 4] += 1.0e-9   # edited in place: the fingerprint (a digest of every byte, once per walk) notices
        run_batch(1.0, wls, n, 4, FIELD, [shared] * 3, outputs=(), dev=ModelDevice(n, 3))
        assert len(calls) == 2
        sag[3, 4] -= 1.0e-9
        # every item its own array: per-item maps and uploads, same fields
        own = [chain_with(sag.copy()) for _ in wls]
        dev2 = ModelDevice(n, 3)
        want = run_batch(1.0, wls, n, 4, FIELD, own, outputs=("wfo",), dev=dev2)
        assert sum(k == "phase_map" for k, _ in dev2.log) == 3
        key = [k for k, v in shared.items() if v["name"] == "SCREEN"][0]
        for i in range(3):
            for k in want[i]:
                assert rel_err(got[i][k]["wfo"], want[i][k]["wfo"]) < 1e-13, (i, k)
        assert key in got[0]
        # ... wherever the edit is, masks included; the digest is taken once per walk and array
        big = rng.standard_normal((700, 900))
        prun._SAG_SEEN.clear()
        f0 = prun._sag_fingerprint(big)
        assert prun._sag_fingerprint(big) is f0
        big[613, 7] = np.nextafter(big[613, 7], 1.0)
        assert prun._sag_fingerprint(big) is f0  # (same walk: not looked at again)
        prun._SAG_SEEN.clear()
        assert prun._sag_fingerprint(big) != f0
        masked = np.ma.masked_array(big, mask=np.zeros(big.shape, dtype=bool))
        f1 = prun._sag_fingerprint(masked)
        masked.mask[5, 5] = True
        prun._SAG_SEEN.clear()
        assert prun._sag_fingerprint(masked) != f1
    finally:
        prun.grid_sag_map = real
        prun._SAG_SEEN.clear()


def test_psd_screens_are_built_by_the_device_from_the_hosts_draws():
    """Round 5: from ``phase_maps.PSD_ON_DEVICE_FROM`` up, a PSD surface hands the context its two
    white-noise draws and twelve numbers (``psd_screen``) instead of a finished map.  The draws are NumPy's, in the
    reference's order, so the generator ends in the same state either way; the twelve numbers reproduce the host path's
    map (<= 1e-13 of its peak, on the NumPy model of the kernels); complex64 contexts and small grids keep the host path."""
    import paos_amd.run as prun
    from paos_amd import phase_maps
    from paos_amd.abcd import ABCD
    from paos_amd.run import run_batch

    n = 64
    kw = dict(A=12.0, B=1.0, C=2.2, fknee=3.0, fmin=0.5, fmax=6.0, SR=2.0, units="nm")

    def chain():
        out = {}
        for key, item in syn20_chain().items():
            num = len(out) + 1
            out[num] = dict(item, num=num)
            if item["name"] == "Z1":
                num = len(out) + 1
                out[num] = dict(kw, num=num, type="PSD", name="SCREEN", is_stop=False, save=True,
                                ABCDt=ABCD(thickness=0.0, curvature=0.0), ABCDs=ABCD(thickness=0.0, curvature=0.0))
        return out

    key = [k for k, v in chain().items() if v["name"] == "SCREEN"][0]
    keep = phase_maps.PSD_ON_DEVICE_FROM
    try:
        phase_maps.PSD_ON_DEVICE_FROM = n
        dev = ModelDevice(n, 1)
        np.random.seed(77)
        got = run_batch(1.0, [1.0e-6], n, 4, FIELD, [chain()], outputs=("wfo",), dev=dev)[0]
        after_device = np.random.get_state()[1].copy()
        assert any(k == "psd_screen" for k, _ in dev.log) and not any(k == "phase_map" for k, _ in dev.log)
        phase_maps.PSD_ON_DEVICE_FROM = 1 << 20  # ... and the host path
        dev2 = ModelDevice(n, 1)
        np.random.seed(77)
        want = run_batch(1.0, [1.0e-6], n, 4, FIELD, [chain()], outputs=("wfo",), dev=dev2)[0]
        assert np.array_equal(after_device, np.random.get_state()[1])
        assert any(k == "phase_map" for k, _ in dev2.log) and not any(k == "psd_screen" for k, _ in dev2.log)
        # the map a single wavefront's surface returns (run(): the surface's `wfe`)
        maps = []
        for first in (n, 1 << 20):
            phase_maps.PSD_ON_DEVICE_FROM = first
            np.random.seed(78)
            d1 = ModelDevice(n, 1)
            d1.fill(1.0)
            maps.append(prun._launch_phase_maps(d1, [{"phase_map": (phase_maps.PsdScreen((n, n), 0.03, 0.04, **kw), 1.0e-6)}], None))
        a, b = np.ma.filled(maps[0], 0.0), np.ma.filled(maps[1], 0.0)
        assert np.abs(b).max() > 0 and np.abs(a - b).max() <= 1e-13 * np.abs(b).max()
        assert isinstance(maps[0], np.ma.MaskedArray) and not np.ma.getmaskarray(maps[0]).any()
        for k in want:
            assert rel_err(got[k]["wfo"], want[k]["wfo"]) < 1e-12, k
        # a batch: every item its own screen, in item order
        phase_maps.PSD_ON_DEVICE_FROM = n
        dev3 = ModelDevice(n, 2)
        np.random.seed(77)
        two = run_batch(1.0, [1.0e-6, 1.3e-6], n, 4, FIELD, [chain(), chain()], outputs=("wfo",), dev=dev3)
        assert sum(k == "psd_screen" for k, _ in dev3.log) == 2
        assert rel_err(two[0][key]["wfo"], want[key]["wfo"]) < 1e-12
        # complex64 contexts build the screen on the host, in doubles
        phase_maps.PSD_ON_DEVICE_FROM = n
        dev4 = ModelDevice(n, 1, precision="fp32")
        assert not phase_maps.psd_on_device(dev4, n)
        # the reference's check of fmax still fires when the call is planned
        bad = chain()
        bad[key] = dict(bad[key], fmax=1.0e9)
        with pytest.raises(AssertionError, match="fmax"):
            run_batch(1.0, [1.0e-6], n, 4, FIELD, [bad], dev=ModelDevice(n, 1))
    finally:
        phase_maps.PSD_ON_DEVICE_FROM = keep


def test_zernike_right_behind_the_start_reads_one_field_per_group_of_copies():
    """Round 5: the wavefronts of a sweep start as copies of one field (same constant, same aperture at the entrance pupil)
    and stay copies until something wavelength-dependent touches them; SYN20's Zernike surface sits right behind the start,
    so the walk tells the library (``zernike(same_as=...)`` -> paos_zernike_like).  The model device checks the claim on
    every pixel the kernel reads; the fields equal those of a walk with the hint switched off; a chain that propagates
    before its Zernike surface, or stops / clips on it, gives no hint."""
    import paos_amd.run as prun
    from paos_amd.run import run_batch

    n, nb = 64, 3
    wls = [1.0e-6, 1.3e-6, 1.7e-6]

    def walk(chains, **kw):
        dev = ModelDevice(n, nb)
        out = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=("wfo",), dev=dev, **kw)
        return dev, out

    chains = [syn20_chain() for _ in range(nb)]
    dev, got = walk(chains)
    assert any(k == "zernike_like" for k, _ in dev.log) and not any(k == "zernike" for k, _ in dev.log)
    keep = prun.TWIN_FIELDS
    try:
        prun.TWIN_FIELDS = False
        dev0, want = walk(chains)
    finally:
        prun.TWIN_FIELDS = keep
    assert not any(k == "zernike_like" for k, _ in dev0.log) and any(k == "zernike" for k, _ in dev0.log)
    for i in range(nb):
        for k in want[i]:
            assert np.array_equal(got[i][k]["wfo"], want[i][k]["wfo"]), (i, k)
    # a propagation between the start and the Zernike surface: the fields have diverged, no hint
    from paos_amd.abcd import ABCD

    moved = [syn20_chain() for _ in range(nb)]
    for c in moved:
        first = next(iter(c))
        c[first] = dict(c[first], ABCDt=ABCD(thickness=0.3, curvature=0.0), ABCDs=ABCD(thickness=0.3, curvature=0.0))
    dev2, _ = walk(moved)
    assert not any(k == "zernike_like" for k, _ in dev2.log) and any(k == "zernike" for k, _ in dev2.log)


def test_batch_planner_equals_the_per_item_planner():
    """``run._plan_surface`` plans the apertures of a whole batch with array arithmetic.  Against the scalar planner of one
    wavefront (tests/plan_np.py: the reference's formulas) item by item, on random batches -- ellipses and rectangles,
    apertures and obscurations, missing centres, different sampling per item: the parameter blocks, the line-record test,
    the live rows and the handles' numbers are identical (==, not close); a non-finite radius skips the aperture for that
    item only; an aperture that misses the grid raises the reference's TypeError; a batch with an off-axis item still
    agrees."""
    import paos_amd.run as prun
    import plan_np
    from paos_amd.abcd import ABCD

    rng = np.random.default_rng(11)
    n, nb = 1024, 12

    def items_of(shape, kind_type, nan_centre=False, bad_radius=None):
        out = []
        for i in range(nb):
            ap = {"shape": shape, "type": kind_type, "xc": float("nan") if nan_centre else float(rng.normal(0, 0.05)),
                  "yc": float(rng.normal(0, 0.05)), "xrad": float(rng.uniform(0.2, 0.6)), "yrad": float(rng.uniform(0.2, 0.6))}
            if bad_radius == i:
                ap["xrad"] = float("nan")
            out.append({"type": "Standard", "is_stop": bool(i % 2), "save": False, "aperture": ap,
                        "ABCDt": ABCD(thickness=0.1), "ABCDs": ABCD(thickness=0.1)})
        return out

    def both(items, fields):
        dxs = [4.0 / n * (1 + 0.01 * i) for i in range(nb)]
        dys = [4.0 / n * (1 + 0.02 * i) for i in range(nb)]
        wls = [1e-6] * nb
        fast = prun._plan_surface(items, n, dxs, dys, wls, lambda i: 0.5, prun._Rays(fields))
        slow = [plan_np.plan_aperture(plan_np.Ray(f), it, n, dxs[i], dys[i]) for i, (f, it) in enumerate(zip(fields, items))]
        return fast, slow

    on_axis = [{"us": 0.0, "ut": 0.0} for _ in range(nb)]
    for shape in ("elliptical", "rectangular"):
        for kind_type in ("aperture", "obscuration"):
            for nan_centre in (False, True):
                items = items_of(shape, kind_type, nan_centre)
                fast, slow = both(items, on_axis)
                assert fast.ap is not None and fast.ap.on.all()
                blocks, codes = fast.ap.blocks()
                for i in range(nb):
                    h, o = slow[i]
                    assert list(blocks[i]) == h.block(obscuration=o), (shape, kind_type, i)
                    assert codes[i] == (_lib.SHAPE_ELLIPSE if shape == "elliptical" else _lib.SHAPE_RECT)
                    fh, fo = fast.aperture(i), bool(fast.ap.obsc[i])
                    assert fo == o and type(fh) is type(h) and fh.block(obscuration=fo) == h.block(obscuration=o)
                    assert fast[i]["stop"] == bool(items[i]["is_stop"])
                assert fast.ap.fits_line_records(n, "fp64") == all(
                    plan_np.fits_line_records(*slow[i], n, "fp64") for i in range(nb))
                la, lb = [[0, n] for _ in range(nb)], [[0, n] for _ in range(nb)]
                prun._live_rows_after(fast, la, n)
                plan_np.live_rows_after(slow, lb, n)
                assert la == lb
                assert fast.summary() == (True, False, False, True)
    # one item without a finite radius: no aperture for that item, handles for the others, same as item by item
    fast, slow = both(items_of("elliptical", "aperture", bad_radius=5), on_axis)
    assert fast.ap.on.tolist() == [i != 5 for i in range(nb)]
    assert fast.aperture(5) is None and slow[5] is None
    assert fast.ap.blocks()[0].tolist() == [plan_np.block_of(ap) for ap in slow]
    assert all(fast.aperture(i).block() == slow[i][0].block() for i in range(nb) if i != 5)
    # an aperture whose box misses the grid: the reference fails on `u *= None`
    far = items_of("elliptical", "aperture")
    far[3]["aperture"]["xc"] = 50.0
    with pytest.raises(TypeError):
        both(far, on_axis)
    # an off-axis item: the radii are scaled by the ray slopes (run.py:97-108)
    off = [{"us": 0.01 if i == 2 else 0.0, "ut": 0.0} for i in range(nb)]
    fast, slow = both(items_of("elliptical", "aperture"), off)
    assert fast.ap.on.all()
    assert fast.ap.blocks()[0].tolist() == [plan_np.block_of(ap) for ap in slow]
    assert all(fast.aperture(i).block() == slow[i][0].block() for i in range(nb))


def _zernike_item(i, abcd, orthonorm=False):
    return {"type": "Zernike", "is_stop": False, "save": False, "ABCDt": abcd, "ABCDs": abcd, "Zindex": np.arange(0, 10 + i % 2),
            "Z": np.linspace(0.0, 1e-8, 10 + i % 2), "Zordering": "noll" if i % 2 else "standard", "Znormalize": True,
            "Zradius": float("nan") if i % 3 else 0.4, "Zorigin": "x", "Zorthonorm": orthonorm}


def test_one_planner_call_serves_items_of_different_kinds():
    """A batch whose items differ in kind at one surface -- Standard, Zernike, Coordinate Break, every one with an aperture,
    on and off axis: the break moves the rays of its items only, every aperture is the scalar planner's (==), and the
    Zernike items get their own tables, radius (the given one, else the beam's), sampling and wavelength."""
    import paos_amd.run as prun
    import plan_np
    from paos_amd.abcd import ABCD
    from paos_amd.zernike import zernike_tables

    n, nb = 1024, 9
    rng = np.random.default_rng(23)
    tie = 94906267.0 * 2.0 ** -40
    fields = [{"us": 0.0, "ut": 0.0}, {"us": 3.0e-4, "ut": -5.0e-4}, {"us": tie, "ut": -tie}] * 3
    dxs = [4.0 / n * (1 + 0.01 * i) for i in range(nb)]
    dys = [4.0 / n * (1 + 0.02 * i) for i in range(nb)]
    wls = [1e-6 * (1 + 0.1 * i) for i in range(nb)]
    abcd = ABCD(thickness=0.3, curvature=0.7)
    kinds = ["Standard", "Zernike", "Coordinate Break", "Zernike", "Coordinate Break", "Standard", "Zernike", "Standard",
             "Coordinate Break"]
    items = []
    for i, kind in enumerate(kinds):
        it = _zernike_item(i, abcd) if kind == "Zernike" else {"type": kind, "is_stop": bool(i % 2), "save": False,
                                                               "ABCDt": abcd, "ABCDs": abcd}
        if kind == "Coordinate Break":
            it.update(xdec=1e-3 * i, ydec=float("nan"), xrot=0.2 * i, yrot=-0.15)
        it["aperture"] = {"shape": "rectangular" if i % 4 == 0 else "elliptical", "type": "aperture" if i % 3 else "obscuration",
                          "xc": float("nan") if i % 2 else float(rng.normal(0, 0.01)), "yc": float(rng.normal(0, 0.01)),
                          "xrad": float(rng.uniform(0.2, 0.6)), "yrad": float(rng.uniform(0.2, 0.6))}
        items.append(it)
    rays = prun._Rays(fields)
    plans = prun._plan_surface(items, n, dxs, dys, wls, lambda i: 0.5 + i, rays)
    slow_rays = [plan_np.Ray(f) for f in fields]
    slow = [plan_np.plan_aperture(r, it, n, dxs[i], dys[i]) for i, (r, it) in enumerate(zip(slow_rays, items))]
    for i, r in enumerate(slow_rays):
        assert rays.vt[i].tolist() == r.vt.tolist() and rays.vs[i].tolist() == r.vs.tolist(), i
        assert bool(rays.still[i]) == r.still
        if kinds[i] != "Coordinate Break":  # untouched: still what the field point started them as
            assert rays.vt[i].tolist() == [0.0, fields[i]["ut"]] and rays.vs[i].tolist() == [0.0, fields[i]["us"]]
    assert plans.ap.on.all()
    assert plans.ap.blocks()[0].tolist() == [plan_np.block_of(ap) for ap in slow]
    for i in range(nb):
        assert type(plans.aperture(i)) is type(slow[i][0])
    la, lb = [[0, n] for _ in range(nb)], [[0, n] for _ in range(nb)]
    prun._live_rows_after(plans, la, n)
    plan_np.live_rows_after(slow, lb, n)
    assert la == lb
    assert plans.summary() == (True, True, False, True)
    for i, (it, p) in enumerate(zip(items, plans)):
        assert p["stop"] == bool(it["is_stop"]) and p["phase_map"] is None
        if kinds[i] != "Zernike":
            assert p["zernike"] is None
            continue
        z = p["zernike"]
        m, nn, norm = zernike_tables(len(it["Zindex"]), it["Zordering"], True)
        assert np.array_equal(z["m"], m) and np.array_equal(z["n"], nn) and np.array_equal(z["norm"], norm)
        assert z["radius"] == (0.4 if i % 3 == 0 else 0.5 + i)
        assert (z["dx"], z["dy"], z["wl"], z["origin"], z["pupil"]) == (dxs[i], dys[i], wls[i], "x", None)
        assert np.array_equal(z["Z"], it["Z"])


def test_a_partly_on_batch_of_mixed_shapes_follows_the_scalar_rules():
    """Some items with an aperture and some without (no entry, or a radius that is not finite), ellipses and rectangles,
    clear and obscuring, on and off axis: the one record's blocks are the per-item blocks with zero rows for the items
    without, and ``fits_line_records`` / ``narrow_rows`` / ``live_cols`` / ``start_shape`` give the scalar rules' answers
    -- on the whole batch and on the sub-batches where those answers differ (all on, all clear, one shape)."""
    import paos_amd.run as prun
    import plan_np
    from paos_amd.abcd import ABCD

    n, nb = 1024, 12
    rng = np.random.default_rng(31)
    abcd = ABCD(thickness=0.1)
    fields = [{"us": 0.0, "ut": 0.0}, {"us": 2.0e-3, "ut": -1.0e-3}] * 6
    dxs = [4.0 / n * (1 + 0.01 * i) for i in range(nb)]
    dys = [4.0 / n * (1 + 0.02 * i) for i in range(nb)]

    def item(i, shape, kind_type="aperture", rad=None, **geo):
        ap = {"shape": shape, "type": kind_type, "xc": float(rng.normal(0, 0.01)), "yc": float("nan") if i % 2 else 0.01,
              "xrad": float(rng.uniform(0.02, 0.3)) if rad is None else rad, "yrad": float(rng.uniform(0.02, 0.3))}
        ap.update(geo)
        return {"type": "Standard", "is_stop": False, "save": False, "aperture": ap, "ABCDt": abcd, "ABCDs": abcd}

    none = {"type": "Standard", "is_stop": False, "save": False, "ABCDt": abcd, "ABCDs": abcd}
    whole = [item(0, "elliptical"), dict(none), item(2, "rectangular"), item(3, "elliptical", rad=float("nan")),
             item(4, "elliptical", "obscuration"), item(5, "rectangular"), dict(none, aperture=None), item(7, "elliptical", rad=0.9),
             item(8, "rectangular", "obscuration"), item(9, "elliptical"), item(10, "rectangular", yrad=float("inf")),
             item(11, "elliptical")]
    on = [i not in (1, 3, 6, 10) for i in range(nb)]
    picks = {"whole": list(range(nb)), "all on": [0, 2, 4, 5, 7, 8, 9, 11], "clear": [0, 2, 5, 9, 11], "ellipses": [0, 9, 11],
             "rectangles": [2, 5], "small clear ellipses and rectangles": [0, 2, 5, 9, 11, 1]}
    answers = set()
    for name, pick in picks.items():
        items, fl = [whole[i] for i in pick], [fields[i] for i in pick]
        dx, dy = [dxs[i] for i in pick], [dys[i] for i in pick]
        plans = prun._plan_surface(items, n, dx, dy, [1e-6] * len(pick), lambda i: 0.5, prun._Rays(fl))
        slow = [plan_np.plan_aperture(plan_np.Ray(f), it, n, dx[k], dy[k]) for k, (f, it) in enumerate(zip(fl, items))]
        assert plans.ap.on.tolist() == [on[i] for i in pick] == [ap is not None for ap in slow], name
        blocks, codes = plans.ap.blocks()
        assert blocks.tolist() == [plan_np.block_of(ap) for ap in slow], name
        for k, ap in enumerate(slow):
            if ap is None:
                assert plans.aperture(k) is None and not blocks[k].any()
            else:
                assert type(plans.aperture(k)) is type(ap[0]) and plans.aperture(k).block(obscuration=ap[1]) == blocks[k].tolist()
                assert codes[k] == plan_np.start_shape([ap])
        fits = plans.ap.fits_line_records(n, "fp64")
        assert fits == plan_np.all_fit_line_records(slow, n, "fp64"), name
        assert not plans.ap.fits_line_records(512, "fp64") and not plans.ap.fits_line_records(n, "fp32")
        la, lb = [[0, n] for _ in pick], [[0, n] for _ in pick]
        plans.ap.narrow_rows(la, n)
        plan_np.live_rows_after(slow, lb, n)
        assert la == lb, name
        cols = plans.ap.live_cols(n)
        assert cols == plan_np.live_cols_of(slow, n) == prun._live_cols_of(plans, n), name
        shape = plans.ap.start_shape()
        assert shape == plan_np.start_shape(slow), name
        assert plans.summary() == (False, False, False, True)
        answers.add((name, fits, cols is not None, shape))
    # (the cases do tell the rules apart: each answer is taken both ways)
    assert {a[1] for a in answers} == {True, False} and {a[2] for a in answers} == {True, False}
    assert {a[3] for a in answers} == {None, _lib.SHAPE_ELLIPSE, _lib.SHAPE_RECT}
    assert any(r != [0, n] for r in la)
    # nobody carries an aperture: no record at all
    plans = prun._plan_surface([whole[1], whole[3], whole[6]], n, dxs[:3], dys[:3], [1e-6] * 3, lambda i: 0.5,
                               prun._Rays(fields[:3]))
    assert plans.ap is None and plans.summary() == (False, False, False, False) and plans.aperture(1) is None


def test_gate_arrays_are_remembered_per_column_and_forgotten_when_a_matrix_is_edited():
    """``run._gate_arrays``: the (Mt, Ms, fl, T, n1n2) arrays of a surface are computed once per column of ABCD objects (matched by
    identity) and recomputed when any matrix is edited in place (abcd.EPOCH) or another object sits in the column."""
    import paos_amd.run as prun
    from paos_amd.abcd import ABCD

    col_t = [ABCD(thickness=0.1 * (i + 1), curvature=0.5) for i in range(5)]
    col_s = [ABCD(thickness=0.1 * (i + 1), curvature=0.25) for i in range(5)]
    a = prun._gate_arrays(col_t, col_s)
    want = prun._surface_gates([{"ABCDt": t, "ABCDs": s} for t, s in zip(col_t, col_s)])
    for got, ref in zip(a, want):
        assert list(got) == list(ref)
    assert prun._gate_arrays(list(col_t), list(col_s)) is a          # same objects, another list: found
    other = list(col_t)
    other[2] = ABCD(thickness=9.0)
    b = prun._gate_arrays(other, col_s)
    assert b is not a and b[3][2] == 9.0                              # another object in the column: recomputed
    m = col_t[1].ABCD.copy()
    m[0, 1] = 7.0
    col_t[1].ABCD = m                                                 # edited in place: the epoch moves
    c = prun._gate_arrays(col_t, col_s)
    assert c is not a and c[3][1] == col_t[1].gates()[2]
