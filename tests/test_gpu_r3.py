"""GPU tests added in round 3.

* The oracle at the sizes BASELINE.json quotes where round 2 stopped short: Excite_TEL fp64 AND fp32 at
  4096^2 (the first oracle check of frugal_pass_kernel<float, 4096, ...>), Ariel_FGS-FGS1 Monte-Carlo draws at
  2048^2 with the on-device metrics, a 32-item heterogeneous batch (the benchmark's gridDim.y) with items
  0 / 15 / 31 against the oracle, the dead-line pruning at 4096^2 with several wavelengths, and SYN20-4096 for
  the last item of the benchmark's sweep.
* The lean walk of run_batch (outputs=()): rows left unwritten at the start, the power of the first surface
  over the live rows, the last pass storing |u|^2 (csrc/frugal_pass.h: STORE) -- against the ordinary walk.
* paos_start_rows / paos_norm2_enqueue_rows / paos_zero_outside_rows / paos_run_program through the C ABI.
* Two ranks asking for RCCL on the ONE GPU of this box: whatever RCCL makes of that, both ranks come out of
  the bring-up on the same transport within the watchdog's time and the collectives work.

Oracle cost on the GPU box's host: ~2.5 s per wavefront at 1024^2, ~11 s at 2048^2, ~50 s at 4096^2.
Aperture-mask VALUES are parity-unpinned (photutils is absent): every end-to-end figure here is
"the reference's arithmetic given the builder's masks".
"""
import os

import numpy as np
import pytest

from conftest import l2_rel_err, rel_err

pytestmark = pytest.mark.gpu

FIELD_TOL = 1e-11
PSF_TOL = 1e-10
FP32_PSF_TOL = 2e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = os.path.join(ROOT, "data", "lens")
WFE = os.path.join(ROOT, "data", "wfe", "wfe_realization_SN20210914.csv")
ON_AXIS = {"us": 0.0, "ut": 0.0}


def _oracle(*args):
    from oracle.run_np import run as oracle_run

    return oracle_run(*args, light=True)


def _check(got, ref, where, psf_tol=PSF_TOL, field_tol=FIELD_TOL):
    assert sorted(got) == sorted(ref), where
    worst = 0.0
    for k in ref:
        if "wfo" in got[k]:
            e = rel_err(got[k]["wfo"], ref[k]["wfo"])
            assert e < field_tol, (where, k, "field", e)
            e2 = l2_rel_err(got[k]["wfo"], ref[k]["wfo"])  # SURVEY 8d's second gate: L2-relative, same bound
            assert e2 < field_tol, (where, k, "field, L2-relative", e2)
        e = rel_err(got[k]["psf"], ref[k]["amplitude"] ** 2)
        worst = max(worst, e)
        assert e < psf_tol, (where, k, "psf", e)
        e2 = l2_rel_err(got[k]["psf"], ref[k]["amplitude"] ** 2)
        assert e2 < psf_tol, (where, k, "psf, L2-relative", e2)
        for key in ("dx", "dy", "wl", "fratio", "wz", "distancetofocus", "propagator"):
            assert got[k][key] == ref[k][key], (where, k, key)
    return worst


def test_excite_fp64_and_fp32_at_4096_vs_oracle():
    """BASELINE configs[4] at its quoted size: two wavelengths of the Excite_TEL sweep, complex128 and complex64
    fields, every saved surface against the oracle.  fp32 bound 2e-5 of the PSF peak (SURVEY 8d predicted 3e-6)."""
    from paos_amd.chains import parse_config_variant
    from paos_amd.run import run_batch

    n = 4096
    pup, par, wls, fields, chains = parse_config_variant(os.path.join(LENS, "Excite_TEL.ini"), [1.0, 3.4])
    w = [1.0e-6 * x for x in wls]
    r64 = run_batch(pup, w, n, par["zoom"], fields[0], chains, outputs=("psf",))
    r32 = run_batch(pup, w, n, par["zoom"], fields[0], chains, outputs=("psf",), precision="fp32")
    report = []
    for i in range(len(w)):
        ref = _oracle(pup, w[i], n, par["zoom"], fields[0], chains[i])
        e64 = _check(r64[i], ref, ("Excite fp64 4096", i))
        e32 = _check(r32[i], ref, ("Excite fp32 4096", i), psf_tol=FP32_PSF_TOL)
        assert e32 > 1e-9, "fp32 mode is expected to differ measurably from fp64"
        last = max(ref)
        assert rel_err(r32[i][last]["psf"], r64[i][last]["psf"]) < FP32_PSF_TOL
        report.append((w[i], e64, e32))
        del ref
    print("Excite_TEL 4096^2 PSF error vs oracle (wavelength, fp64, fp32):", report)


def test_fgs1_monte_carlo_at_2048_vs_oracle():
    """BASELINE configs[3] at its quoted size: Ariel_FGS-FGS1 with the WFE surface un-ignored, two draws of the
    realisation table as ONE batch at 2048^2, against the oracle, with the on-device PSF metrics."""
    from paos_amd.chains import inject_wfe, parse_config_variant, read_wfe_table
    from paos_amd.run import run_batch

    n = 2048
    pup, par, wls, fields, chains = parse_config_variant(os.path.join(LENS, "Ariel_FGS-FGS1.ini"), unignore=("Z1",))
    _, _, _, table = read_wfe_table(WFE)
    wl = 1.0e-6 * wls[0]
    mc = [inject_wfe(chains[0], table[:, c]) for c in (5, 17)]
    radii = np.geomspace(2.0, 256.0, 8)
    got = run_batch(pup, [wl] * 2, n, par["zoom"], fields[0], mc, outputs=("psf",), metrics_radii_px=radii)
    yy, xx = np.mgrid[0:n, 0:n]
    d2 = (xx - n / 2) ** 2 + (yy - n / 2) ** 2
    for c in range(2):
        ref = _oracle(pup, wl, n, par["zoom"], fields[0], mc[c])
        _check(got[c], ref, ("FGS1 2048 draw", c))
        last = max(ref)
        psf = ref[last]["amplitude"] ** 2
        m = got[c][last]["metrics"]
        assert abs(m["power"] - psf.sum()) < 1e-11 * psf.sum()
        for r, ee in zip(radii, m["encircled"]):
            assert abs(ee - psf[d2 <= r * r].sum()) < 1e-10 * psf.sum(), (c, r)
    last = max(got[0])
    assert rel_err(got[0][last]["psf"], got[1][last]["psf"]) > 1e-6  # two different draws


def test_batch_of_32_wavelengths_vs_oracle():
    """The benchmark launches with gridDim.y = 32; so does this: 32 Ariel_AIRS-CH0 wavelengths across the channel
    (each its own chain: glass indices, prism magnification) at 1024^2 in ONE run_batch, items 0, 15 and 31 against
    the oracle, and all 32 distinct."""
    from paos_amd.chains import parse_config_variant
    from paos_amd.run import run_batch

    n = 1024
    sweep = np.linspace(1.95, 3.9, 32)
    pup, par, wls, fields, chains = parse_config_variant(os.path.join(LENS, "Ariel_AIRS-CH0.ini"), sweep)
    w = [1.0e-6 * x for x in wls]
    got = run_batch(pup, w, n, par["zoom"], fields[0], chains, outputs=("psf",))
    assert len(got) == 32
    for i in (0, 15, 31):
        ref = _oracle(pup, w[i], n, par["zoom"], fields[0], chains[i])
        _check(got[i], ref, ("AIRS x32", i))
        last = max(ref)
        assert abs(got[i][last]["power"] - float(np.sum(ref[last]["amplitude"] ** 2))) < 1e-11
    last = max(got[0])
    peaks = {float(g[last]["psf"].max()) for g in got}
    assert len(peaks) == 32


def test_dead_line_pruning_changes_nothing_at_4096():
    """The 4096^2 shapes of the pruning (512-thread workgroups, 2-row tiles): four wavelengths of the SYN20 sweep,
    pruning on and off, bit-equal saved fields and powers."""
    import paos_amd.run as prun
    from paos_amd import _lib
    from paos_amd.chains import syn20_chain, syn20_wavelength

    n = 4096
    wls = [syn20_wavelength(k) for k in (0, 150, 333, 511)]
    chains = [syn20_chain() for _ in wls]
    out = []
    for on in (True, False):
        dev = _lib.DeviceFields(n, len(chains))
        dev.set_pruning(on)
        res = prun.run_batch(1.0, wls, n, 4, ON_AXIS, chains, outputs=("wfo",), dev=dev)
        out.append([(r[20]["wfo"], r[20]["power"], r[1]["power"]) for r in res])
        dev.close()
    for (a, pa, qa), (b, pb, qb) in zip(*out):
        assert np.array_equal(a, b)
        assert pa == pb and qa == qb


def test_syn20_4096_last_item_of_the_sweep_vs_oracle():
    """SYN20 at 4096^2 for k = 31, the last wavelength of the benchmark's 32-wavefront step (round 2 checked
    k = 0), run as item 1 of a two-item batch next to k = 0."""
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.run import run_batch

    n = 4096
    wls = [syn20_wavelength(0), syn20_wavelength(31)]
    got = run_batch(1.0, wls, n, 4, ON_AXIS, [syn20_chain(), syn20_chain()], outputs=("psf",))
    ref = _oracle(1.0, wls[1], n, 4, ON_AXIS, syn20_chain())
    e = _check(got[1], ref, ("SYN20 4096 k=31",))
    print("SYN20 4096^2 k=31 PSF error vs oracle:", e)


def test_syn20_without_the_ptp_identities_vs_oracle_and_vs_the_fused_chain():
    """The pass compiler's two ptp identities (consecutive ptp share a middle pass; a ptp and its exact inverse
    cancel: 24 passes per SYN20 wavefront instead of 44) switched off -- the configuration bench.py reports as
    ``without_ptp_algebra`` -- against the oracle, and the default chain against it: the identities move the PSF by
    rounding only."""
    import paos_amd.passes as ppasses
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.run import run_batch

    n = 2048
    wls = [syn20_wavelength(0), syn20_wavelength(17)]
    chains = [syn20_chain(), syn20_chain()]
    fused_stats, plain_stats = {}, {}
    fused = run_batch(1.0, wls, n, 4, ON_AXIS, chains, outputs=("psf",), stats=fused_stats)
    assert ppasses.PTP_ALGEBRA is True
    ppasses.PTP_ALGEBRA = False
    try:
        plain = run_batch(1.0, wls, n, 4, ON_AXIS, chains, outputs=("psf",), stats=plain_stats)
    finally:
        ppasses.PTP_ALGEBRA = True
    assert plain_stats["fused_passes"] > fused_stats["fused_passes"] + 15
    ref = _oracle(1.0, wls[1], n, 4, ON_AXIS, syn20_chain())
    e_plain = _check(plain[1], ref, ("SYN20 2048 k=17, no ptp identities",))
    e_fused = _check(fused[1], ref, ("SYN20 2048 k=17",))
    for a, b in zip(fused, plain):
        for k in a:
            assert rel_err(a[k]["psf"], b[k]["psf"]) < 1e-12, k
            assert abs(a[k]["power"] / b[k]["power"] - 1.0) < 1e-12
    print("SYN20 2048^2 k=17 PSF error vs oracle: %.2e without the identities, %.2e with" % (e_plain, e_fused))


@pytest.mark.parametrize("n,precision", [(256, "fp64"), (512, "fp32"), (1024, "fp64"), (4096, "fp64"), (2048, "fp32")])
def test_lean_walk_equals_the_ordinary_walk(n, precision):
    """run_batch(outputs=(), keep_psf=True) -- the benchmark's mode -- leaves the dark rows of the first surface
    unwritten, sums the first power over the live rows and has the last pass store |u|^2: PSFs bit-equal to the
    ones the ordinary walk downloads, powers equal to rounding (another order of summation).  At 256^2 / 512^2 the
    generic kernels run: the rows that stand for zeros are cleared before the first program and the PSF comes from
    the intensity sweep -- the same answers through the fall-back paths."""
    from paos_amd import _lib
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.run import run_batch

    wls = [syn20_wavelength(k) for k in (0, 31, 300)]
    chains = [syn20_chain() for _ in wls]
    plain = run_batch(1.0, wls, n, 4, ON_AXIS, chains, outputs=("psf",), precision=precision)
    dev = _lib.DeviceFields(n, len(wls), precision)
    try:
        # poison the buffer: rows the lean start does not write must never be read as values
        for i in range(len(wls)):
            dev.upload(i, np.full((n, n), complex(np.nan, np.nan)))
        stats = {}
        lean = run_batch(1.0, wls, n, 4, ON_AXIS, chains, outputs=(), dev=dev, keep_psf=True, precision=precision,
                         stats=stats)
        for i in range(len(wls)):
            psf = dev.psf_fetch(i)
            assert np.array_equal(psf, plain[i][20]["psf"]), i
            for k in (1, 20):
                assert abs(lean[i][k]["power"] - plain[i][k]["power"]) <= 1e-13 * plain[i][k]["power"], (i, k)
                for key in ("dx", "dy", "fratio", "wz", "propagator"):
                    assert lean[i][k][key] == plain[i][k][key]
        # and again on the same context: the second run starts from the first run's leftovers
        lean2 = run_batch(1.0, wls, n, 4, ON_AXIS, chains, outputs=(), dev=dev, keep_psf=True, precision=precision)
        for i in range(len(wls)):
            assert np.array_equal(dev.psf_fetch(i), plain[i][20]["psf"])
            assert lean2[i][20]["power"] == lean[i][20]["power"] and lean2[i][1]["power"] == lean[i][1]["power"]
    finally:
        dev.close()


def test_psf_zeros_are_reused_only_while_they_are_there():
    """The pass that stores the PSF does not write the zeros of its dead tiles again when the buffer is known to hold
    them (the previous storing pass had the same live lines: passes.hip, psf_zero_*).  A sequence that keeps and
    breaks that knowledge -- the same chain twice, a chain with a wider field stop (other live columns), back, an
    intensity sweep over junk in between -- must give the ordinary walk's PSFs bit for bit every time."""
    from paos_amd import _lib
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.run import run_batch

    n = 1024
    wls = [syn20_wavelength(k) for k in (0, 200)]

    def chains(stop_mm):
        out = []
        for _ in wls:
            c = syn20_chain()
            c[19]["aperture"]["xrad"] = c[19]["aperture"]["yrad"] = stop_mm * 1.0e-3
            out.append(c)
        return out

    plain = {mm: run_batch(1.0, wls, n, 4, ON_AXIS, chains(mm), outputs=("psf",)) for mm in (1.0, 2.5)}
    assert not np.array_equal(plain[1.0][0][20]["psf"], plain[2.5][0][20]["psf"])
    assert (plain[2.5][0][20]["psf"] > 0).sum() > 2 * (plain[1.0][0][20]["psf"] > 0).sum()  # more live columns
    dev = _lib.DeviceFields(n, len(wls))
    rng = np.random.default_rng(3)
    try:
        for step, mm in enumerate((1.0, 1.0, 2.5, 2.5, 1.0, "junk", 1.0, "junk", 2.5, 1.0)):
            if mm == "junk":  # the whole PSF buffer rewritten by the intensity sweep of an unrelated field
                for i in range(len(wls)):
                    dev.upload(i, rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
                dev.psf_keep()
                assert dev.psf_fetch(0).min() > 0.0
                continue
            run_batch(1.0, wls, n, 4, ON_AXIS, chains(mm), outputs=(), dev=dev, keep_psf=True)
            for i in range(len(wls)):
                assert np.array_equal(dev.psf_fetch(i), plain[mm][i][20]["psf"]), (step, mm, i)
    finally:
        dev.close()


def test_row_window_entry_points():
    """paos_start_rows + paos_norm2_enqueue_rows + paos_zero_outside_rows + paos_run_program(rows_stale) against
    paos_start + paos_norm2_enqueue + paos_run_passes_live on the same inputs; argument checks."""
    from paos_amd import _lib
    from paos_amd.aperture import make_aperture
    from paos_amd.passes import PassCompiler
    from paos_amd.planner import PilotBeam

    n, nb = 1024, 2
    dev = _lib.DeviceFields(n, nb)
    ref = _lib.DeviceFields(n, nb)
    try:
        beam = PilotBeam(1.0, 1.0e-6, n, 4)
        handles = [make_aperture(n, beam.dx, beam.dy, 0.0, 0.0, hx=0.5, hy=0.5, shape="elliptical"),
                   make_aperture(n, beam.dx, beam.dy, 0.01, -0.02, hx=0.4, hy=0.3, shape="elliptical")]
        blocks = [h.block(obscuration=False) for h in handles]
        rows = []
        for h in handles:
            yc, ext = float(h.positions[1]), h.b
            rows.append([max(0, int(np.floor(yc - ext + 0.5)) - 1), min(n, int(np.ceil(yc + ext + 0.5)) + 1)])
        for d in (dev, ref):
            for i in range(nb):
                d.upload(i, np.full((n, n), 7.0 - 3.0j))  # leftovers
        ref.start(1.0 + 0j, _lib.SHAPE_ELLIPSE, blocks, [1.0, 1.0])
        dev.start(1.0 + 0j, _lib.SHAPE_ELLIPSE, blocks, [1.0, 1.0], write_rows=rows)
        for i in range(nb):
            a, b = dev.download(i), ref.download(i)
            lo, hi = (rows[i][0] // 4) * 4, -(-rows[i][1] // 4) * 4
            assert np.array_equal(a[lo:hi], b[lo:hi])
            assert np.all(a[:lo] == 7.0 - 3.0j) and np.all(a[hi:] == 7.0 - 3.0j)  # untouched
            assert not b[:lo].any() and not b[hi:].any()
        # the power over the live rows is the power of the zero-filled field, to the last bit
        assert np.array_equal(dev.norm2_fetch(dev.norm2_enqueue(rows)), ref.norm2_fetch(ref.norm2_enqueue()))
        assert np.array_equal(ref.norm2_fetch(ref.norm2_enqueue(rows)), ref.norm2_fetch(ref.norm2_enqueue()))
        # copies are summed once (paos_norm2_enqueue_rows_like): a context whose items start from the same field
        twin = _lib.DeviceFields(n, 3)
        try:
            twin.start(1.0 + 0j, _lib.SHAPE_ELLIPSE, [blocks[0], blocks[1], blocks[0]], [1.0, 1.0, 1.0], write_rows=[rows[0], rows[1], rows[0]])
            wr = [rows[0], rows[1], rows[0]]
            plain = twin.norm2_fetch(twin.norm2_enqueue(wr))
            assert np.array_equal(twin.norm2_fetch(twin.norm2_enqueue(wr, same_as=[0, 1, 0])), plain) and plain[0] == plain[2]
            assert np.array_equal(twin.norm2_fetch(twin.norm2_enqueue(wr, same_as=[2, 1, 2])), plain)  # any member may lead
            for bad in ([0, 1, 1], [1, 1, 0], [0, 1, 3], [0, 1, -1], [0, 1, 0.5]):  # other window / not its own leader / range
                with pytest.raises(_lib.PaosHipError):
                    twin.norm2_enqueue(wr, same_as=bad)
        finally:
            twin.close()
        # a program that consumes the stale rows == the same program on real zeros
        comp = PassCompiler(nb, n)
        comp.ptp([beam.ptp(3.0)] * nb)
        passes, pblocks = comp.program()
        dev.run_passes(passes, pblocks, live_rows=rows, rows_stale=True)
        ref.run_passes(passes, pblocks, live_rows=rows)
        for i in range(nb):
            assert np.array_equal(dev.download(i), ref.download(i))
        # zero_outside_rows
        dev.start(1.0 + 0j, _lib.SHAPE_ELLIPSE, blocks, [1.0, 0.0], write_rows=rows)
        dev.zero_outside_rows(rows)
        ref.start(1.0 + 0j, _lib.SHAPE_ELLIPSE, blocks, [1.0, 0.0])
        for i in range(nb):
            assert np.array_equal(dev.download(i), ref.download(i))
        # the PSF instead of the field: same PSF, same power to rounding
        ticket = dev.run_passes(passes, pblocks, final_intensity=True)
        ref.run_passes(passes, pblocks)
        want = ref.norm2_fetch(ref.psf_keep_power())
        got = dev.norm2_fetch(ticket)
        assert np.allclose(got, want, rtol=1e-13, atol=0)
        for i in range(nb):
            assert np.array_equal(dev.psf_fetch(i), ref.psf_fetch(i))
        with pytest.raises(_lib.PaosHipError, match="row range"):
            dev.norm2_enqueue([[0, n + 4], [0, n]])
        with pytest.raises(_lib.PaosHipError, match="row range"):
            dev.start(1.0 + 0j, _lib.SHAPE_ELLIPSE, blocks, [1.0, 1.0], write_rows=[[600, 400], [0, n]])
        with pytest.raises(ValueError):
            dev.zero_outside_rows([[0, n]])
    finally:
        dev.close()
        ref.close()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_items_sharing_a_start_field_or_a_wfe_map_equal_their_solo_runs(precision):
    """Items of a batch with the same aperture record / the same Zernike record up to the wavelength are written by
    the first of them (start_write_kernel, zernike_kernel: one evaluation of the weights / polynomials per pixel for
    the whole group).  A batch that mixes two groups, a loner and a switched-off item, against one-item contexts:
    bit for bit."""
    from paos_amd import _lib
    from paos_amd.aperture import make_aperture
    from paos_amd.planner import jacobi_recurrence, zernike_block
    from paos_amd.zernike import Zernike

    n, nb = 512, 6
    dx = 4.0 / n
    # apertures: items 0, 2, 5 equal; 1, 3 equal (another radius); 4 alone (and not a stop)
    radius = [0.5, 0.42, 0.5, 0.42, 0.37, 0.5]
    stops = [1.0, 1.0, 1.0, 1.0, 0.0, 1.0]
    handles = [make_aperture(n, dx, dx, 0.0, 0.0, hx=r, hy=r, shape="elliptical") for r in radius]
    blocks = [h.block(obscuration=False) for h in handles]
    rows = [[96, 416], [112, 400], [96, 416], [112, 400], [0, n], [96, 416]]
    # Zernike records: items 0, 2, 5 one draw at three wavelengths; 1, 3 another draw; item 4 switched off
    rng = np.random.default_rng(11)
    draws = [rng.normal(0.0, 30e-9, 15), rng.normal(0.0, 30e-9, 15)]
    which = [0, 1, 0, 1, None, 0]
    wls = [1.0e-6, 1.3e-6, 1.7e-6, 2.1e-6, 1.0e-6, 0.8e-6]
    m, nn = Zernike.j2mn(15, "standard")
    norm = np.sqrt(nn + 1.0) * np.where(m == 0, 1.0, np.sqrt(2.0))
    nmax = int(nn.max())
    zb = []
    for i in range(nb):
        if which[i] is None:
            blk = np.zeros(_lib.ZERNIKE_HEAD + 2 * (nmax + 1) * (nmax // 2 + 1))
        else:
            blk, _, kdim = zernike_block(m, nn, norm, draws[which[i]], dx, dx, 0.5, wls[i], nmax=nmax)
        zb.append(blk)
    table = jacobi_recurrence(nmax)
    value = 1.0 + 0.0j

    def run(dev, items, windowed):
        sel = lambda seq: [seq[i] for i in items]  # noqa: E731
        if windowed:
            dev.start(value, _lib.SHAPE_ELLIPSE, sel(blocks), sel(stops), write_rows=sel(rows))
            dev.zero_outside_rows(sel(rows))
        else:
            dev.start(value, _lib.SHAPE_ELLIPSE, sel(blocks), sel(stops))
        dev.zernike(nmax, nmax // 2 + 1, table, np.array(sel(zb)))
        return [dev.download(k) for k in range(len(items))]

    many = _lib.DeviceFields(n, nb, precision)
    one = _lib.DeviceFields(n, 1, precision)
    try:
        for windowed in (False, True):
            got = run(many, list(range(nb)), windowed)
            for i in range(nb):
                (solo,) = run(one, [i], windowed)
                assert np.array_equal(got[i], solo), (windowed, i)
            assert not np.array_equal(got[0], got[2]) and not np.array_equal(got[1], got[3])  # the wavelengths differ
            assert np.abs(got[4]).max() == 1.0  # not a stop, no Zernike: the bare aperture
    finally:
        many.close()
        one.close()


@pytest.mark.parametrize("name,n", [("Ariel_FGS-FGS1", 2048), ("Ariel_FGS-FGS2", 1024), ("Excite_TEL", 1024)])
def test_light_output_chains_with_cancelled_hops_vs_oracle(name, n):
    """Only the image plane saved (pipeline.py:111-114): the stretches between saved surfaces are long enough for the
    pass compiler to find a wts and the stw that undoes it (flat windows: two outside-to-outside hops become one;
    FGS1 35 -> 17 passes with all identities).  Two wavelengths / WFE draws per batch, both against the oracle."""
    from paos_amd.chains import inject_wfe, parse_config_variant, read_wfe_table
    from paos_amd.run import run_batch

    pup, par, wls, fields, chains = parse_config_variant(os.path.join(LENS, name + ".ini"), unignore=("Z1",))
    table = read_wfe_table(WFE)[3]
    batch = []
    for k in (0, 1):
        chain = chains[min(k, len(chains) - 1)]
        if any(it["name"] == "Z1" for it in chain.values()):
            chain = inject_wfe(chain, table[:, 3 + k])
        chain = {key: dict(item, save=item["name"] == "IMAGE_PLANE") for key, item in chain.items()}
        batch.append((1.0e-6 * wls[min(k, len(wls) - 1)], chain))
    stats = {}
    got = run_batch(pup, [b[0] for b in batch], n, par["zoom"], fields[0], [b[1] for b in batch], outputs=("psf", "wfo"),
                    stats=stats)
    for i, (wl, chain) in enumerate(batch):
        ref = _oracle(pup, wl, n, par["zoom"], fields[0], chain)
        e = _check(got[i], ref, (name, n, i))
        print(f"{name} {n}^2 item {i}: {stats['fused_passes']} passes, PSF error vs oracle {e:.2e}")


def test_two_ranks_asking_for_rccl_on_one_gpu_agree():
    """ncclCommInitRank with nranks = 2 actually runs (under the watchdog): RCCL may refuse two ranks on one
    device -- then both ranks must agree on the TCP transport -- or accept them, or never come back -- then the
    watchdog ends both with an error; in no case does a rank hang or the two disagree.  The ranks are forked from
    the fork server conftest.py started before this process touched the GPU (no exec from a process that holds
    a GPU context)."""
    import multiprocessing as mp
    import uuid

    import rccl_pair_worker

    ctx = mp.get_context("forkserver")
    out = ctx.Queue()
    key = "pytest_" + uuid.uuid4().hex
    procs = [ctx.Process(target=rccl_pair_worker.run, args=(r, key, out)) for r in range(2)]
    for p in procs:
        p.start()
    results = sorted(out.get(timeout=150) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    kinds = [r[1] for r in results]
    print("two ranks on one GPU:", kinds, [r[2] for r in results if r[1] == "error"])
    assert kinds[0] == kinds[1] and kinds[0] in ("rccl", "socket", "error")
    if kinds[0] == "error":
        assert all("ncclCommInitRank did not return" in r[2] for r in results)
        return
    for rank, transport, text, slowest, parts in results:
        assert text == b"two ranks, one GPU" and slowest == 1.0
        assert parts == [[0.0, 1.0], [0.0, 1.0, 2.0]]


def test_record_sets_are_reused_and_evicted_correctly():
    """The context keeps a few rendered sets of aperture line records (csrc/host.h: MaskSet): a chain whose
    relays repeat one aperture renders it once, a second batch through the same optics renders nothing, and a
    chain with more distinct apertures than there are sets evicts.  Whatever the cache does, the fields equal those
    of a fresh context bit for bit, and those of the stand-alone aperture kernel to rounding."""
    import paos_amd.run as prun
    from paos_amd import _lib
    from paos_amd.chains import syn20_chain, syn20_wavelength

    n = 1024
    wls = [syn20_wavelength(0), syn20_wavelength(40)]

    def chain(radii):
        c = syn20_chain()
        relays = [k for k, it in c.items() if it["name"].endswith("c")]
        for k, r in zip(relays, radii):
            c[k] = dict(c[k], aperture=dict(c[k]["aperture"], xrad=r, yrad=0.9 * r), save=True)
        return c

    same = [chain([0.5] * 5) for _ in wls]
    many = [chain([0.5, 0.45, 0.4, 0.35, 0.3]) for _ in wls]  # with `same` before and after: 11 distinct record sets > the 8 kept

    def fields(res):
        return [(k, r[k]["wfo"]) for r in res for k in sorted(r)]

    dev = _lib.DeviceFields(n, len(wls))
    try:
        a1 = fields(prun.run_batch(1.0, wls, n, 4, ON_AXIS, same, outputs=("wfo",), dev=dev))
        b1 = fields(prun.run_batch(1.0, wls, n, 4, ON_AXIS, many, outputs=("wfo",), dev=dev))
        a2 = fields(prun.run_batch(1.0, wls, n, 4, ON_AXIS, same, outputs=("wfo",), dev=dev))   # after evictions
        b2 = fields(prun.run_batch(1.0, wls, n, 4, ON_AXIS, many, outputs=("wfo",), dev=dev))
    finally:
        dev.close()
    fresh_a = fields(prun.run_batch(1.0, wls, n, 4, ON_AXIS, same, outputs=("wfo",)))
    fresh_b = fields(prun.run_batch(1.0, wls, n, 4, ON_AXIS, many, outputs=("wfo",)))
    for got in (a1, a2):
        assert all(k == kk and np.array_equal(x, y) for (k, x), (kk, y) in zip(got, fresh_a))
    for got in (b1, b2):
        assert all(k == kk and np.array_equal(x, y) for (k, x), (kk, y) in zip(got, fresh_b))
    old = prun.FUSE_APERTURES
    prun.FUSE_APERTURES = False
    try:
        alone = fields(prun.run_batch(1.0, wls, n, 4, ON_AXIS, many, outputs=("wfo",)))
    finally:
        prun.FUSE_APERTURES = old
    for (k, x), (kk, y) in zip(b1, alone):
        assert k == kk and rel_err(x, y) < 1e-12, k
    assert rel_err(b1[-1][1], a1[-1][1]) > 1e-6  # the two chains really differ


def test_bench_two_self_launched_ranks_on_one_gpu():
    """`python bench.py --gpus 2` with no launcher in the environment: bench.py starts its own two ranks before it
    touches the GPU, they share this box's one GPU over the TCP transport (PAOS_BENCH_REHEARSAL=1: the N > 1 control
    flow -- launch, rendezvous, ONE broadcast, shards, barrier, MAX -- end to end; the rate means nothing), and the
    parent relays rank 0's JSON line.  Without --allow-tcp a run that did not end on RCCL exits 3 AND prints a line
    with value null and every rank's bring-up note.  bench.py is started from the fork server (no exec from this
    process, which holds a GPU context)."""
    import json
    import multiprocessing as mp

    import rccl_pair_worker

    ctx = mp.get_context("forkserver")
    import os
    import tempfile

    detail = os.path.join(tempfile.mkdtemp(prefix="paos_bench_"), "detail.json")
    small = ["--gpus", "2", "--grid", "1024", "--batch", "4", "--steps", "2", "--warmup", "1", "--no-cpu-baseline",
             "--no-extras", "--no-traffic", "--detail", detail]

    def bench(argv, env):
        out = ctx.Queue()
        p = ctx.Process(target=rccl_pair_worker.run_bench, args=(argv, env, out))
        p.start()
        res = out.get(timeout=1000)
        p.join(timeout=60)
        return res

    rc, stdout, stderr = bench(small + ["--allow-tcp"], {"PAOS_BENCH_REHEARSAL": "1"})
    assert rc == 0, (rc, stderr)
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["value"] > 0 and line["config"]["ranks_seen"] == 2
    assert line["config"]["devices_seen"] == [0, 0] and line["config"]["transport"] == "socket"
    assert line["config"]["launcher"].startswith("self") and len(lines[0]) < 4096
    # (round 5: the contract line is the contract's keys only; everything else is in the detail record)
    assert {"roofline", "cpu_baseline", "dtype", "ms_per_step"} <= set(line) and line["roofline"]["launches"] > 0
    full = json.load(open(detail))
    assert full["sweep"]["walked"] is True and full["value"] == pytest.approx(line["value"], rel=1e-4)
    assert abs(full["power_check"] - 1.0) < 1e-9 or full["power_check"] > 0.0
    print("two self-launched ranks on one GPU:", round(line["value"], 1), "wavefronts/s (rehearsal)", line["config"]["transport"])

    # the driver's command: an external launcher (python -m torch.distributed.run) starts the ranks, bench.py joins them
    rc, stdout, stderr = bench(small + ["--allow-tcp"], {"PAOS_BENCH_REHEARSAL": "1", "LAUNCH_WITH_TORCHRUN": "1"})
    assert rc == 0, (rc, stderr)
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["value"] > 0 and line["config"]["launcher"].startswith("external")

    # asking for RCCL with two ranks on a ONE-GPU box: rank 1 finds no device 1 -> the ranks agree on TCP -> exit 3
    # with a null line that says so
    rc, stdout, stderr = bench(small, {})
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    if rc == 3:
        assert len(lines) == 1, (stdout, stderr)
        line = json.loads(lines[0])
        assert line["value"] is None and line["config"]["transport"] == "socket" and line["config"]["ranks_seen"] == 2
        assert "bring-up notes per rank: 0:" in line["error"] or "bring-up notes per rank: 1:" in line["error"], line
        print("no-RCCL record:", line["error"])
    else:  # RCCL accepted two ranks on one device (not seen so far), or the bring-up failed loudly: never a silent number
        assert rc != 0 or (len(lines) == 1 and json.loads(lines[0])["config"]["transport"] == "rccl"), (rc, stdout, stderr)


def test_a_ticket_kept_for_long_does_not_block_the_ring():
    """The power tickets come off a ring of 64 slots; a caller that keeps one ticket for long (bench.py keeps the last
    step's) must not make the library report "64 outstanding" when the ring comes round to it (round 4: found with
    bench.py --steps 20).  65 outstanding tickets are still refused."""
    from paos_amd import _lib

    dev = _lib.DeviceFields(256, 2)
    try:
        dev.fill(1.0 + 0.0j)
        keep = dev.norm2_enqueue()
        for _ in range(200):
            t = dev.norm2_enqueue()
            assert t != keep
            assert np.array_equal(dev.norm2_fetch(t), [256.0 * 256.0] * 2)
        held = [dev.norm2_enqueue() for _ in range(_lib.NORM_SLOTS - 1)]
        with pytest.raises(_lib.PaosHipError, match="outstanding"):
            dev.norm2_enqueue()
        assert np.array_equal(dev.norm2_fetch(keep), [256.0 * 256.0] * 2)
        for t in held:
            dev.norm2_release(t)
        assert np.array_equal(dev.norm2_fetch(dev.norm2_enqueue()), [256.0 * 256.0] * 2)
    finally:
        dev.close()


def test_record_windows_follow_the_lines_a_pass_reads():
    """Round 4: aperture line records are rendered only for the lines a pass's live tiles read (a quarter of them
    behind a clear aperture at zoom 4).  A set found in the context's store is good only if it was rendered that far:
    the same chain on the same context with the pruning on (narrow windows), off (every line is read: the kept sets
    must be rendered again, not trusted) and on again -- every run equal to a fresh context's, bit for bit."""
    import paos_amd.run as prun
    from paos_amd import _lib
    from paos_amd.chains import syn20_chain, syn20_wavelength

    n = 1024
    wls = [syn20_wavelength(3), syn20_wavelength(77)]
    chains = [syn20_chain() for _ in wls]

    def psfs(dev):
        return [r[20]["psf"] for r in prun.run_batch(1.0, wls, n, 4, ON_AXIS, chains, outputs=("psf",), dev=dev)]

    fresh = psfs(None)
    dev = _lib.DeviceFields(n, len(wls))
    try:
        runs = []
        for prune in (True, False, True, False):
            dev.set_pruning(prune)
            runs.append(psfs(dev))
            found, rendered = dev.record_set_stats()
            print(f"pruning {prune}: records found {found}, rendered {rendered}")
    finally:
        dev.close()
    for got in runs:
        assert all(np.array_equal(a, b) for a, b in zip(got, fresh))
    # the un-pruned runs could not use what the pruned ones had rendered (narrower windows): they rendered again
    assert rendered >= 12


@pytest.mark.parametrize("seed", range(6))
def test_random_chains_on_the_production_kernels_vs_the_numpy_model(seed):
    """Differential test of the pass kernels beyond the fixed prescriptions: random chains (lenses, gaps, nanometre
    hops, flat windows, apertures, saved flats -- tests/test_host_logic.py::_random_chain) at 1024^2, the smallest grid
    of the production kernel, two wavelengths per batch, on the GPU against the NumPy model of the device contract
    (tests/fakes.py) driven by the same planner and pass compiler: every saved field to 1e-11, max-norm and L2."""
    from fakes import ModelDevice
    from test_host_logic import _random_chain

    import paos_amd.run as prun
    from paos_amd.run import _Item, _walk, run_batch

    rng = np.random.default_rng(4200 + seed)
    chain = _random_chain(rng, int(rng.integers(6, 12)))
    wls = [1.0e-6, float(rng.choice([1.3e-6, 1.7e-6, 2.3e-6]))]
    n = 1024
    prun.FUSE_APERTURES = [True, "auto"][seed % 2]
    try:
        try:
            got = run_batch(1.0, wls, n, 4, ON_AXIS, [chain, chain], outputs=("wfo",))
        except (ValueError, AssertionError, TypeError) as exc:
            pytest.skip(f"the planner refuses this draw like the reference would ({type(exc).__name__}: {exc})")
        dev = ModelDevice(n, 2)
        states = [_Item(1.0, wl, n, 4, ON_AXIS) for wl in wls]
        want = {}

        def on_saved(key, items, plans, wfe):
            for i, it in enumerate(items):
                if it["save"]:
                    want.setdefault(i, {})[it["num"]] = dev.download(i)

        _walk(dev, states, [chain, chain], on_saved, fresh=1.0 + 0.0j)
    finally:
        prun.FUSE_APERTURES = "auto"
    worst = 0.0
    for i in range(2):
        assert sorted(got[i]) == sorted(want[i])
        for k in want[i]:
            e, e2 = rel_err(got[i][k]["wfo"], want[i][k]), l2_rel_err(got[i][k]["wfo"], want[i][k])
            worst = max(worst, e, e2)
            assert e < 1e-11 and e2 < 1e-11, (seed, i, k, e, e2)
    print(f"seed {seed}: {len(chain)} surfaces, {len(want[0])} saved, worst error {worst:.1e}")


def test_power_summed_by_the_storing_pass_equals_the_separate_reduction():
    """Round 4: the power of a saved surface rides on the pass that stores its field (STORE = 2 builds of the pass kernel,
    paos_run_program: final_intensity = 2).  Ariel_AIRS-CH0 (12 saved surfaces, apertures riding on passes) and
    Excite_TEL at 1024^2 / 2048^2, fp64 and fp32: the powers equal those of the ordinary reductions
    (PAOS_POWER_ON_STORE off) and the sum over the downloaded field.  (Path against path; the sums themselves are held to a
    long-double reference by tests/test_gpu_ledger_xprec.py::test_power_on_store_against_long_double.)"""
    import paos_amd.run as prun
    from paos_amd.chains import parse_config_variant
    from paos_amd.run import run_batch

    for name, n, sweep in (("Ariel_AIRS-CH0", 1024, [1.95, 3.9]), ("Excite_TEL", 2048, [1.0, 3.4])):
        pup, par, wls, fields, chains = parse_config_variant(os.path.join(LENS, name + ".ini"), sweep)
        w = [1.0e-6 * x for x in wls]
        for precision, tol in (("fp64", 1e-12), ("fp32", 2e-6)):
            got = run_batch(pup, w, n, par["zoom"], fields[0], chains, outputs=(), precision=precision)
            prun.POWER_ON_STORE = False
            try:
                want = run_batch(pup, w, n, par["zoom"], fields[0], chains, outputs=("wfo",), precision=precision)
            finally:
                prun.POWER_ON_STORE = True
            worst = 0.0
            for i in range(len(w)):
                assert sorted(got[i]) == sorted(want[i])
                for k in want[i]:
                    direct = float(np.sum(np.abs(want[i][k]["wfo"].astype(np.complex128)) ** 2))
                    worst = max(worst, abs(got[i][k]["power"] - want[i][k]["power"]) / want[i][k]["power"])
                    assert abs(got[i][k]["power"] - want[i][k]["power"]) <= tol * want[i][k]["power"], (name, precision, i, k)
                    assert abs(got[i][k]["power"] - direct) <= max(tol, 1e-12) * direct * 10, (name, precision, i, k)
            print(f"{name} {n}^2 {precision}: {len(want[0])} saved surfaces, worst power difference {worst:.1e}")


def test_a_stop_whose_scaling_rides_on_the_next_pass():
    """Round 4: Excite_TEL's stop (M1) sits behind a pass program; its power comes off that program's last pass and its
    scaling 1 / sqrt(P) is multiplied into the middle slot of the NEXT program's first pass (paos_stop_defer_last_power):
    the stop costs no sweep over the field.  A lean walk (the ride) against the same walk with the scaling sweep at the
    stop and against the round-3 make_stop: PSFs and powers to 1e-13 (fp32: 1e-6); with arrays downloaded at the stop
    (the library applies the factor before anything else reads the field) bit-identical to the sweep.  (Which of the two
    happened, and the stop's error against a long-double reference:
    tests/test_gpu_ledger_xprec.py::test_stop_from_a_known_power_swept_deferred_and_riding.)"""
    import paos_amd.run as prun
    from paos_amd import _lib
    from paos_amd.chains import parse_config_variant
    from paos_amd.run import run_batch

    n = 2048
    pup, par, wls, fields, chains = parse_config_variant(os.path.join(LENS, "Excite_TEL.ini"), [1.0, 2.2, 3.4])
    w = [1.0e-6 * x for x in wls]
    args = (pup, w, n, par["zoom"], fields[0], chains)

    def lean(precision):
        dev = _lib.DeviceFields(n, len(w), precision)
        try:
            res = run_batch(*args, outputs=(), dev=dev, keep_psf=True, precision=precision)
            return res, [dev.psf_fetch(i) for i in range(len(w))]
        finally:
            dev.close()

    for precision, tol in (("fp64", 1e-13), ("fp32", 2e-6)):
        ride, ride_psf = lean(precision)
        prun.STOP_DEFERRED = False
        try:
            sweep, sweep_psf = lean(precision)
            prun.STOP_FROM_PROGRAM = False
            try:
                old, old_psf = lean(precision)
            finally:
                prun.STOP_FROM_PROGRAM = True
        finally:
            prun.STOP_DEFERRED = True
        for i in range(len(w)):
            assert rel_err(ride_psf[i], old_psf[i]) < tol and rel_err(sweep_psf[i], old_psf[i]) < tol, (precision, i)
            for k in old[i]:
                for got in (ride, sweep):
                    assert abs(got[i][k]["power"] - old[i][k]["power"]) <= max(tol, 1e-12) * old[i][k]["power"], (precision, i, k)
        print(f"Excite_TEL {n}^2 {precision}: ride vs make_stop PSF {max(rel_err(a, b) for a, b in zip(ride_psf, old_psf)):.1e}")
    # arrays downloaded at the stop: the pending factor is applied first, by the same sweep
    a = run_batch(*args, outputs=("wfo",))
    prun.STOP_DEFERRED = False
    try:
        b = run_batch(*args, outputs=("wfo",))
    finally:
        prun.STOP_DEFERRED = True
    for i in range(len(w)):
        for k in b[i]:
            assert np.array_equal(a[i][k]["wfo"], b[i][k]["wfo"]), (i, k)
