"""The lean walk's deferred start on the NumPy model of the device (tests/fakes.py): ``_walk`` writes the first field with the
Zernike phase of the next surface on it when the device offers ``start_zernike`` (paos_start_zernike_box) and nothing sits
between the two surfaces -- and runs the two calls, in their old order, in every other case."""
import numpy as np

from fakes import ModelDevice

FIELD = {"us": 0.0, "ut": 0.0}
N = 128


class FusedModel(ModelDevice):
    """The model device with the fused call: by definition what the pair of calls leaves, with the start field's power
    (what a saved first surface reports) enqueued in between."""

    def start_zernike(self, value, shape, blocks, stop, write_rows, write_cols, nmax, kdim, table, zblocks, power=False):
        self.log.append(("start_zernike", power))
        self.start(value, shape, blocks, stop, write_rows=write_rows, write_cols=write_cols)
        seen, same_as = {}, []
        for i, b in enumerate(np.asarray(blocks, dtype=np.float64)):
            key = (b.tobytes(), float(stop[i]), tuple(write_rows[i]), tuple(write_cols[i]))
            same_as.append(seen.setdefault(key, i))
        ticket = self.norm2_enqueue(write_rows, same_as=same_as, live_cols=write_cols) if power else None
        self.zernike(nmax, kdim, table, zblocks, same_as=same_as)
        return ticket


class PairSpy(ModelDevice):
    def start(self, *a, **k):
        self.log.append(("pair_start", None))
        return super().start(*a, **k)


def _calls(dev, name):
    return [d for k, d in dev.log if k == name]


def _same(a, b, dev_a, dev_b, nb):
    assert [sorted(r) for r in a] == [sorted(r) for r in b]
    for i in range(nb):
        for k in a[i]:
            assert a[i][k]["power"] == b[i][k]["power"], (i, k)
        assert np.array_equal(dev_a.psf_fetch(i), dev_b.psf_fetch(i)), i


def test_the_walk_takes_the_fused_start_when_the_device_offers_it_and_changes_nothing():
    """A sweep batch and a Monte-Carlo batch of SYN20: with ``start_zernike`` present the walk calls it once (and neither
    ``start`` on its own behind it nor a Zernike call for that surface), without it the pair runs; powers of every saved
    surface and the kept PSFs are identical.  ``PAOS_FUSE_START=0`` (run.FUSE_START) forces the pair on the same device."""
    import paos_amd.run as prun
    from paos_amd.chains import syn20_chain, syn20_coefficients, syn20_wavelength
    from paos_amd.run import run_batch

    sweep = ([syn20_wavelength(k) for k in (0, 200, 400)], [syn20_chain() for _ in range(3)])
    monte = ([syn20_wavelength(5)] * 3, [syn20_chain(syn20_coefficients(rng_seed=s)) for s in (1, 2, 3)])
    for wls, chains in (sweep, monte):
        pair_dev, fused_dev, off_dev = PairSpy(N, 3), FusedModel(N, 3), FusedModel(N, 3)
        stats_pair, stats_fused, stats_off = {}, {}, {}
        pair = run_batch(1.0, wls, N, 4, FIELD, chains, outputs=(), dev=pair_dev, keep_psf=True, stats=stats_pair)
        fused = run_batch(1.0, wls, N, 4, FIELD, chains, outputs=(), dev=fused_dev, keep_psf=True, stats=stats_fused)
        assert prun.FUSE_START is True
        prun.FUSE_START = False
        try:
            off = run_batch(1.0, wls, N, 4, FIELD, chains, outputs=(), dev=off_dev, keep_psf=True, stats=stats_off)
        finally:
            prun.FUSE_START = True
        assert len(_calls(pair_dev, "pair_start")) == 1 and stats_pair["fused_start"] == 0
        assert _calls(fused_dev, "start_zernike") == [True] and stats_fused["fused_start"] == 1  # (S01 is saved: its power rides along)
        assert _calls(off_dev, "start_zernike") == [] and stats_off["fused_start"] == 0
        _same(fused, pair, fused_dev, pair_dev, 3)
        _same(off, pair, off_dev, pair_dev, 3)


def test_the_walk_falls_back_to_the_pair_when_something_sits_between_start_and_zernike():
    """An orthonormal pupil on the Zernike surface, a stop on it, an aperture on it, a non-lean call, a single wavefront
    whose saved Zernike surface wants its wfe map, a first surface with a lens on it: the fused call is not made and the
    results are those of the device without it."""
    from paos_amd.abcd import ABCD
    from paos_amd.chains import syn20_chain, syn20_orthonorm_chain, syn20_wavelength
    from paos_amd.run import run_batch

    wls = [syn20_wavelength(3), syn20_wavelength(77)]

    def stop_on_z(c):
        c[2] = dict(c[2], is_stop=True)
        return c

    def aperture_on_z(c):
        c[2] = dict(c[2], aperture={"shape": "elliptical", "type": "aperture", "xrad": 0.4, "yrad": 0.4, "xc": 0.0, "yc": 0.0})
        return c

    def lens_on_first(c):
        c[1] = dict(c[1], ABCDt=ABCD(thickness=0.0, curvature=0.01), ABCDs=ABCD(thickness=0.0, curvature=0.01))
        return c

    cases = [(syn20_orthonorm_chain, ()), (lambda: stop_on_z(syn20_chain()), ()), (lambda: aperture_on_z(syn20_chain()), ()),
             (syn20_chain, ("amplitude",)), (lambda: lens_on_first(syn20_chain()), ())]
    for make, outputs in cases:
        chains = [make() for _ in wls]
        a_dev, b_dev, stats = FusedModel(N, 2), ModelDevice(N, 2), {}
        a = run_batch(1.0, wls, N, 4, FIELD, chains, outputs=outputs, dev=a_dev, keep_psf=True, stats=stats)
        b = run_batch(1.0, wls, N, 4, FIELD, chains, outputs=outputs, dev=b_dev, keep_psf=True)
        assert _calls(a_dev, "start_zernike") == [] and stats["fused_start"] == 0
        _same(a, b, a_dev, b_dev, 2)
        for name in outputs:
            for i in range(2):
                for k in a[i]:
                    assert np.array_equal(a[i][k][name], b[i][k][name]), (name, i, k)
    # one wavefront, the Zernike surface saved: the caller of a single run gets the wfe map of a saved surface
    chain = syn20_chain()
    chain[2] = dict(chain[2], save=True)
    a_dev, b_dev, stats = FusedModel(N, 1), ModelDevice(N, 1), {}
    a = run_batch(1.0, wls[:1], N, 4, FIELD, [chain], outputs=(), dev=a_dev, keep_psf=True, stats=stats)
    b = run_batch(1.0, wls[:1], N, 4, FIELD, [chain], outputs=(), dev=b_dev, keep_psf=True)
    assert _calls(a_dev, "start_zernike") == [] and stats["fused_start"] == 0
    _same(a, b, a_dev, b_dev, 1)
