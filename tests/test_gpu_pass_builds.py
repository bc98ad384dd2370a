"""Every build of the frugal pass kernel a program can reach (tests/pass_builds.py: 820 built records less UNREACHABLE), one
case per record: the recipe's program runs through the C ABI, DeviceFields.pass_builds() must name exactly the record, and items
0 and 1 are held to the long-double restatement of xprec_np on sampled lines at the bound of the case -- the harness and the
numbers of test_gpu_xprec.py (xprec_np.check with bound(n, transforms, K); complex64: + K FP32_FACTOR_BOUND["frugal"]; PSF rows
at twice the bound; powers at 1e-14 / 1e-6 of the long-double sum) and, for the two-axis recipes, of
test_single_table_pass_on_one_line_workgroups / test_gpu_central_half.py.  A disabled third item comes back bit for bit; it
holds one field per family, is never changed, and so is uploaded once per context.  Fields behind an entry box hold NaN beyond the
8 x 8 blocks of the box (test_gpu_xprec._poison, test_gpu_central_half._boxed): a build that loads outside its window shows.

One context per (family, batch) lives for the module; the central-half records run on one created under PAOS_CENTRAL_HALF=1.
The bound of an item counts the transforms that are switched on for it.  When the module ends, the fixture prints per family the
largest kernel error as a fraction of its bound and the record that produced it (run with -s)."""
import numpy as np
import pytest

import pass_builds as pb
import test_gpu_central_half as tc
import test_gpu_xprec as tx
import xprec_np as xp

pytestmark = pytest.mark.gpu

CASES = [(p, n, r) for p, n in pb.FAMILIES for r in pb.built_records(p, n) if (p, n, r) not in pb.UNREACHABLE]
PTOL = {"fp64": 1e-14, "fp32": 1e-6}  # test_storing_builds_psf_and_power
WORST = {}  # family -> (fraction of the bound, record): printed when the module's contexts are closed


def _id(case):
    p, n, r = case
    return f"{p}-{n}-" + "-".join(f"{k}{v}" for k, v in zip(("ax", "pre", "mid", "nfft", "st", "tab", "fuse", "one", "ch"), r))


@pytest.fixture(scope="module")
def contexts():
    """(precision, n, batch, central) -> (DeviceFields, {"bystander": the seed item 2 holds}), created once; a new family closes
    the contexts of the one before."""
    lib = tx._lib()
    held = {}

    def get(precision, n, batch, central):
        key = (precision, n, batch, central)
        if key not in held:
            for k in [k for k in held if k[:2] != key[:2]]:
                held.pop(k)[0].close()
            held[key] = (tc._device(lib, batch, True) if central else lib.DeviceFields(n, batch, precision), {"bystander": None})
        return held[key]

    yield get
    for dev, _ in held.values():
        dev.close()
    for family, (frac, record) in sorted(WORST.items()):
        print(f"\nPASS-BUILDS {family[0]} {family[1]}: worst kernel error {frac:.3f} of its bound, record {dict(zip(pb.FIELDS, record))}")


_MASKS, _POWER, _BYSTANDER = {}, {}, {}


def _bystander(n, precision):
    """What a context holds of the bystander's field after upload (complex64 contexts round it), once per family."""
    key = (n, precision)
    if key not in _BYSTANDER:
        _BYSTANDER.clear()
        _BYSTANDER[key] = tx._as_input(tx._field(n, pb.BYSTANDER_SEED), precision)
    return _BYSTANDER[key]


def _mask(dev, n, params):
    key = (n, tuple(params))
    if key not in _MASKS:
        if len(_MASKS) >= 8:
            _MASKS.clear()
        _MASKS[key] = dev.aperture_mask(tx._lib().SHAPE_ELLIPSE, list(params))
    return _MASKS[key]


def _inputs(n, spec, precision):
    """-> (what is uploaded, what the reference starts from) per item."""
    up, ref = [], []
    for i, seed in enumerate(spec["seeds"]):
        bystander = spec["batch"] == 3 and i == 2
        if spec["kind"] == "whole" or bystander:
            f = z = tx._field(n, seed)
        elif spec["kind"] == "window":
            # the box, zeros around it as far as its 8 x 8 blocks reach, NaN beyond them; the reference starts from zeros
            (r0, r1), (c0, c1) = spec["rows"] or (0, n), spec["cols"] or (0, n)
            z = np.zeros((n, n), dtype=np.complex128)
            z[r0:r1, c0:c1] = tx._field(n, seed)[r0:r1, c0:c1]
            f = np.full((n, n), np.nan + 1j * np.nan, dtype=np.complex128)
            rb, cb = slice((r0 // 8) * 8, -(-r1 // 8) * 8), slice((c0 // 8) * 8, -(-c1 // 8) * 8)
            f[rb, cb] = z[rb, cb]
        else:
            f = tc._boxed(seed, spec["axis"], spec["window"][i], spec["lines"])
            z = tc._boxed(seed, spec["axis"], spec["window"][i], spec["lines"], stale=False)
        up.append(f)
        ref.append(z if precision == "fp64" else tx._as_input(z, precision))
    return up, ref


def _sampled(n):
    """xprec_np.sample_lines; at 4096^2 every second one of them (and the last line): still both edges, one side of every
    boundary of 64 lines and of the block rows around the start, the middle and the end, and the stride.  (Every fourth line was
    measured as well: the 4096^2 complex128 family took 210 s either way -- a case's time is its fields, not its reference.)"""
    lines = xp.sample_lines(n)
    return lines if n < 4096 else np.union1d(lines[::2], lines[-1:])


def _item_counts(lib, rc, i):
    """(transforms switched on for item i, the product of its squared scales in long double)."""
    nfft, factor = 0, np.longdouble(1.0)
    for p in rc.passes:
        for ctl in (p.get("fft1", -1), p.get("fft2", -1)):
            if ctl >= 0 and rc.blocks[ctl, i, 0] != 0.0:
                nfft += 1
        for slot in ("pre", "mid"):
            for kind, _, blk in p.get(slot, ()):
                if kind == lib.PW_SCALE and rc.blocks[blk, i, 0] != 0.0:
                    factor = factor * np.longdouble(rc.blocks[blk, i, 3]) ** 2
    return nfft, factor


def _note(family, frac, record):
    if frac > WORST.get(family, (0.0, None))[0]:
        WORST[family] = (frac, record)


def _hold(got, ref, yard, axis, n, nfft, k, precision, what, family, record, psf=False):
    """The project's measures: xprec_np.check (complex128 fields), bound + K FP32_FACTOR_BOUND (complex64), twice the bound (PSFs);
    the NumPy yardstick in the kernel's precision stays below half of what the kernel is held to."""
    if psf:
        ref, yard = ref.real ** 2 + ref.imag ** 2, np.abs(yard) ** 2
    if precision == "fp64":
        b_l2, b_el = xp.bound(n, nfft, k, precision)
    else:
        b_l2, b_el = (b + k * tx.FP32_FACTOR_BOUND["frugal"] for b in xp.bound(n, nfft, 0, precision))
    if psf:
        b_l2, b_el = 2 * b_l2, 2 * b_el
    if precision == "fp64" and not psf:
        g_l2, g_el, y_l2, y_el, msg = xp.check(got, ref, yard, axis, n, nfft, k, precision, what)
    else:
        g_l2, g_el = xp.line_errors(got, ref, axis)
        y_l2, y_el = xp.line_errors(yard, ref, axis)
        msg = (f"{what}: kernel L2 {g_l2:.3g} / element {g_el:.3g}; NumPy {precision} yardstick L2 {y_l2:.3g} / element {y_el:.3g}; "
               f"bound L2 {b_l2:.3g} / element {b_el:.3g}")
        assert b_l2 >= 2 * y_l2 and b_el >= 2 * y_el, "bound tighter than twice the yardstick -- " + msg
        assert g_l2 <= b_l2 and g_el <= b_el, msg
    _note(family, max(g_l2 / b_l2, g_el / b_el), record)
    return msg


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_build_against_long_double(case, contexts):
    lib = tx._lib()
    precision, n, r = case
    rc = pb.recipe(precision, n, r)
    spec = rc.fields
    dt = tx.DT[precision]
    dev, held = contexts(precision, n, spec["batch"], bool(r.central))
    up, zin = _inputs(n, spec, precision)
    for i, f in enumerate(up):
        if i == 2 and held["bystander"] == spec["seeds"][2]:
            continue  # (it came back bit for bit from every case since: asserted below)
        dev.upload(i, f)
    if spec["batch"] == 3:
        held["bystander"] = spec["seeds"][2]
    ticket = dev.run_passes(rc.passes, rc.blocks, **rc.kw)
    builds = dev.pass_builds()
    power = None if ticket is None else dev.norm2_fetch(ticket)
    # 1. the build
    want_launches = 1 if spec["axes"] == 1 else 2
    assert len(builds) == want_launches, f"{want_launches} launch(es) expected, the log holds {builds}"
    assert builds[rc.index] == tuple(r), (f"launch {rc.index} ran the build {dict(zip(pb.FIELDS, builds[rc.index]))}, "
                                          f"the recipe is for {dict(zip(pb.FIELDS, r))}")
    out = [dev.psf_fetch(i) if r.store == 1 else dev.download(i) for i in range(spec["batch"])]
    masks = {blk: [_mask(dev, n, q) for q in per_item] + [None] for blk, per_item in spec["apertures"].items()} or None
    family, report = (precision, n), []
    # 4. the bystander
    if spec["batch"] == 3:
        assert np.array_equal(out[2], _bystander(n, precision)), f"{_id(case)}: the disabled item changed"
    for i in range(2):
        nfft_i, pfac = _item_counts(lib, rc, i)
        what = f"{_id(case)} item {i}"
        if spec["axes"] == 1:
            # 2. sampled lines against the long-double restatement
            lines = _sampled(n)
            sel = {"rows": lines} if r.axis == 0 else {"cols": lines}
            part = zin[i][lines] if r.axis == 0 else zin[i][:, lines]
            ref = xp.run_item(part, rc.passes, rc.blocks, i, n, masks=masks, **sel)
            yard = xp.run_item(part.astype(dt), rc.passes, rc.blocks, i, n, masks=masks, dtype=dt, **sel)
            got = out[i][lines] if r.axis == 0 else out[i][:, lines]
            assert np.isfinite(got if spec["kind"] == "whole" else out[i]).all(), f"{what}: stale data reached the output"
            report.append(_hold(got, ref, yard, r.axis, n, nfft_i, rc.k, precision, what, family, r, psf=r.store == 1))
        else:
            # the first pass on its live lines, the second on sampled lines the aperture leaves non-zero
            # (test_gpu_central_half.test_single_table_pass_on_the_central_half_build)
            other = 1 - r.axis
            live = np.arange(*spec["lines"])
            m = masks[rc.passes[1]["pre"][0][2]][i]
            nonzero = np.nonzero(m.any(axis=1 if other == 0 else 0))[0]
            kept = nonzero[:: max(1, nonzero.size // 12)]
            part = zin[i][live] if r.axis == 0 else zin[i][:, live]
            sel = {"rows": live} if r.axis == 0 else {"cols": live}
            refs = []
            for d in (xp.LD, np.complex128):
                mid = xp.run_item(part, rc.passes[:1], rc.blocks, i, n, masks=masks, dtype=d, **sel)
                if other == 0:  # mid: [every row, live columns] -> rows `kept`, every column
                    u = np.zeros((kept.size, n), dtype=d)
                    u[:, live] = mid[kept]
                    refs.append(xp.run_item(u, rc.passes[1:], rc.blocks, i, n, rows=kept, masks=masks, dtype=d))
                else:           # mid: [live rows, every column] -> every row, columns `kept`
                    u = np.zeros((n, kept.size), dtype=d)
                    u[live] = mid[:, kept]
                    refs.append(xp.run_item(u, rc.passes[1:], rc.blocks, i, n, cols=kept, masks=masks, dtype=d))
            got = out[i][kept] if other == 0 else out[i][:, kept]
            dead = np.setdiff1d(np.arange(n), nonzero)
            assert not np.any(out[i][dead] if other == 0 else out[i][:, dead]), f"{what}: lines the aperture zeroes"
            report.append(_hold(got, refs[0], refs[1], other, n, nfft_i, rc.k, precision, what, family, r))
        # 3. the power of a storing build
        if r.store:
            assert not spec["apertures"], "a storing recipe carries no aperture: its power is known in closed form"
            key = (precision, n, spec["seeds"][i], spec["kind"], spec["rows"], spec["cols"])
            if key not in _POWER:
                _POWER[key] = np.sum(zin[i].real ** 2 + zin[i].imag ** 2, dtype=np.longdouble)
            exact = _POWER[key] * pfac * np.longdouble(n) ** nfft_i
            perr = abs(float((np.longdouble(power[i]) - exact) / exact))
            report.append(f"{what}: power off by {perr:.3g} relative (tolerance {PTOL[precision]:g})")
            assert perr <= PTOL[precision], report[-1]
    print("\nXPREC " + "\nXPREC ".join(report))
