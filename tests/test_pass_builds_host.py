"""The table of pass-kernel builds and recipes (tests/pass_builds.py) against the library's own statement of what is built
(paos_frugal_built -> csrc/frugal_launch.h: frugal_built) and against restatements of the host rules that lead a program to a
build (pass_program.h: lower_frugal's counting; passes.hip: can_fuse_pair's static conditions).  No device."""
import collections
import ctypes

import numpy as np
import pytest

import pass_builds as pb
import xprec_np as xp
from paos_amd import _lib


def test_long_double_is_wider_than_fp64():
    xp.require_long_double()


@pytest.mark.parametrize("precision,n", pb.FAMILIES)
def test_built_records_per_family_and_class(precision, n):
    """156 / 168 / 184 / 156 / 156, split as frugal_launch.h's comment says: 96 evaluating (12 shapes that store the field, 4
    the PSF, 8 field + power, per axis and number of transforms), 36 single table passes, 24 fused launches; 12 one-line single
    passes at 2048^2 and 4096^2 complex128; 16 central-half builds (8 fused, 8 one-line with kpre = 1) at 4096^2 complex128."""
    built = pb.built_records(precision, n)
    assert len(built) == pb.BUILT[(precision, n)] and len(set(built)) == len(built)
    classes = collections.Counter(pb.classify(r) for r in built)
    want = {"evaluating": 96, "table": 36, "fused": 24}
    if precision == "fp64" and n >= 2048:
        want["one_line"] = 12
    if precision == "fp64" and n == 4096:
        want["central"] = 16
    assert dict(classes) == want
    ev = [r for r in built if pb.classify(r) == "evaluating"]
    assert collections.Counter(r.store for r in ev) == {0: 48, 1: 16, 2: 32}
    assert all(r.kpre <= 1 and r.kmid <= 1 for r in ev if r.store == 1) and all(r.kpre <= 1 for r in ev if r.store == 2)
    assert all(r.tab and r.kpre == 1 and r.kmid == 1 and r.nfft == 2 for r in built if r.fuse)
    assert all(r.tab and not r.fuse and r.store == 0 for r in built if r.one_line)
    central = [r for r in built if r.central]
    assert all(r.tab and r.kpre == 1 and r.store == 0 and (r.fuse or r.one_line) for r in central)
    assert sum(1 for r in central if r.fuse) == (8 if central else 0)


def test_all_families_together_have_820_builds_and_72_unreachable():
    assert sum(len(pb.built_records(p, n)) for p, n in pb.FAMILIES) == 820
    assert len(pb.UNREACHABLE) == 72
    for (p, n, r), rule in pb.UNREACHABLE.items():
        assert _lib.frugal_built(p, n, r), "UNREACHABLE lists built records only"
        assert p == "fp32" and r.tab == 1 and r.fuse == 0 and "stage_groups" in rule


def test_query_refuses_unknown_families_and_out_of_range_fields():
    lib = _lib.load()
    good = (ctypes.c_int * 9)(0, 1, 1, 2, 0, 0, 0, 0, 0)
    assert lib.paos_frugal_built(_lib.PAOS_F64, 1024, good) == 1
    for precision, n in ((_lib.PAOS_F64, 512), (_lib.PAOS_F32, 1024), (_lib.PAOS_F64, 8192), (2, 2048), (-1, 4096), (_lib.PAOS_F64, 0)):
        assert lib.paos_frugal_built(precision, n, good) < 0, (precision, n)
    assert lib.paos_frugal_built(_lib.PAOS_F64, 1024, None) < 0
    with pytest.raises(ValueError):
        _lib.frugal_built("fp32", 1024, tuple(good))
    with pytest.raises(ValueError):
        _lib.frugal_built("fp64", 2048, (0, 1, 1, 2))
    base = [0, 1, 1, 2, 0, 1, 0, 0, 0]
    assert _lib.frugal_built("fp64", 4096, base)
    for k, top in enumerate(pb.FIELD_MAX):
        for v in (-1, top + 1, 1 << 20):
            rec = list(base)
            rec[k] = v
            for p, n in pb.FAMILIES:
                assert not _lib.frugal_built(p, n, rec), (pb.FIELDS[k], v)
    assert not _lib.frugal_built("fp64", 4096, [0, 1, 1, 0, 0, 1, 0, 0, 0]), "nfft = 0"


ALL = [(p, n, r) for p, n in pb.FAMILIES for r in pb.built_records(p, n)]


def test_every_built_record_is_unreachable_or_has_a_recipe_never_both():
    with_recipe = 0
    for p, n, r in ALL:
        rc = pb.recipe(p, n, r)
        assert (rc is None) == ((p, n, r) in pb.UNREACHABLE), (p, n, r)
        with_recipe += rc is not None
    assert with_recipe == 820 - len(pb.UNREACHABLE) == 748


def test_no_recipe_for_an_unbuilt_record():
    for p, n in pb.FAMILIES:
        built = set(pb.built_records(p, n))
        for r in pb.record_space():
            if r not in built:
                assert pb.recipe(p, n, r) is None, (p, n, r)


def _recipes():
    for p, n, r in ALL:
        rc = pb.recipe(p, n, r)
        if rc is not None:
            yield p, n, r, rc


def test_recipes_lower_to_their_records():
    """lower_frugal's counting gives the record's kpre, kmid and nfft (a table build folds a count to "has phases", a fused launch
    to 1 / 1), the grouping of run_passes_impl on can_fuse_pair's static conditions its `fuse`; the table / evaluating side
    follows stage_groups: phases along the lines only, complex128 for a single pass, at most half of the lines."""
    for p, n, r, rc in _recipes():
        first = rc.passes[rc.index]
        low = pb.lowered_counts(first, rc.blocks)
        assert low is not None, (p, n, r)
        kpre, kmid, nfft = low
        if r.tab:
            kpre, kmid = min(kpre, 1), min(kmid, 1)
        if r.fuse:
            kpre = kmid = 1
        assert (kpre, kmid, nfft) == (r.kpre, r.kmid, r.nfft), (p, n, r, low)
        assert pb.fuse_of_first_launch(rc.passes, rc.blocks) == r.fuse, (p, n, r)
        for q in rc.passes:
            assert pb.lowered_counts(q, rc.blocks) is not None, "every pass of a recipe runs on the frugal kernels"
            assert all(len(q.get(s, ())) <= _lib.MAX_PW for s in ("pre", "mid"))
        along = pb.phases_along_lines(first, rc.blocks)
        if r.fuse:
            assert all(pb.phases_along_lines(q, rc.blocks, True) for q in rc.passes)
            assert any(sum(1 for op in q.get(s, ()) if op[0] in (_lib.PW_QPHASE_CENTRED, _lib.PW_QPHASE_NATURAL)) == 0
                       for q in rc.passes for s in ("pre", "mid")), "a fused recipe leaves a slot to the table of ones"
        elif r.tab:
            assert along and p == "fp64"
            rows, cols = rc.kw["live_rows"], rc.kw.get("live_cols")
            lines = rows if r.axis == 0 else cols
            assert all(2 * (hi - lo) <= n for lo, hi in lines[:2]), "a single table pass works on at most half of the lines"
            low_counts = pb.lowered_counts(first, rc.blocks)
            assert low_counts[0] in (0, 1, 2) and (low_counts[0] == 2 or r.kpre == 0 or r.store), "two phases where the storing rules allow"
        else:
            assert not along or p == "fp32" or r.kpre + r.kmid == 0
        # the storing rules of run_passes_impl: every item in the last pass, its lowered counts inside the built shapes
        if r.store:
            last = rc.passes[-1]
            lk = pb.lowered_counts(last, rc.blocks)
            assert rc.kw["final_intensity"] == r.store and rc.blocks.shape[1] == 2
            assert all(pb.item_active(last, rc.blocks, it) for it in range(2))
            assert lk[0] <= 1 and (r.store == 2 or lk[1] <= 1)
        else:
            whole = pb.classify(r) in ("evaluating", "fused")
            assert rc.blocks.shape[1] == (3 if whole else 2) and (whole or rc.kw["rows_stale"]), "a third item on whole grids"
            assert not whole or not any(pb.item_active(q, rc.blocks, 2) for q in rc.passes), "a disabled third item"
            assert not whole or rc.fields["seeds"][2] == pb.BYSTANDER_SEED not in rc.fields["seeds"][:2]
        # one-line and central-half recipes: the loads of the first pass
        if r.one_line or r.central:
            pos = rc.kw["live_cols"] if r.axis == 0 else rc.kw["live_rows"]
            for lo, hi in pos[:2]:
                assert (4 * lo >= n and 4 * hi <= 3 * n) == bool(r.central), "central: every active item loads inside [n/4, 3n/4)"
                if r.one_line:
                    assert 2 * (-(-hi // 8) * 8 - (lo // 8) * 8) <= n, "one-line: at most half of the positions are loaded"
            assert rc.kw["rows_stale"]
        if r.one_line:
            assert len(rc.passes) == 2 and rc.passes[1]["axis"] == 1 - r.axis and rc.passes[1]["pre"][0][0] == _lib.PW_MASK


def test_run_time_variation_covers_what_the_builds_leave_open():
    modes, apertures, off = collections.Counter(), collections.Counter(), collections.Counter()
    scales, targets, singles = 0, set(), 0
    for p, n, r, rc in _recipes():
        first, b = rc.passes[0], rc.blocks
        slot = "pre" if any(op[0] == _lib.PW_SIGN for op in first.get("pre", ())) else "mid"
        m = [pb.slot_sign_mode(first, slot, b, it) for it in range(2)]
        assert m[0] != m[1] and tuple(m) == pb.sign_modes(p, n, r), "items 0 and 1 differ in the sign mode of one slot"
        modes.update(m)
        # transform direction, sampling and phase sign differ; a scale != 1 rides in the middle slot
        assert b[first["fft1"], 0, 1] != b[first["fft1"], 1, 1]
        sc = [b[op[2]] for op in first["mid"] if op[0] == _lib.PW_SCALE]
        assert len(sc) == 1 and sc[0][0, 3] != 1.0 and sc[0][0, 3] != sc[0][1, 3]
        scales += 1
        for q in rc.passes:
            for s in ("pre", "mid"):
                for kind, flags, blk in q.get(s, ()):
                    if kind in (_lib.PW_QPHASE_CENTRED, _lib.PW_QPHASE_NATURAL):
                        assert b[blk, 0, 4] == -b[blk, 1, 4] and abs(b[blk, 0, 4]) == 1.0
                        assert (b[blk, 0, 1], b[blk, 0, 2]) != (b[blk, 1, 1], b[blk, 1, 2])
                        for it in range(2):
                            sx, sy, coef = b[blk, it, 1:4]
                            arg = coef * ((0.5 * n * sx) ** 2 + (0.5 * n * sy) ** 2) * (pb.TWO_PI if flags & _lib.PWF_MUL2PI else 1.0)
                            hit = [t for t in pb.TARGETS if abs(arg - t) <= 1e-12 * t]
                            assert hit and arg < 1e12, (p, n, r, arg)
                            targets.add(hit[0])
        # a transform of item 1 switched off: the documented share
        which = pb.fft_off(p, n, r)
        on = [b[first["fft1"], 1, 0] != 0.0, r.nfft == 2 and b[first.get("fft2", 0), 1, 0] != 0.0]
        assert on == [which != 1, r.nfft == 2 and which != 2]
        if r.nfft == 2 and not r.one_line:
            singles += 1
            off[which] += 1
        # apertures: on the stated subset, per family, axis and class
        riding = [op for q in rc.passes[:1] for s in ("pre", "mid") for op in q.get(s, ()) if op[0] == _lib.PW_MASK]
        assert bool(riding) == pb.has_aperture(r)
        if riding:
            apertures[(p, n, r.axis, pb.classify(r))] += 1
    assert set(modes) == {0, 1, 2, 3}, "all four sign_on values occur"
    assert targets == set(pb.TARGETS)
    assert off[1] > 0 and off[2] > 0 and 0.3 * singles <= off[1] + off[2] <= 0.7 * singles, (off, singles)
    for p, n in pb.FAMILIES:
        for axis in (0, 1):
            assert apertures[(p, n, axis, "evaluating")] >= 1 and apertures[(p, n, axis, "fused")] >= 1
            assert (apertures[(p, n, axis, "table")] >= 1) == (p == "fp64")


def test_pass_builds_binding_matches_the_record_layout():
    assert pb.FIELDS == ("axis", "kpre", "kmid", "nfft", "store", "tab", "fuse", "one_line", "central")
    assert len(pb.record_space()) == 5760 == int(np.prod([top + (0 if name == "nfft" else 1) for name, top in zip(pb.FIELDS, pb.FIELD_MAX)]))
