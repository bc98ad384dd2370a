"""The builds of the frugal pass kernel by name (csrc/host.h: FrugalBuild; csrc/frugal_launch.h: frugal_built), and for every
build a program can reach a recipe: a pass program that makes passes.hip's pick_build return exactly that record.

Needs no device: ``built_records`` asks the library's host-only query (paos_frugal_built), the recipes are plain data in the
terms of the long-double harness (test_gpu_xprec._run, xprec_np.run_item).  tests/test_pass_builds_host.py holds the table to
restatements of the host rules (pass_program.h: lower_frugal; passes.hip: can_fuse_pair); tests/test_gpu_pass_builds.py runs
every recipe, reads back the build each launch took (DeviceFields.pass_builds) and holds the result to the long-double reference.

What a recipe varies inside its record is a function of the record alone (``_mix``), so a failure reproduces:
  * items 0 and 1 differ in sampling, transform direction and phase sign, and in the sign mode of one slot;
  * the middle slot carries a scale != 1, different per item;
  * item 1's first or second transform is switched off where ``_mix(record) % 4`` is 1 or 3 (two-transform first passes of the
    single-axis recipes only: half of them);
  * corner arguments come from TARGETS;
  * where nothing is stored (store = 0) and the program works on whole grids (the evaluating and the fused recipes) a third item
    has every operator disabled; the recipes behind an entry box (single table passes, one-line, central half) run on two items,
    because an untouched item there makes the library zero the surroundings of every item's box, poison included;
  * an aperture rides in the middle slot of the first pass of the store = 0, nfft = 2, (kpre, kmid) = (1, 1) records of the
    single-axis recipes: one evaluating, one table (complex128) and four fused records per family and axis (``has_aperture``)."""
from collections import namedtuple

import numpy as np

from paos_amd import _lib

FIELDS = _lib.BUILD_FIELDS
FIELD_MAX = (1, 2, 3, 2, 2, 1, 4, 1, 1)  # frugal_launch.h: kFrugalFieldMax; nfft starts at 1
FAMILIES = (("fp64", 1024), ("fp64", 2048), ("fp64", 4096), ("fp32", 2048), ("fp32", 4096))
BUILT = {("fp64", 1024): 156, ("fp64", 2048): 168, ("fp64", 4096): 184, ("fp32", 2048): 156, ("fp32", 4096): 156}
TARGETS = (1.0, 1e3, 1e6, 1e9, 0.99e12)  # phase argument at the grid corner, rad (test_gpu_xprec.TARGETS)
TWO_PI = 6.283185307179586
BYSTANDER_SEED = 4  # the disabled third item holds one field per family: it never changes, so it is uploaded once per context

Record = namedtuple("Record", FIELDS)
Recipe = namedtuple("Recipe", "passes blocks fields kw index nfft k")


def record_space():
    """Every record of the space 2 * 3 * 4 * 2 * 3 * 2 * 5 * 2 * 2 = 5760."""
    import itertools

    ranges = [range(1 if name == "nfft" else 0, top + 1) for name, top in zip(FIELDS, FIELD_MAX)]
    return [Record(*r) for r in itertools.product(*ranges)]


_BUILT = {}


def built_records(precision, n):
    """The records of the family that have a build, by brute force through the library's own statement."""
    key = (precision, n)
    if key not in _BUILT:
        _BUILT[key] = [r for r in record_space() if _lib.frugal_built(precision, n, r)]
    return _BUILT[key]


def classify(r):
    """The classes of frugal_launch.h's comment: evaluating, table, fused, one_line, central (the last two win)."""
    if r.central:
        return "central"
    if r.one_line:
        return "one_line"
    if r.fuse:
        return "fused"
    return "table" if r.tab else "evaluating"


def unreachable(precision, n, record):
    """The rule that keeps any program from getting ``record`` out of pick_build, or None.

    complex64, tab = 1, fuse = 0 (36 records per complex64 family, 72 of 820): passes.hip, stage_groups decides per launch
    whether its slots read tables, ``g.tables = g.count > 1 || (c->precision == PAOS_F64 && phases_along_lines(...))`` -- a
    single pass (g.count == 1) of a complex64 context never does, and launch_lowered's own staging goes through the same line.
    Read for every other class: each built record of the complex128 families, and the evaluating and fused ones of complex64,
    is what pick_build returns for the recipe below."""
    r = Record(*record)
    if precision == "fp32" and r.tab == 1 and r.fuse == 0:
        return "stage_groups: a single pass of a complex64 context never reads tables (g.tables needs g.count > 1 or PAOS_F64)"
    return None


def _single_table_records():
    """tab = 1, fuse = 0 on the ordinary workgroups: axis x nfft x store x {(1,0), (0,1), (1,1)} = 36."""
    return [Record(a, kp, km, nf, st, 1, 0, 0, 0) for a in (0, 1) for kp, km in ((1, 0), (0, 1), (1, 1)) for nf in (1, 2) for st in (0, 1, 2)]


# built records that no program can make pick_build return: {(precision, n, record): the rule that says so}
UNREACHABLE = {(p, n, r): unreachable(p, n, r) for p, n in FAMILIES if p == "fp32" for r in _single_table_records()}


def _mix(precision, n, r):
    h = 17 if precision == "fp64" else 5
    h = h * 3 + (n // 1024)
    for v in r:
        h = h * 7 + v + 1
    return h


def corner_coef(target, n, sx, sy, mul2pi):
    """coef so that the argument at the grid corner (g = -n/2 on both axes) is ``target`` (test_gpu_xprec._corner_coef)."""
    h2 = (0.5 * n * sx) ** 2 + (0.5 * n * sy) ** 2
    return target / (h2 * (TWO_PI if mul2pi else 1.0))


def has_aperture(r):
    return r.store == 0 and r.nfft == 2 and r.kpre == 1 and r.kmid == 1 and not r.one_line and not r.central


def fft_off(precision, n, r):
    """Which transform of item 1 is switched off in the first pass: 1, 2 or None."""
    if r.one_line or r.nfft != 2:
        return None
    return {1: 1, 3: 2}.get(_mix(precision, n, r) % 4)


class _Blocks:
    def __init__(self, batch):
        self.batch, self.rows = batch, []

    def add(self, item0, item1, off=(0.0, 0.5, 0.5, 1e-3, 1.0)):
        """One block set: items 0 and 1 as given, the bystander (if any) disabled."""
        row = [list(item0), list(item1)]
        if self.batch == 3:
            row.append(list(off))
        self.rows.append(row)
        return len(self.rows) - 1

    def array(self):
        return np.array(self.rows, dtype=np.float64)


def _sign_ops(lib, b, axis, modes):
    """Two PW_SIGN operators -- (-1)^column and (-1)^row -- whose per-item enables give item i the slot sign mode modes[i]
    (FrugalSlot::sign_on: 0 none, 1 checkerboard, 2 (-1)^position, 3 (-1)^line)."""
    along = [1.0 if m in (1, 2) else 0.0 for m in modes]
    across = [1.0 if m in (1, 3) else 0.0 for m in modes]
    x_en, y_en = (along, across) if axis == 0 else (across, along)
    bx = b.add([x_en[0], 0, 0, 0, 0], [x_en[1], 0, 0, 0, 0], off=(0.0, 0, 0, 0, 0))
    by = b.add([y_en[0], 0, 0, 0, 0], [y_en[1], 0, 0, 0, 0], off=(0.0, 0, 0, 0, 0))
    return [(lib.PW_SIGN, lib.PWF_X_ONLY, bx), (lib.PW_SIGN, lib.PWF_Y_ONLY, by)]


def sign_modes(precision, n, r):
    h = _mix(precision, n, r)
    m0 = h % 4
    return m0, (m0 + 1 + (h // 4) % 3) % 4


def _phase_ops(lib, b, n, axis, count, h, slot, along_only, flip):
    """``count`` phase operators of one slot: kinds and MUL2PI alternate, the items differ in sampling, sign and target."""
    ops = []
    for j in range(count):
        kind = lib.PW_QPHASE_CENTRED if (j + h + slot) % 2 == 0 else lib.PW_QPHASE_NATURAL
        flags = lib.PWF_MUL2PI if (j + h // 2) % 2 == 0 else 0
        items = []
        for i in range(2):
            s_along, s_across = ((0.9, 0.0) if i == 0 else (0.55, 0.0)) if along_only else ((1.0, 0.6) if i == 0 else (0.45, 1.3))
            s_along *= 1.0 + 0.125 * j
            sx, sy = (s_along, s_across) if axis == 0 else (s_across, s_along)
            target = TARGETS[(h + 2 * j + 3 * i + slot) % len(TARGETS)]
            sgn = (-1.0 if i == 0 else 1.0) * flip
            items.append([1.0, sx, sy, corner_coef(target, n, sx, sy, flags != 0), sgn])
        ops.append((kind, flags, b.add(items[0], items[1])))
    return ops


def _counts(r):
    """Phases per slot of the pass that carries the record's shape: an evaluating build's own numbers; a table slot 'with
    phases' gets two where the storing rules of run_passes_impl allow (store = 1: at most one per slot, store = 2: at most one
    in front)."""
    if not r.tab:
        return r.kpre, r.kmid
    kpre = 0 if r.kpre == 0 else (1 if r.store else 2)
    kmid = 0 if r.kmid == 0 else (1 if r.store == 1 else 2)
    return kpre, kmid


def _first_pass(lib, b, precision, n, r, axis, kpre, kmid, nfft, along_only, aperture=None, off=None, signs=True, salt=0):
    """A pass of the given shape: [signs] kpre phases | transform | scale [aperture] kmid phases | [transform]."""
    h = _mix(precision, n, r) + salt
    c1 = b.add([1.0, 0.0, 0, 0, 0], [0.0 if off == 1 else 1.0, 1.0, 0, 0, 0], off=(0.0, 0, 0, 0, 0))
    c2 = b.add([1.0, 1.0, 0, 0, 0], [0.0 if off == 2 else 1.0, 0.0, 0, 0, 0], off=(0.0, 0, 0, 0, 0))
    scale = b.add([1.0, 0, 0, 1.0 / n, 0], [1.0, 0, 0, 0.75 / n, 0], off=(0.0, 0, 0, 3.0, 0))
    sg = _sign_ops(lib, b, axis, sign_modes(precision, n, r)) if signs else []
    flip = 1.0 if h % 2 else -1.0
    pre = _phase_ops(lib, b, n, axis, kpre, h, 0, along_only, flip)
    mid = [(lib.PW_SCALE, 0, scale)]
    if aperture is not None:
        mid.append((lib.PW_MASK, 0, aperture))
    mid += _phase_ops(lib, b, n, axis, kmid, h, 1, along_only, -flip)
    if kpre > 0:
        pre = sg + pre
    else:
        mid = sg + mid  # (kpre = 0: nothing at all in front of the first transform)
    p = {"axis": axis, "fft1": c1, "pre": pre, "mid": mid}
    if nfft == 2:
        p["fft2"] = c2
    return p


def _aperture_blocks(lib, b, params):
    """Two consecutive block sets of a clear ellipse per item; returns the first one's index."""
    first = b.add(params[0], params[1], off=(0.0, 1.0, 1.0, 1.0, 1.0))
    b.add([0.0, 0.0, 32.0, lib.SHAPE_ELLIPSE, 0.0], [0.0, 0.0, 32.0, lib.SHAPE_ELLIPSE, 0.0], off=(0.0, 0.0, 32.0, lib.SHAPE_ELLIPSE, 0.0))
    return first


def _riding_aperture(n):
    return [[1.0, n / 2 + 0.3, n / 2 - 0.2, n / 10, n / 9], [1.0, n / 2 - 5.5, n / 2 + 7.25, n / 9, n / 10]]


def _k_total(passes, lib):
    return sum(1 for p in passes for slot in ("pre", "mid") for op in p.get(slot, ())
               if op[0] in (lib.PW_QPHASE_CENTRED, lib.PW_QPHASE_NATURAL))


def _nfft_total(passes):
    return sum((1 if p.get("fft1", -1) >= 0 else 0) + (1 if p.get("fft2", -1) >= 0 else 0) for p in passes)


def recipe(precision, n, record):
    """-> Recipe(passes, blocks, fields spec, run keywords, index of the launch that must carry the record, transforms of the
    program, phase factors per point), or None for a record without a build or one no program reaches.

    fields spec: {"batch", "seeds", "rows": (lo, hi) or None, "cols": ..., "kind": "whole" | "window" | "boxed",
    "apertures": {block: [[8 aperture parameters] per item]}, "axes": 1 | 2, "axis", "lines", "window"} -- "window": items 0
    and 1 live on rows x cols, zeros around it as far as its 8 x 8 blocks reach and NaN beyond them; "boxed": test_gpu_central_half._boxed(seed, axis, window, lines)."""
    lib = _lib
    r = Record(*record)
    if not _lib.frugal_built(precision, n, r) or unreachable(precision, n, r):
        return None
    kind = classify(r)
    # the bystander: where nothing is stored and the program works on whole grids.  (Behind an entry box an item that no pass
    # touches makes run_passes_impl write the zeros the box stands for, for every item -- the poison around the box would be gone
    # before the first pass loads anything; those recipes run on two items.)
    batch = 3 if r.store == 0 and kind in ("evaluating", "fused") else 2
    b = _Blocks(batch)
    h = _mix(precision, n, r)
    spec = {"batch": batch, "seeds": (h % 4, (h + 1) % 4, BYSTANDER_SEED)[:batch], "rows": None, "cols": None, "kind": "whole",
            "apertures": {}, "axes": 1, "axis": r.axis, "lines": None, "window": None}
    kw = {}
    if r.store:
        kw["final_intensity"] = r.store
    full = [0.0, float(n)]
    if kind in ("evaluating", "table", "fused") or (kind == "central" and r.fuse):
        along_only = kind != "evaluating"
        ap = None
        if has_aperture(r):
            params = _riding_aperture(n)
            ap = _aperture_blocks(lib, b, params)
            spec["apertures"][ap] = [p + [0.0, 0.0, 32.0] for p in params]
        kpre, kmid = (2, 1) if r.fuse else _counts(r)
        passes = [_first_pass(lib, b, precision, n, r, r.axis, kpre, kmid, r.nfft, along_only, ap, fft_off(precision, n, r))]
        if r.fuse:
            # the passes that ride along: [1], [2], [2][1], [2][2] transforms.  The second pass has nothing in front of its first
            # transform, the third nothing but a scale behind it -- slots that read the table of ones --, and either keeps to the
            # storing rules of a last pass (at most one phase per slot)
            tail = {1: (1,), 2: (2,), 3: (2, 1), 4: (2, 2)}[r.fuse]
            for q, nf in enumerate(tail):
                kp, km = (0, 1) if q == 0 else (1, 0)
                passes.append(_first_pass(lib, b, precision, n, r, r.axis, kp, km, nf, True, signs=False, salt=q + 1))
        if kind == "table":
            # at most half of the lines: rows [n/4, 3n/4) hold the field and the others stand for zeros, or -- a column pass -- columns
            lo, hi = n // 4, 3 * n // 4
            win = [[lo, hi]] * 2
            if r.axis == 0:
                spec.update(kind="window", rows=(lo, hi))
                kw.update(live_rows=np.array(win, dtype=np.float64), rows_stale=True)
            else:
                spec.update(kind="window", cols=(lo, hi))
                kw.update(live_rows=np.array([full] * batch, dtype=np.float64), live_cols=np.array(win, dtype=np.float64), rows_stale=True)
        if kind == "central":
            # every active item loads inside [n/4, 3n/4): the entry box of test_gpu_central_half (64 lines, two windows)
            lines, windows = (n // 2 - 32, n // 2 + 32), [(1532, 2564), (1024, 3072)]
            ln = [list(lines), list(lines)]
            ps = [list(windows[0]), list(windows[1])]
            rows, cols = (ln, ps) if r.axis == 0 else (ps, ln)
            kw.update(live_rows=np.array(rows, dtype=np.float64), live_cols=np.array(cols, dtype=np.float64), rows_stale=True)
            spec.update(kind="boxed", lines=lines, window=windows)
        return Recipe(passes, b.array(), spec, kw, 0, _nfft_total(passes), _k_total(passes, lib))
    # one-line single table passes (and their central-half builds): entry box, the pass of the record along its axis, then a pass
    # along the other axis whose aperture keeps at most half of ITS lines -- so the first loads and stores at most half
    central = kind == "central"
    other = 1 - r.axis
    lines = (n // 2 - 32, n // 2 + 32)
    window = (3 * n // 8 + 3, 5 * n // 8 - 3) if central else (n // 8 + 3, 3 * n // 8 + 3)
    wc = 0.5 * (window[0] + window[1])
    kpre, kmid = _counts(r)
    passes = [_first_pass(lib, b, precision, n, r, r.axis, kpre, kmid, r.nfft, True)]
    # (both extents of the aperture inside the window: a two-transform first pass hands its window back)
    e0, e1 = n / 10, n / 9
    if other == 0:  # the second pass runs along rows: its lines are rows, the window is a range of rows
        params = [[1.0, n / 2 + 0.3, wc - 0.2, e0, e1], [1.0, n / 2 - 5.5, wc + 7.25, e1, e0]]
    else:
        params = [[1.0, wc + 0.3, n / 2 - 0.2, e1, e0], [1.0, wc - 5.5, n / 2 + 7.25, e0, e1]]
    ap = _aperture_blocks(lib, b, params)
    spec["apertures"][ap] = [p + [0.0, 0.0, 32.0] for p in params]
    fwd = b.add([1.0, 0.0, 0, 0, 0], [1.0, 0.0, 0, 0, 0], off=(0.0, 0, 0, 0, 0))
    passes.append({"axis": other, "fft1": fwd, "pre": [(lib.PW_MASK, 0, ap)]})
    ln = [list(lines), list(lines)]
    ps = [list(window), list(window)]
    rows, cols = (ln, ps) if r.axis == 0 else (ps, ln)
    kw.update(live_rows=np.array(rows, dtype=np.float64), live_cols=np.array(cols, dtype=np.float64), rows_stale=True)
    spec.update(kind="boxed" if central else "window", axes=2, lines=lines, window=[window, window])
    if not central:
        spec.update(rows=lines if r.axis == 0 else window, cols=window if r.axis == 0 else lines)
    return Recipe(passes, b.array(), spec, kw, 0, _nfft_total(passes), _k_total(passes, lib))


# ---- restatements of the host rules (what test_pass_builds_host.py holds the recipes to) ---------------------------------
def lowered_counts(p, blocks, lib=_lib):
    """pass_program.h, lower_frugal: (kpre, kmid, nfft) of a pass as lowered -- phases per slot, every enabled phase with
    |sgn| = 1 (else None: the generic kernel), and a sign, a scale != 1 or an aperture in an otherwise phase-free first slot
    of an active item promotes kpre 0 -> 1."""
    blocks = np.asarray(blocks)
    batch = blocks.shape[1]
    k = [0, 0]
    if p.get("post") or p.get("fft1", -1) < 0 or p["axis"] not in (0, 1):
        return None
    for l, slot in enumerate(("pre", "mid")):
        for kind, _, blk in p.get(slot, ()):
            if kind in (lib.PW_QPHASE_CENTRED, lib.PW_QPHASE_NATURAL):
                k[l] += 1
                if any(blocks[blk, it, 0] != 0.0 and abs(blocks[blk, it, 4]) != 1.0 for it in range(batch)):
                    return None
    if k[0] > 2 or k[1] > 3:
        return None
    if k[0] == 0:
        for it in range(batch):
            if not item_active(p, blocks, it):
                continue
            for kind, _, blk in p.get("pre", ()):
                q = blocks[blk, it]
                if q[0] != 0.0 and (kind in (lib.PW_SIGN, lib.PW_MASK) or (kind == lib.PW_SCALE and q[3] != 1.0)):
                    k[0] = 1
    return k[0], k[1], 2 if p.get("fft2", -1) >= 0 else 1


def item_active(p, blocks, it):
    """lower_frugal: an item takes part in a pass if a transform or any operator of it is enabled."""
    ctl = [c for c in (p.get("fft1", -1), p.get("fft2", -1)) if c >= 0]
    ops = [op[2] for slot in ("pre", "mid") for op in p.get(slot, ())]
    return any(blocks[c, it, 0] != 0.0 for c in ctl + ops)


def slot_sign_mode(p, slot, blocks, it, lib=_lib):
    """lower_frugal: FrugalSlot::sign_on of item ``it`` -- 0 none, 1 checkerboard, 2 (-1)^position, 3 (-1)^line."""
    bits = 0
    for kind, flags, blk in p.get(slot, ()):
        if kind != lib.PW_SIGN or blocks[blk, it, 0] == 0.0:
            continue
        x_only, y_only = bool(flags & lib.PWF_X_ONLY), bool(flags & lib.PWF_Y_ONLY)
        along = (0 if y_only else 1) if p["axis"] == 0 else (0 if x_only else 1)
        across = (0 if x_only else 1) if p["axis"] == 0 else (0 if y_only else 1)
        bits ^= along | (across << 1)
    return {0: 0, 3: 1, 1: 2, 2: 3}[bits]


def phases_along_lines(p, blocks, or_none=False, lib=_lib):
    """passes.hip, phases_along_lines: no phase of an active item varies across the lines (and there is one, unless or_none)."""
    batch = blocks.shape[1]
    have = False
    for slot in ("pre", "mid"):
        for kind, _, blk in p.get(slot, ()):
            if kind not in (lib.PW_QPHASE_CENTRED, lib.PW_QPHASE_NATURAL):
                continue
            have = True
            for it in range(batch):
                if item_active(p, blocks, it) and blocks[blk, it, 0] != 0.0 and blocks[blk, it, 2 if p["axis"] == 0 else 1] != 0.0:
                    return False
    return have or or_none


def can_fuse_pair(p, p2, blocks):
    """passes.hip, can_fuse_pair, the conditions a program fixes before any plan: same axis, a two-transform pass in front, both
    on phases along the lines (or none), every item in both passes or in neither.  (Its remaining conditions -- equal live lines, no
    shared aperture record set -- hold for the recipes by construction: whole grids or one entry box, at most one aperture.)"""
    if lowered_counts(p, blocks) is None or lowered_counts(p2, blocks) is None or p["axis"] != p2["axis"] or p.get("fft2", -1) < 0:
        return False
    if not phases_along_lines(p, blocks, True) or not phases_along_lines(p2, blocks, True):
        return False
    return all(item_active(p, blocks, it) == item_active(p2, blocks, it) for it in range(blocks.shape[1]))


def fuse_of_first_launch(passes, blocks):
    """run_passes_impl's grouping, for the launch that starts at pass 0: FrugalBuild::fuse."""
    nf = [2 if p.get("fft2", -1) >= 0 else 1 for p in passes]
    pair = len(passes) > 1 and can_fuse_pair(passes[0], passes[1], blocks)
    triple = pair and len(passes) > 2 and can_fuse_pair(passes[1], passes[2], blocks)
    return 2 + nf[2] if triple else (nf[1] if pair else 0)
