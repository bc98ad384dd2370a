"""Propagation loop: ``run`` (drop-in) and ``run_batch`` (many wavefronts per launch).

``run(pupil_diameter, wavelength, gridsize, zoom, field, opt_chain)`` keeps the
signature, the per-surface order of operations and the returned dictionary of
``paos.core.run.run`` (reference paos/core/run.py:30-228).  All scalar decisions
are taken on the host exactly as there (coordinate break :81-91, aperture
geometry :96-122, Zernike radius :131, gating of Magnification / ChangeMedium /
lens / propagate :181-207, ray and ABCD bookkeeping :209-219); the field never
leaves HBM except for the arrays of surfaces marked ``save``.

``run_batch`` runs B independent wavefronts (wavelengths of one lens file, or
Monte-Carlo WFE realisations -- what the reference fans out over joblib workers,
paos/core/pipeline.py:140-150) through ONE sequence of kernel launches: every
launch carries a per-item parameter block with an enable flag, so items whose
planners disagree (a ptp skipped for one wavelength, II vs OI) still share
launches.
"""
import atexit
import gc
import math
import threading
from collections.abc import Mapping, Sequence
from copy import deepcopy
from numbers import Real

import numpy as np

from . import _lib
from . import abcd as _abcd
from .abcd import ABCD
from .aperture import EllipticalAperture, RectangularAperture, make_aperture
from .coordinate_break import coordinate_break
from . import passes as _passes
from .passes import PassCompiler, SeparableCompiler
from . import phase_maps as _phase_maps
from .phase_maps import MAP_SERIAL as _MAP_SERIAL, PsdScreen, grid_sag_map
from .planner import (BeamBatch, gram_polynomials, jacobi_recurrence, orthonorm_matrix,
                      zernike_block)
from .zernike import zernike_tables

# Apertures ride on FFT passes as PW_MASK operators when the library can hold them as per-line
# records (csrc/frugal_pass.h: MaskLine; complex128, N >= 1024, untilted ellipse whose partial
# runs fit, or untilted rectangular aperture): no stand-alone pass and the fusion chain does
# not break.  PAOS_FUSE_APERTURES=0 turns it off, =1 forces it for every aperture (the generic
# kernel then uses a rendered weight map, which measured slower than a stand-alone pass).
import os as _os

FUSE_APERTURES = {"0": False, "1": True}.get(_os.environ.get("PAOS_FUSE_APERTURES", "auto"), "auto")
# The power of a saved surface whose field is exactly what its pass program stored is summed by that program's last pass
# (csrc/frugal_pass.h: STORE = 2) instead of by a reduction that reads the field back; PAOS_POWER_ON_STORE=0 switches it off.
POWER_ON_STORE = _os.environ.get("PAOS_POWER_ON_STORE", "1") != "0"
# ... and a stop right behind a pass program scales by the power that program's last pass has summed (make_stop's own
# reduction would read the field back); PAOS_STOP_FROM_PROGRAM=0 switches it off.
STOP_FROM_PROGRAM = _os.environ.get("PAOS_STOP_FROM_PROGRAM", "1") != "0"
# ... and the pass program that reaches the last surface that does anything (a saved slit with the image plane right behind
# it) stores the PSF for the inert surfaces behind it as well; PAOS_INERT_TAIL=0 switches it off.
INERT_TAIL = _os.environ.get("PAOS_INERT_TAIL", "1") != "0"
# ... and such a stop leaves even its scaling to the next pass program's first pass (paos_stop_defer_last_power);
# PAOS_STOP_DEFERRED=0 runs the scaling sweep at the stop.
STOP_DEFERRED = _os.environ.get("PAOS_STOP_DEFERRED", "1") != "0"
# ... and a lean walk's first field is written inside the aperture's bounding BOX only (rows and columns: paos_start_box,
# round 5; rounds 3-4 wrote whole rows); PAOS_START_BOX=0 writes whole rows again.
START_BOX = _os.environ.get("PAOS_START_BOX", "1") != "0"
# Items that start from the same constant under the same aperture hold copies of one field until something that depends on the
# wavelength touches them: a Zernike surface right behind the start reads one field per group of copies (paos_zernike_like,
# round 5).  PAOS_TWIN_FIELDS=0: every item's field is read.
TWIN_FIELDS = _os.environ.get("PAOS_TWIN_FIELDS", "1") != "0"
# ... and where that Zernike surface follows the start with nothing in between, a lean walk writes the first field once, with
# the phase already on it (paos_start_zernike_box) -- instead of the masked constant, read back and rewritten by the Zernike
# kernel.  PAOS_FUSE_START=0: the two calls.
FUSE_START = _os.environ.get("PAOS_FUSE_START", "1") != "0"
_MASK_RUN = 192  # kMaskW of csrc/frugal_pass.h




class _Reduction:
    """One reduction of sum |u|^2 per item that is outstanding on the device (a ticket slot of paos_norm2_enqueue* /
    paos_run_program).  The library frees the slot on the first fetch and hands it out again, so the values are fetched
    at most once and kept here; every record that the reduction answers for shares this object."""

    __slots__ = ("dev", "slot", "raw", "released")

    def __init__(self, dev, slot):
        self.dev, self.slot, self.raw, self.released = dev, int(slot), None, False

    def values(self):
        if self.raw is None:
            if self.released:
                raise RuntimeError("this power was given back unread (PowerTicket.release)")
            self.raw = self.dev.norm2_fetch(self.slot)  # synchronises the stream
        return self.raw

    def release(self):
        if self.raw is None and not self.released:
            self.dev.norm2_release(self.slot)
            self.released = True


class PowerTicket:
    """What ``run_batch(..., sync=False)`` leaves under ``'power_ticket'``: a handle to the powers (one per batch item)
    of a saved surface that are still being reduced on the GPU.  ``fetch()`` waits for them and returns the array --
    any number of times, from any of the records that share the reduction (several saved surfaces can be answered by
    one reduction: a saved slit and the image plane right behind it); ``release()`` gives the slot back unread.
    ``dev.norm2_fetch(ticket)`` / ``dev.norm2_release(ticket)`` accept the handle as well.  A power that is derived
    from the reduced one (the power BEHIND a stop that scales by it) is derived at fetch time: nothing synchronises
    before the caller asks."""

    __slots__ = ("_red", "_post")

    def __init__(self, reduction, post=None):
        self._red, self._post = reduction, post

    def fetch(self):
        v = self._red.values()
        return self._post(v) if self._post is not None else v

    def release(self):
        self._red.release()

    def __int__(self):  # the slot, for diagnostics
        return self._red.slot

    def __repr__(self):
        state = "fetched" if self._red.raw is not None else ("released" if self._red.released else "outstanding")
        return f"PowerTicket(slot {self._red.slot}, {state}{', derived' if self._post is not None else ''})"


class _PowerLedger:
    """The powers of the saved surfaces of one ``run_batch``: ``entries`` holds (_Reduction, [(item index, record)], post)
    in the order taken, ``post`` deriving the reported powers from the reduced ones.  They are fetched after the walk, so
    the host keeps planning while the GPU works -- except when a chain saves more surfaces than the library has ticket
    slots: then the oldest are fetched early (``make_room``).  Every ticket is a reduction of its own (a slot number does
    not say which: the library hands a slot out again once it was fetched or released) -- except the one a pass program
    left behind when it stored the PSF for good (``lean.final_ticket``), which answers for every saved surface from there
    on: those entries share ONE _Reduction (``final``), fetched once, also when a mid-walk drain has already read it.
    The walk ``offer``s the power a pass program summed while it stored a surface's field (csrc/frugal_pass.h:
    pow_partial); ``on_saved`` may ``claim`` it for that surface's records, and what nobody claimed is given back
    (``decline``) when the next surface begins and when the walk ends."""

    def __init__(self, dev):
        self.dev, self.entries, self.drained, self._final, self.offered = dev, [], 0, {}, None

    def final(self, ticket):
        return self._final.setdefault(ticket, _Reduction(self.dev, ticket))

    def record(self, ticket, pending, post=None, final=False):
        red = self.final(ticket) if final else _Reduction(self.dev, ticket)
        self.entries.append((red, pending, post))
        return red

    def offer(self, ticket, post=None):
        self.offered = (ticket, post)

    def claim(self, pending):
        (ticket, post), self.offered = self.offered, None
        self.record(ticket, pending, post)

    def decline(self):
        if self.offered is not None:
            self.dev.norm2_release(self.offered[0])
            self.offered = None

    def outstanding(self):
        return sum(1 for e in self.entries[self.drained:] if e[0].raw is None and not e[0].released)

    def drain(self):
        for red, pending, post in self.entries[self.drained:]:
            values = red.values()
            if post is not None:
                values = post(values)
            for i, rec in pending:
                rec["power"] = float(values[i])
        self.drained = len(self.entries)

    def make_room(self, spare=2):
        """Before a ticket is taken: fetch what is pending when the library's ring is about to fill."""
        if self.outstanding() >= _lib.NORM_SLOTS - spare:
            self.drain()

    def hand_out(self):
        """``sync=False``: handles to the reductions still outstanding instead of their values (nothing waits here)."""
        for red, pending, post in self.entries[self.drained:]:
            handle = PowerTicket(red, post)
            for i, rec in pending:
                rec["power_ticket"] = handle


class _SurfaceApertures:
    """The apertures of one surface for every wavefront of a batch, as arrays over the batch: pixel-unit centres ``ixc, iyc``
    and sizes ``ea, eb`` (semi-axes of an ellipse, FULL widths of a rectangle: wfo.py:224,261-264), ``theta``, the flags
    ``rect`` and ``obsc``, and ``on`` -- true where the item carries an aperture here (the other entries of an item that is
    off mean nothing).  Everything the walk wants to know about a surface's apertures is asked here, once: the library's
    parameter blocks, the line-record test, the live rows and columns, the start's shape -- without a Python object per
    wavefront (at 1024^2 x 256 wavefronts the per-item Python was 40 % of a step that the GPU finishes in half the time
    the host needed to describe it).  ``handle(i)`` makes the photutils-like object of item i when somebody wants to see it
    (a saved surface's record, an orthonormal Zernike pupil)."""

    def __init__(self, ixc, iyc, ea, eb, theta, rect, obsc, on):
        self.ixc, self.iyc, self.ea, self.eb, self.theta = ixc, iyc, ea, eb, theta
        self.rect, self.obsc, self.on = rect, obsc, on
        self.batch = len(ixc)
        self._handles = {}

    @classmethod
    def from_blocks(cls, shape_code, blocks):
        """From [batch][8] parameter blocks of one shape (aperture.py: block), tilt included."""
        b = np.asarray(blocks, dtype=np.float64).reshape(-1, _lib.APERTURE_STRIDE)
        return cls(b[:, 1], b[:, 2], b[:, 3], b[:, 4], b[:, 5], np.full(len(b), shape_code == _lib.SHAPE_RECT),
                   b[:, 6] != 0.0, b[:, 0] != 0.0)

    def handle(self, i):
        """The aperture object of item i (None where it has none), made when it is first looked at."""
        if not self.on[i]:
            return None
        h = self._handles.get(i)
        if h is None:
            cls = RectangularAperture if self.rect[i] else EllipticalAperture
            h = self._handles[i] = cls((float(self.ixc[i]), float(self.iyc[i])), float(self.ea[i]), float(self.eb[i]),
                                       float(self.theta[i]))
        return h

    def blocks(self):
        """[batch][8] parameter blocks of paos_aperture / paos_start (aperture.py: block; all zero for an item that is off)
        and the shape code per item."""
        b = np.zeros((self.batch, _lib.APERTURE_STRIDE), dtype=np.float64)
        b[:, 0] = 1.0
        b[:, 1], b[:, 2], b[:, 3], b[:, 4], b[:, 5] = self.ixc, self.iyc, self.ea, self.eb, self.theta
        b[:, 6] = self.obsc
        b[:, 7] = np.where(self.rect, 32.0, 0.0)
        b[~self.on] = 0.0
        return b, np.where(self.rect, float(_lib.SHAPE_RECT), float(_lib.SHAPE_ELLIPSE))

    def fits_line_records(self, n, precision):
        """May the apertures ride on a pass as per-line records (csrc/frugal_pass.h: MaskLine)?  Every item that is on must
        fit: an untilted ellipse whose partial runs fit, or an untilted clear rectangle."""
        if n < (1024 if precision == "fp64" else 2048) or not self.on.any():
            return False
        a, b = self.ea, self.eb
        with np.errstate(all="ignore"):
            ell = (a >= 2.0) & (b >= 2.0) & (2.0 * a * np.sqrt(3.0 / b) + 8.0 <= _MASK_RUN) & (2.0 * b * np.sqrt(3.0 / a) + 8.0 <= _MASK_RUN)
        rec = ~self.obsc & (a > 0.0) & (b > 0.0)
        return bool(np.all(~self.on | ((self.theta == 0.0) & np.where(self.rect, rec, ell))))

    def _clear_extent(self, centre, size, n):
        """Per item [lo, hi) along one axis outside which a clear, untilted aperture leaves exact zeros (photutils' bounding
        box, widened by a pixel), and where that holds: not for items that are off, obscuring, tilted or degenerate."""
        ext = np.where(self.rect, size / 2.0, size)
        ok = self.on & ~self.obsc & (self.theta == 0.0) & np.isfinite(centre) & np.isfinite(ext) & (ext > 0.0)
        with np.errstate(all="ignore"):
            lo = np.maximum(0, np.floor(centre - ext + 0.5) - 1)
            hi = np.minimum(n, np.ceil(centre + ext + 0.5) + 1)
        return lo, hi, ok & (lo < hi)

    def narrow_rows(self, live, n):
        """Rows that may be non-zero after the stand-alone apertures were applied; ``live`` is updated in place, one
        [lo, hi) per item."""
        lo, hi, ok = self._clear_extent(self.iyc, self.eb, n)
        for i in np.nonzero(ok)[0].tolist():
            r = live[i]
            r[0], r[1] = max(r[0], int(lo[i])), min(r[1], int(hi[i]))
            if r[0] >= r[1]:  # disjoint boxes: everything is zero; keep a token range
                r[0], r[1] = 0, 0

    def live_cols(self, n):
        """Per item the columns [lo, hi) outside which the aperture leaves exact zeros, or None when some item has no
        such aperture."""
        lo, hi, ok = self._clear_extent(self.ixc, self.ea, n)
        if not ok.all():
            return None
        return [[int(a), int(b)] for a, b in zip(lo.tolist(), hi.tolist())]

    def start_shape(self):
        """The shape code when every item carries an aperture and all are of one shape (paos_start takes one), else None."""
        if not self.on.all() or (self.rect.any() and not self.rect.all()):
            return None
        return _lib.SHAPE_RECT if self.rect[0] else _lib.SHAPE_ELLIPSE


class _Plans(list):
    """The per-item plans of one surface (``_plan_surface``): dicts with ``stop``, ``zernike``, ``phase_map``; ``ap`` is the
    surface's ``_SurfaceApertures``, or None when no item carries an aperture here.
    ``summary()``: (any stop, any Zernike, any phase map, any aperture) over the items -- looked at a dozen times per
    surface by the walk, scanned once."""

    ap = None
    _summary = None
    chief_ray = None  # (batch, 2) chief-ray positions (x, y) at a saved surface (_walk)

    def summary(self):
        if self._summary is None:
            self._summary = (any(p["stop"] for p in self), any(p["zernike"] is not None for p in self),
                             any(p["phase_map"] is not None for p in self), self.ap is not None)
        return self._summary

    def aperture(self, i):
        """The aperture object of item i at this surface, or None."""
        return self.ap.handle(i) if self.ap is not None else None


class _Item:
    """One wavefront of a walk: the beam's scalars and its field point.  (The pilot beams of all wavefronts live together
    in a ``planner.BeamBatch``, their paraxial rays in a ``_Rays``.)"""

    def __init__(self, pupil_diameter, wavelength, gridsize, zoom, field):
        # the argument checks of WFO.__init__ (wfo.py:100-103)
        assert np.log2(gridsize).is_integer(), "Grid size should be 2**n"
        assert zoom > 0, "zoom factor should be positive"
        assert pupil_diameter > 0, "beam diameter should be positive"
        assert wavelength > 0, "a wavelength should be positive"
        self.pupil_diameter, self.wavelength, self.gridsize, self.zoom = pupil_diameter, wavelength, gridsize, zoom
        self.field = field


def _fields_of(field, nb):
    """``field`` of ``run_batch``: one dict for every wavefront, or a sequence of one dict per wavefront.  Returns the list
    of ``nb`` dicts; every slope must be finite (``ValueError`` otherwise, and for a sequence of another length)."""
    if isinstance(field, Mapping):
        fields = [field] * nb
    else:
        if isinstance(field, (str, bytes)) or not isinstance(field, Sequence):
            raise ValueError("field must be a dict {'us': ..., 'ut': ...} or a sequence of one such dict per chain")
        fields = list(field)
        if len(fields) != nb:
            raise ValueError(f"one field per chain is required: {len(fields)} fields for {nb} chains")
    for f in (fields[:1] if isinstance(field, Mapping) else fields):
        if not isinstance(f, Mapping):
            raise ValueError("every field must be a dict {'us': ..., 'ut': ...}")
        for k in ("us", "ut"):
            v = f.get(k)
            if isinstance(v, bool) or not isinstance(v, Real) or not math.isfinite(float(v)):
                raise ValueError(f"field slope {k!r} must be a finite number, got {v!r}")
    return fields


class _Rays:
    """The two paraxial rays of every wavefront of a batch as arrays: ``vt`` / ``vs`` (batch, 2), started from the field
    points (run.py:64-65), and ``still`` (both rays exactly zero: an on-axis field point, whose rays stay [0, 0] under
    every ABCD matrix -- A @ 0 = 0 -- until a coordinate break moves them).  The one ray state of a walk: ``_plan_surface``
    plans the apertures from it, ``coordinate_break`` and ``advance`` move it."""

    def __init__(self, fields):
        self.vt = np.array([[0.0, f["ut"]] for f in fields], dtype=np.float64).reshape(len(fields), 2)
        self.vs = np.array([[0.0, f["us"]] for f in fields], dtype=np.float64).reshape(len(fields), 2)
        self._settle()

    def _settle(self):
        self.still = ~(self.vt.any(axis=1) | self.vs.any(axis=1))
        self._all_still = bool(self.still.all())

    def all_still(self):
        return self._all_still

    def coordinate_break(self, items):
        """``coordinate_break`` of the items that are one (run.py:81-91), once per distinct (rays, break) of the batch; the
        rays of the others stay as they are."""
        memo = {}
        for i, it in enumerate(items):
            if it["type"] != "Coordinate Break":
                continue
            key = (self.vt[i].tobytes(), self.vs[i].tobytes(), it["xdec"], it["ydec"], it["xrot"], it["yrot"])
            hit = memo.get(key)
            if hit is None:
                hit = memo[key] = coordinate_break(self.vt[i], self.vs[i], it["xdec"], it["ydec"], it["xrot"], it["yrot"], 0.0)
            self.vt[i], self.vs[i] = hit
        if memo:
            self._settle()

    def advance(self, col_t, col_s):
        """``v <- A @ v`` for the items whose rays are not zero (an on-axis item's stay [0, 0] under every matrix)."""
        if self._all_still:
            return
        mt, ms = _ray_matrices(col_t, col_s)
        idx = np.flatnonzero(~self.still)
        # (a stack of 2 x 2 @ 2 products: np.matmul runs the kernel of the single product once per item)
        self.vt[idx] = np.matmul(mt[idx], self.vt[idx][:, :, None])[:, :, 0]
        self.vs[idx] = np.matmul(ms[idx], self.vs[idx][:, :, None])[:, :, 0]

    def chief(self):
        """(batch, 2): the chief ray's position (x, y) = (vs[0], vt[0]) of every item, metres."""
        return np.stack([self.vs[:, 0], self.vt[:, 0]], axis=1)


class ABCDProduct(ABCD):
    """The accumulated ray-transfer matrix ``f_k * ... * f_1 * ABCD()`` of a saved surface
    (run.py:215-219), multiplied out when it is first read -- most callers never look at it."""

    def __init__(self, factors):  # noqa: D107 -- deliberately does not build a matrix
        object.__setattr__(self, "_factors", factors)

    def __getattr__(self, name):  # only reached while the product has not been formed
        if name in ("_mat", "_cin", "_cout", "_cache"):
            acc = ABCD()
            for f in object.__getattribute__(self, "_factors"):
                acc = f * acc
            self._mat, self._cin, self._cout, self._cache = acc._mat, acc._cin, acc._cout, {}
            return object.__getattribute__(self, name)
        raise AttributeError(name)


# Round 5: a measured surface map is one array that every wavelength of a sweep and every draw of a Monte-Carlo batch passes
# through WFO.grid_sag with the same sampling: the map the reference would build per wavefront (wfo.py:745-867: masking,
# Fourier shift, padding / cropping, resampling -- seconds at 4096^2) is built once per distinct (array, geometry) and shared;
# ``_launch_phase_maps`` then uploads it once for all the items that carry it.  An entry keeps its input array alive (so that
# the id stays unique) and is matched by the array's identity plus a digest of ALL of its bytes (xxh3: ~5 ms for a 4096^2 map
# on the GPU box's host, taken once per walk and array -- ``_SAG_SEEN``), so an array edited in place between two runs,
# wherever, is rebuilt.
_SAG_MAPS = {}


def forget_maps():
    """Drop what the module keeps between calls: the Grid Sag maps (``_sag_map_once``) with their zero-filled copies, and the
    gate arrays remembered per column of ABCD objects (``_gate_arrays``: they keep those objects alive)."""
    _SAG_MAPS.clear()
    _SAG_SEEN.clear()
    _FILLED_MAPS.clear()
    _GATE_COLUMNS.clear()
    _RAY_COLUMNS.clear()


_SAG_SEEN = {}  # id(array) -> (array, fingerprint) within ONE walk (cleared when a walk starts): the items of a batch share it


def _digest(buf):
    """A 64-bit digest of every byte of a contiguous uint8 view (xxh3: ~5 ms for the 128 MiB of a 4096^2 map on the GPU
    box's host).  Without the xxhash module: the wrap-around uint64 sums of the rows and of the columns of the bytes laid
    out as a matrix, hashed -- an edit, a flip or a roll changes one of them."""
    try:
        import xxhash

        return xxhash.xxh3_64_intdigest(buf)
    except ImportError:
        import zlib

        words = buf[: buf.size // 8 * 8].view(np.uint64)
        side = max(1, int(np.sqrt(words.size)))
        mat = words[: words.size // side * side].reshape(-1, side)
        tail = bytes(words[mat.size:]) + bytes(buf[buf.size // 8 * 8:])
        return zlib.crc32(mat.sum(axis=0, dtype=np.uint64).tobytes() + mat.sum(axis=1, dtype=np.uint64).tobytes() + tail)


def _sag_fingerprint(sag):
    """Shape, type, masked-or-not and a digest of every byte of the array (and of its mask), once per walk and array."""
    seen = _SAG_SEEN.get(id(sag))
    if seen is not None and seen[0] is sag:
        return seen[1]
    a = np.ascontiguousarray(np.ma.getdata(sag))
    digests = [_digest(a.reshape(-1).view(np.uint8))]
    if isinstance(sag, np.ma.MaskedArray) and sag.mask is not np.ma.nomask:
        digests.append(_digest(np.ascontiguousarray(np.ma.getmaskarray(sag)).reshape(-1).view(np.uint8)))
    fp = (a.shape, a.dtype.str, isinstance(sag, np.ma.MaskedArray), tuple(digests))
    _SAG_SEEN[id(sag)] = (sag, fp)
    return fp


def _sag_map_once(sag, nx, ny, delx, dely, xdec, ydec, n, dx, dy):
    key = (id(sag), nx, ny, delx, dely, xdec, ydec, n, dx, dy)
    fp = _sag_fingerprint(sag)
    hit = _SAG_MAPS.get(key)
    if hit is not None and hit[0] is sag and hit[1] == fp:
        return hit[2]
    m = grid_sag_map(sag, nx, ny, delx, dely, xdec, ydec, (n, n), dx, dy)
    if len(_SAG_MAPS) >= 2:  # (a 4096^2 map with its mask is 144 MiB: keep the last two)
        _SAG_MAPS.pop(next(iter(_SAG_MAPS)))
    _SAG_MAPS[key] = (sag, fp, m)
    return m


_NO_GEOMETRY = (float("nan"),) * 4
_RENDERED_SHAPES = {"elliptical", "rectangular", None}  # (None: an item without an aperture entry)


def _plan_apertures(aps, n, dxs, dys, rays):
    """The apertures of one surface (run.py:96-122) for all items with array arithmetic, from their ``aperture`` entries
    ``aps`` (None where an item has none): a ``_SurfaceApertures``, or None when no item carries one.  The numbers are the ones the reference forms item by item, operation for operation:
    ``vs[1] ** 2`` of a NumPy scalar is C ``pow``, which rounds differently from ``vs[1] * vs[1]`` (what an array's
    ``** 2`` forms) at ties, so the squares are taken of the scalars; the pixel quantities are the same IEEE divisions and
    sums.  While every ray is zero (no off-axis item, no coordinate break has moved them) ``xrad * sqrt(1 / (0**2 + 1))``
    and ``xdec - 0.0`` are exact identities and are not formed.  An item whose radii are not both finite has no aperture
    (run.py:112); one whose bounding box misses the grid raises the reference's ``TypeError``."""
    geo = np.array([(a["xc"], a["yc"], a["xrad"], a["yrad"]) if a is not None else _NO_GEOMETRY for a in aps], dtype=np.float64)
    xc, yc, xrad, yrad = geo[:, 0], geo[:, 1], geo[:, 2], geo[:, 3]
    dx, dy = np.asarray(dxs, dtype=np.float64), np.asarray(dys, dtype=np.float64)
    if not rays.all_still():  # run.py:97-108 with the rays of every item
        vs0, vs1, vt0, vt1 = rays.vs[:, 0], rays.vs[:, 1], rays.vt[:, 0], rays.vt[:, 1]
        with np.errstate(all="ignore"):
            xrad = xrad * np.sqrt(1 / (np.array([v ** 2 for v in vs1]) + 1))
            yrad = yrad * np.sqrt(1 / (np.array([v ** 2 for v in vt1]) + 1))
            xaper = np.where(np.isfinite(xc), xc, vs0) - vs0  # (a missing centre falls back on the chief ray)
            yaper = np.where(np.isfinite(yc), yc, vt0) - vt0
    else:
        xaper = np.where(np.isfinite(xc), xc, 0.0)  # (a missing centre falls back on the chief ray: zero here)
        yaper = np.where(np.isfinite(yc), yc, 0.0)
    on = np.isfinite(xrad) & np.isfinite(yrad)  # (never for an item without an aperture entry)
    if not on.any():
        return None
    shapes = [a["shape"] if a is not None else None for a in aps]
    rect = np.array([sh == "rectangular" for sh in shapes])
    with np.errstate(all="ignore"):
        ixc, iyc = xaper / dx + n / 2, yaper / dy + n / 2
        ea, eb = xrad / dx, yrad / dy
        xe, ye = np.where(rect, np.abs(ea / 2.0), np.abs(ea)), np.where(rect, np.abs(eb / 2.0), np.abs(eb))
        x0, x1 = np.floor(ixc - xe + 0.5), np.ceil(ixc + xe + 0.5)
        y0, y1 = np.floor(iyc - ye + 0.5), np.ceil(iyc + ye + 0.5)
        miss = ~(np.isfinite(ixc) & np.isfinite(iyc) & np.isfinite(xe) & np.isfinite(ye))
        miss |= (np.maximum(x0, 0) >= np.minimum(x1, n)) | (np.maximum(y0, 0) >= np.minimum(y1, n))
    bad = on & miss
    if not _RENDERED_SHAPES.issuperset(shapes):
        bad |= on & np.array([sh not in _RENDERED_SHAPES for sh in shapes])
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        if shapes[i] not in _RENDERED_SHAPES:
            # ("circular" needs r, which run() never passes: make_aperture raises as the reference does)
            make_aperture(n, dxs[i], dys[i], float(xaper[i]), float(yaper[i]), hx=float(xrad[i]), hy=float(yrad[i]),
                          shape=shapes[i])
        raise TypeError("aperture does not overlap the grid (mask is None in the reference)")
    obsc = np.array([a is not None and a["type"] != "aperture" for a in aps])
    return _SurfaceApertures(ixc, iyc, ea, eb, np.zeros(len(aps)), rect, obsc, on)


def _plan_surface(items, n, dxs, dys, wls, wz_of, rays):
    """Host half of one loop iteration of run.py:77-178 for every wavefront of a batch -- everything but the pilot-beam
    scalars (those are advanced for the whole batch in one C call, planner.BeamBatch).  ``dxs, dys, wls`` are the
    wavefronts' current samplings and wavelengths, ``wz_of(i)`` item i's beam radius, ``rays`` the walk's ``_Rays``.  In
    the reference's order: the coordinate break, the apertures (``_plan_apertures``: arrays over the batch), then, item
    by item in item order, what is per item by nature -- a Zernike surface's tables, a Grid Sag map, the draws of a PSD
    screen."""
    kinds = [it["type"] for it in items]  # (looked through at C speed: a step of 256 wavefronts plans 20 surfaces)
    if "Coordinate Break" in kinds:
        rays.coordinate_break(items)
    plans = _Plans({"stop": bool(it["is_stop"]), "zernike": None, "phase_map": None} for it in items)
    aps = [it.get("aperture") for it in items]
    if aps.count(None) < len(aps):
        plans.ap = _plan_apertures(aps, n, dxs, dys, rays)
    if "Zernike" in kinds or "Grid Sag" in kinds or "PSD" in kinds:
        tables = {}
        for i, (it, plan, kind) in enumerate(zip(items, plans, kinds)):
            if kind == "Zernike":
                # (run.py:124-152; what depends only on the index array / ordering / normalisation -- the continuity check,
                # the (m, n, norm) tables -- is looked up once per distinct index array of the batch)
                radius = it["Zradius"] if math.isfinite(it["Zradius"]) else wz_of(i)
                pupil = None
                if it["Zorthonorm"]:  # run.py:133-141: orthonormal over THIS surface's aperture object
                    assert "aperture" in it, "Zorthonorm requires aperture"
                    # to_mask("exact") of a RectangularAperture: photutils has no exact rectangle overlap and maps that
                    # request to the 32 x 32 sub-pixel rule (its _translate_mask_mode), i.e. the very mask WFO.aperture
                    # applies -- so both shapes are served by the aperture kernel
                    pupil = plans.aperture(i)
                    if pupil is None:
                        raise KeyError("aperture")  # the reference finds no _retval_["aperture"]
                index = np.asarray(it["Zindex"])
                key = (index.tobytes(), index.dtype.str, it["Zordering"], bool(it["Znormalize"]))
                hit = tables.get(key)
                if hit is None:
                    assert not np.any(np.diff(index) - 1), "Zernike sequence should be continuous"
                    if it["Zordering"] not in ("ansi", "noll", "fringe", "standard"):
                        raise AssertionError("Unrecognised ordering scheme.")
                    hit = tables[key] = zernike_tables(len(index), it["Zordering"], bool(it["Znormalize"]))
                m, nn, norm = hit
                plan["zernike"] = dict(m=m, n=nn, norm=norm, Z=np.asarray(it["Z"], dtype=np.float64), dx=dxs[i], dy=dys[i],
                                       radius=radius, wl=wls[i], origin=it["Zorigin"], pupil=pupil)
            elif kind == "Grid Sag":  # run.py:154-164
                plan["phase_map"] = (_sag_map_once(it["grid_sag"], it["nx"], it["ny"], it["delx"], it["dely"],
                                                   it["xdec"], it["ydec"], n, dxs[i], dys[i]), wls[i])
            elif kind == "PSD":  # run.py:166-177
                # (the draws are taken here, in the reference's order; the screen itself is built when the surface is
                # launched: on the device where the context can -- _launch_phase_maps)
                plan["phase_map"] = (PsdScreen((n, n), dxs[i], dys[i], it["A"], it["B"], it["C"], it["fknee"], it["fmin"],
                                               it["fmax"], it["SR"], it["units"]), wls[i])
    plans.summary()
    return plans


def _surface_gates(items):
    """Mt, Ms, fl, T, n1n2 of one surface for every item -- the quantities run.py:181-190 reads off the
    surface's ABCD matrices (fl = cout / power, inf for a powerless surface; T = cout * thickness)."""
    Mt, fl, T, n1n2 = zip(*[it["ABCDt"].gates() for it in items])
    Ms = [it["ABCDs"].M for it in items]
    return Mt, Ms, fl, T, n1n2


# The same for the columns of ABCD objects the walk has gathered anyway, as arrays, remembered per column: the batches of a
# sweep or of a Monte-Carlo study meet the SAME matrix objects at every step (parse_config's, shared by the shallow copies
# inject_wfe makes), and asking 2 x 256 objects per surface again was a tenth of the host's time per step at 256 wavefronts.
# An entry is valid while the column holds the very same objects (list equality on objects without __eq__ is identity, at C
# speed) and no matrix has been edited in place since (abcd.EPOCH).
_GATE_COLUMNS = {}


def _gate_arrays(col_t, col_s):
    key = (id(col_t[0]), id(col_s[0]), len(col_t))
    hit = _GATE_COLUMNS.get(key)
    if hit is not None and hit[0] == _abcd.EPOCH[0] and hit[1] == col_t and hit[2] == col_s:
        return hit[3]
    Mt, fl, T, n1n2 = zip(*[a.gates() for a in col_t])
    arrays = tuple(np.array(v, dtype=np.float64) for v in (Mt, [a.M for a in col_s], fl, T, n1n2))
    if len(_GATE_COLUMNS) >= 1024:
        _GATE_COLUMNS.clear()
    _GATE_COLUMNS[key] = (_abcd.EPOCH[0], list(col_t), list(col_s), arrays)
    return arrays


_RAY_COLUMNS = {}


def _ray_matrices(col_t, col_s):
    """The (batch, 2, 2) stacks of a surface's ABCD matrices, remembered per column like ``_gate_arrays``."""
    key = (id(col_t[0]), id(col_s[0]), len(col_t))
    hit = _RAY_COLUMNS.get(key)
    if hit is not None and hit[0] == _abcd.EPOCH[0] and hit[1] == col_t and hit[2] == col_s:
        return hit[3]
    arrays = (np.array([a() for a in col_t], dtype=np.float64), np.array([a() for a in col_s], dtype=np.float64))
    if len(_RAY_COLUMNS) >= 1024:
        _RAY_COLUMNS.clear()
    _RAY_COLUMNS[key] = (_abcd.EPOCH[0], list(col_t), list(col_s), arrays)
    return arrays


def _identity_gates(item):
    """The surface's ABCD matrices do nothing to the field: Mt = Ms = 1, fl = inf, T = 0, n1n2 = 1 (run.py:181-207)."""
    Mt, fl, T, n1n2 = item["ABCDt"].gates()
    return Mt == 1.0 and item["ABCDs"].M == 1.0 and math.isinf(fl) and T == 0.0 and n1n2 == 1.0


def _inert(item):
    """A surface that does nothing to the field whatever the beam: no aperture, no stop, no phase, and identity ABCD
    matrices (zero thickness, no power, unit magnification, no change of medium) -- the image plane right behind a slit,
    a coordinate break.  (What run.py:181-207 would gate on: Mt = Ms = 1, fl = inf, T = 0, n1n2 = 1.)"""
    if item.get("aperture") is not None or item.get("is_stop") or item["type"] in ("Zernike", "Grid Sag", "PSD"):
        return False
    return _identity_gates(item)


def _live_rows_after(plans, live, n):
    """Rows that may be non-zero after the stand-alone apertures of ``plans`` were applied: a clear
    aperture (not an obscuration) leaves exact zeros outside its bounding box (photutils' box,
    widened by a pixel here).  ``live`` is updated in place, one [lo, hi) per item."""
    if plans.ap is not None:
        plans.ap.narrow_rows(live, n)


def _live_cols_of(plans, n):
    """Per item the columns [lo, hi) outside which a clear aperture leaves exact zeros (like ``_live_rows_after`` for the
    rows), or None when some item has no such aperture."""
    return plans.ap.live_cols(n) if plans.ap is not None else None


def _launch_apertures(dev, plans):
    """The surface's apertures as stand-alone kernels: one call per shape, enable = 0 for the items of the other."""
    if plans.ap is None:
        return
    blocks, codes = plans.ap.blocks()
    for code in (_lib.SHAPE_ELLIPSE, _lib.SHAPE_RECT):
        mine = plans.ap.on & (codes == float(code))
        if mine.any():
            b = blocks.copy()
            b[~mine] = 0.0
            dev.aperture(code, b)



def _zernike_tables(plans):
    """(zs, nmax, kdim, table, build) of a surface's Zernike plans: ``build(coeffs)`` forms the [batch][stride] parameter
    blocks of paos_zernike from per-item coefficient vectors."""
    zs = [p["zernike"] for p in plans]
    nmax = max(int(z["n"].max()) for z in zs if z is not None)
    kdim = nmax // 2 + 1
    stride = _lib.ZERNIKE_HEAD + 2 * (nmax + 1) * kdim
    table = jacobi_recurrence(nmax)

    def build(coeffs):
        blocks = np.zeros((len(plans), stride), dtype=np.float64)
        # (items of a sweep share polynomial tables and coefficients and differ in the header only -- sampling, radius,
        # wavelength: the coefficient planes are formed once per distinct (tables, coefficients) and copied)
        planes = {}
        for i, z in enumerate(zs):
            if z is None:
                continue
            c = np.asarray(coeffs[i], dtype=np.float64)
            key = (id(z["m"]), id(z["n"]), id(z["norm"]), c.tobytes(), z["origin"])
            hit = planes.get(key)
            if hit is None:
                hit = planes[key] = zernike_block(z["m"], z["n"], z["norm"], c, 1.0, 1.0, 1.0, 1.0, origin=z["origin"], nmax=nmax)[0]
            if not (np.isfinite(z["radius"]) and z["radius"] > 0):
                raise ValueError(f"Zernike radius must be finite and > 0, got {z['radius']}")
            row = blocks[i]
            row[:] = hit
            row[1], row[2], row[3], row[7] = z["dx"], z["dy"], z["radius"], 1.0 / z["wl"]
        return blocks

    return zs, nmax, kdim, table, build


def _launch_zernike(dev, plans, want_wfe=False, same_as=None):
    if isinstance(plans, _Plans) and not plans.summary()[1]:
        return None
    if not any(p["zernike"] is not None for p in plans):
        return None
    zs, nmax, kdim, table, build = _zernike_tables(plans)
    ortho = [z is not None and z["pupil"] is not None for z in zs]
    coeffs = [z["Z"] if z is not None else None for z in zs]
    if not any(ortho):
        if same_as is not None:  # (the items named hold copies of one field: the surface right behind the start)
            return dev.zernike(nmax, kdim, table, build(coeffs), want_wfe=want_wfe, same_as=same_as)
        return dev.zernike(nmax, kdim, table, build(coeffs), want_wfe=want_wfe)

    # PolyOrthoNorm (zernike.py:320-402): U = M Z, so sum_k c_k U_k = sum_n (M^T c)_n Z_n -- the
    # ordinary expansion with transformed coefficients, restricted to the pupil.
    live = [z for z in zs if z is not None]
    if not all(ortho[i] for i, z in enumerate(zs) if z is not None):
        raise NotImplementedError("a batch must use Zorthonorm on all of its items or on none")
    if any(not (np.array_equal(z["m"], live[0]["m"]) and np.array_equal(z["n"], live[0]["n"])
                and np.array_equal(z["norm"], live[0]["norm"])) for z in live):
        raise NotImplementedError("batched Zorthonorm surfaces must share index range, ordering and normalisation")
    for code, is_ellipse in ((_lib.SHAPE_ELLIPSE, True), (_lib.SHAPE_RECT, False)):
        ap = np.zeros((len(plans), _lib.APERTURE_STRIDE), dtype=np.float64)
        for i, z in enumerate(zs):
            if z is not None and isinstance(z["pupil"], EllipticalAperture) == is_ellipse:
                ap[i] = z["pupil"].block(obscuration=False)
        if ap[:, 0].any():  # items of the other shape keep enable = 0 and are left alone
            dev.pupil_aperture(code, ap)
    k = len(live[0]["m"])
    sums, counts = dev.zernike_gram(nmax, kdim, table, build(coeffs), gram_polynomials(live[0]["m"], live[0]["n"],
                                                                                      live[0]["norm"]), pupil=True)
    for i, z in enumerate(zs):
        if z is not None:
            coeffs[i] = orthonorm_matrix(sums[i], counts[i], k).T @ np.asarray(z["Z"], dtype=np.float64)
    return dev.zernike(nmax, kdim, table, build(coeffs), want_wfe=want_wfe, pupil=True)


def _launch_phase_maps(dev, plans, wfe):
    """Grid Sag / PSD surfaces (run.py:154-177): each item's host-built WFE map multiplies its field
    (paos_phase_map).  Returns what the surface's ``wfe`` entry holds for a single wavefront: the map
    of the LAST of Zernike / Grid Sag / PSD (each assignment at run.py:143,156,168 overwrites)."""
    if isinstance(plans, _Plans) and not plans.summary()[2]:
        return wfe
    groups = {}  # items that carry the very same map object (round 5: _sag_map_once): one upload for all of them
    for i, p in enumerate(plans):
        if p["phase_map"] is not None:
            m, wl = p["phase_map"]
            if isinstance(m, PsdScreen):  # a random screen of this item's own
                if _phase_maps.psd_on_device(dev, m.args[0][0]):
                    # fft2 -> power-law filter -> ifft2 -> roughness on the library's passes (paos_psd_screen); the map stays on
                    # the device and comes back only where the reference returns it (one wavefront: the surface's `wfe`)
                    serial = next(_MAP_SERIAL)
                    out = dev.psd_screen(m.noise, m.rough, m.params, key=serial, want_map=len(plans) == 1)
                    dev.phase_map_items(None, [i], [wl], key=serial)
                    if len(plans) == 1:
                        wfe = np.ma.masked_array(out, mask=np.zeros(out.shape, dtype=bool))
                    p["phase_map"] = None  # (its two draws: 2 x 8 n^2 bytes per item)
                    continue
                m = m.host_map()  # complex64 contexts: the screen is built in doubles on the host
                p["phase_map"] = None
            groups.setdefault(id(m), (m, [], []))
            groups[id(m)][1].append(i)
            groups[id(m)][2].append(wl)
            if len(plans) == 1:
                # (a map _sag_map_once keeps is handed out as a copy: the caller owns what run() returns, like the reference's)
                wfe = m.copy() if any(hit[2] is m for hit in _SAG_MAPS.values()) else m
    for m, idx, wls in groups.values():
        if len(idx) > 1 and hasattr(dev, "phase_map_items"):
            filled = _FILLED_MAPS.get(id(m))
            if filled is None or filled[0] is not m:
                if len(_FILLED_MAPS) >= 2:
                    _FILLED_MAPS.pop(next(iter(_FILLED_MAPS)))
                filled = _FILLED_MAPS[id(m)] = (m, np.ascontiguousarray(np.ma.filled(m, 0.0), dtype=np.float64), next(_MAP_SERIAL))
            # (the key under which the library keeps the copy on the device: a serial number given to this map object when it was
            # first sent -- never the object's id, which the allocator hands out again once an evicted map has been freed)
            dev.phase_map_items(filled[1], idx, wls, key=filled[2])
        else:
            for i, wl in zip(idx, wls):
                dev.phase_map(i, np.ma.filled(m, 0.0), wl)
    return wfe


_FILLED_MAPS = {}  # id(map) -> (map, its zero-filled contiguous copy: what crosses PCIe, serial number = the library's content key)


def _queue_apertures(comp, plans):
    """Apertures as pass operators (their weight maps are rendered right before the pass
    they ride on, csrc/passes.hip: launch_one_pass)."""
    if plans.ap is not None:
        comp.aperture(plans.ap.blocks())


def _queue_steps(comp, lens, stw, ptp, wts, inv_stw, inv_wts):
    """Lens and stw / ptp / wts of one surface go to the pass compiler, in the fixed slot
    order every regime respects (OI: stw, ptp; IO: ptp, wts; OO: stw, wts; II: ptp --
    wfo.py:560-570).  Blocks are [batch][5] arrays with enable = 0 where an item skips the step.
    Nothing is launched here: consecutive surfaces fuse (passes.py)."""
    comp.lens(lens)
    comp.stw(stw, inv_stw != 0.0)
    comp.ptp(ptp)
    comp.wts(wts, inv_wts != 0.0)


def _given(**kw):
    """The keywords that are not None: a device call names only those that apply."""
    return {k: v for k, v in kw.items() if v is not None}


def _enqueue_power(dev, rows=None, like=None, cols=None):
    """Enqueue sum |u|^2 of every item; returns the ticket.  ``rows`` (and ``cols`` with them): only these may be non-zero,
    the others are not read; ``like``: per item the index of an item that holds the same field."""
    if rows is None:
        return dev.norm2_enqueue()
    if cols is not None:
        return dev.norm2_enqueue(rows, same_as=like, live_cols=cols)
    return dev.norm2_enqueue(rows, **_given(same_as=like))


def _start_field(dev, fs, plans, value, lean, may_defer):
    """The wavefront is still the constant ``value`` (wfo.py:118) at the first surface that does something.  When every
    item opens with a stand-alone aperture of one shape, ones -> aperture -> [make_stop] is a single write of the field
    (paos_start) -- in a lean walk inside the aperture's rows only, the others left standing for zeros (paos_start_rows),
    and with ``START_BOX`` inside its columns as well.  Returns (True, copies): the surface's aperture and stop are done,
    ``copies`` names per item the first item with the same field (None: all differ).  Otherwise fill, and (False, None):
    the surface runs as usual.  ``may_defer``: a box start is not launched but left as ``lean.deferred_start``."""
    code = plans.ap.start_shape() if plans.ap is not None else None
    if code is None:
        dev.fill(value)
        return False, None
    rows = cols = None
    if lean is not None and hasattr(dev, "zero_outside_rows"):
        trial = [[0, dev.n] for _ in plans]
        plans.ap.narrow_rows(trial, dev.n)
        # worth it only when every item's aperture leaves whole rows dark
        if all(r[0] > 0 or r[1] < dev.n for r in trial) and all(r[0] < r[1] for r in trial):
            rows = trial
            if START_BOX:  # ... and whole columns: the field is written inside the aperture's box only
                cols = plans.ap.live_cols(dev.n)
    blocks = plans.ap.blocks()[0].tolist()
    stops = [1.0 if p["stop"] else 0.0 for p in plans]
    # which items now hold the same field: same aperture record, stop flag and window
    seen, same_as = {}, []
    for i, (b, st) in enumerate(zip(blocks, stops)):
        key = (tuple(float(x) for x in b), st, tuple(rows[i]) if rows is not None else None,
               tuple(cols[i]) if cols is not None else None)
        same_as.append(seen.setdefault(key, i))
    copies = same_as if len(set(same_as)) < len(same_as) else None
    if may_defer and cols is not None:  # (launched later: _launch_start, a Zernike surface may ride on the write)
        lean.deferred_start = dict(value=value, code=code, blocks=blocks, stops=stops, rows=rows, cols=cols, like=copies)
    else:
        dev.start(value, code, blocks, stops, **_given(write_rows=rows, write_cols=cols))
    _live_rows_after(plans, fs.live, dev.n)
    fs.stale, fs.stale_cols = rows is not None, cols if rows is not None else None
    return True, copies


class _WalkState:
    """What ``on_saved`` may want to know about the field at a saved surface of a lean walk:
    ``rows`` -- per item [lo, hi) outside which the field is zero (or stands for zero), or None;
    ``psf_ticket`` -- set when the pass program that ended at this surface has already written |u|^2 to the
    PSF buffer and enqueued its sum (the field itself is then undefined);
    ``same_as`` -- per item the index of an item whose field is known to be identical (the first surface of a sweep:
    the start field does not depend on the wavelength), or None."""

    def __init__(self):
        self.rows, self.psf_ticket, self.same_as = None, None, None
        self.cols = None  # with ``rows``: the columns outside which those rows stand for zeros as well (the start box)
        # set once a pass program has stored the PSF for good (nothing but inert surfaces follows): the saved surfaces
        # still to come report this ticket's power, and the PSF is already where keep_psf wants it
        self.final_ticket = None
        # a dict while the start field of the walk has not been launched yet (it waits for the surface behind it, whose Zernike
        # phase may ride on the write): ``on_saved`` leaves the reduction that will hold the start field's power under "power"
        self.deferred_start = None


class _FieldState:
    """What the walk knows about the fields in memory:
    ``live`` -- per item the rows [lo, hi) outside which the field is exactly zero: set by stand-alone apertures, kept by
    what multiplies (stops, Zernike, phase screens), skipped by the next pass program and forgotten once it has run;
    ``stale`` -- the rows outside ``live`` hold old data that stands for zeros (lean start), as do, with ``stale_cols``,
    the columns outside these [lo, hi) per item (paos_start_box);
    ``dead`` -- the field has been given up for its PSF (lean end): nothing may run on it any more;
    ``twins`` -- per item the index of an item whose field is a copy of its own (None: nothing known);
    ``power`` -- the ticket of the power of the field a pass program has just stored (``flush(final_power=True)``)."""

    def __init__(self, n, batch):
        self.n, self.live = n, [[0, n] for _ in range(batch)]
        self.stale, self.stale_cols, self.dead, self.twins, self.power = False, None, False, None, None

    def known_rows(self):
        return [list(r) for r in self.live] if any(r[0] > 0 or r[1] < self.n for r in self.live) else None

    def stale_cols_for(self, rows):
        """The columns that go with ``rows`` (``known_rows()``, or None) for somebody who reads those rows only."""
        return self.stale_cols if (self.stale and rows is not None) else None

    def settle(self, dev):
        """Before anything reads whole fields: rows that stand for zeros become zeros."""
        if self.stale:
            if self.stale_cols is not None:
                dev.zero_outside_rows(self.live, self.stale_cols)
            else:
                dev.zero_outside_rows(self.live)
            self.stale, self.stale_cols = False, None

    def flush(self, dev, comp, lean, ledger, final_intensity=False, final_power=False):
        """Run what the compiler has queued.  ``final_intensity``: the last pass stores the PSF instead of the field, which
        is given up; ``final_power``: it sums |u|^2 while it stores the field (paos_run_program: final_intensity = 2) -- the
        surface reached is saved (or a stop) and nothing but the program touches its field first, so no sweep has to read
        the field back.  Returns the number of passes run."""
        if self.dead:
            comp.program()  # drop what was queued behind the PSF store
            return 0
        rows = self.known_rows()
        if not comp.pending():
            return 0
        store = True if final_intensity else (2 if final_power else False)
        if store == 2 and ledger is not None:
            ledger.make_room()  # (the ticket is taken inside)
        out = comp.flush(dev, live_rows=rows, rows_stale=self.stale and rows is not None, final_intensity=store,
                         live_cols=self.stale_cols_for(rows))
        done, ticket = out if store else (out, None)
        if final_intensity:
            lean.psf_ticket = lean.final_ticket = ticket
            self.dead = True
        elif final_power:
            self.power = ticket if done else None
        if done:  # the program has written every row and column: nothing stands for zeros, nothing is known to be zero
            self.stale, self.stale_cols = False, None
            for r in self.live:
                r[0], r[1] = 0, self.n
        return done


def _zernike_rides(d, plans, items, n, pending):
    """May this surface's Zernike phase be applied while the deferred start field ``d`` is written?  Every item carries
    an ordinary Zernike expansion whose unit disk lies inside the start's box, nothing else of the surface comes in
    front of it (aperture, stop), nothing is queued (``pending``), and nobody wants the wfe map."""
    any_stop, any_zern, _, any_ap = plans.summary()
    if not any_zern or any_stop or any_ap or pending or (len(plans) == 1 and bool(items[0]["save"])):
        return False
    for p, rows, cols in zip(plans, d["rows"], d["cols"]):
        z = p["zernike"]
        if z is None or z["pupil"] is not None or not (z["radius"] > 0 and z["dx"] > 0 and z["dy"] > 0):
            return False
        hx, hy = z["radius"] / z["dx"], z["radius"] / z["dy"]
        if not (cols[0] <= n // 2 - hx and n // 2 + hx <= cols[1] - 1 and
                rows[0] <= n // 2 - hy and n // 2 + hy <= rows[1] - 1):
            return False
    return True


def _launch_start(dev, lean, plans=None, items=None, pending=True):
    """Launch the deferred start field -- with the Zernike phase of ``plans`` on it when that is possible (True: the
    surface's Zernike is done), else as the walk would have launched it at the first surface."""
    d, lean.deferred_start = lean.deferred_start, None
    power = d.get("power")
    if plans is not None and _zernike_rides(d, plans, items, dev.n, pending):
        zs, nmax, kdim, table, build = _zernike_tables(plans)
        slot = dev.start_zernike(d["value"], d["code"], d["blocks"], d["stops"], d["rows"], d["cols"], nmax, kdim, table,
                                 build([z["Z"] for z in zs]), power=power is not None)
        if power is not None:
            power.slot = int(slot)
        return True
    dev.start(d["value"], d["code"], d["blocks"], d["stops"], write_rows=d["rows"], write_cols=d["cols"])
    if power is not None:
        power.slot = int(_enqueue_power(dev, d["rows"], d["like"], d["cols"]))
    return False


def _walk(dev, states, chains, on_saved, stats=None, fresh=None, lean=None, psf_at=None, ledger=None):
    """Drive all items through their chains in lock-step, one surface at a time.  ``fresh``: the
    constant the field is meant to hold but has not been filled with yet (see _start_field).
    ``lean`` (a _WalkState, optional): the caller reads no arrays at saved surfaces, only powers (through
    ``lean.rows`` / ``lean.psf_ticket``) -- the walk may then leave dead rows unwritten at the start and, when
    ``psf_at`` names the last surface, have the last pass store the PSF instead of the field.  ``ledger`` (a
    ``_PowerLedger``, optional): the power a pass program sums while it stores a saved surface's field is offered there."""
    _SAG_SEEN.clear()  # (a Grid Sag array is hashed once per walk, not once per item)
    keys = [list(c.keys()) for c in chains]
    if any(k != keys[0] for k in keys[1:]):
        raise ValueError("batched chains must list the same surfaces (same keys, same order)")
    st0 = states[0]
    if any((st.pupil_diameter, st.gridsize, st.zoom) != (st0.pupil_diameter, st0.gridsize, st0.zoom) for st in states):
        raise ValueError("the wavefronts of a batch share beam diameter, grid and zoom")
    beams = BeamBatch(st0.pupil_diameter, [st.wavelength for st in states], st0.gridsize, st0.zoom)
    state, n = beams.state, beams.n
    comp = (SeparableCompiler if _passes.SEPARABLE else PassCompiler)(len(states), dev.n)
    fs = _FieldState(dev.n, len(states))
    npass = fused_start = 0  # fused_start: the first field was written with the Zernike phase of the next surface on it
    factor_cols_t, factor_cols_s = [], []  # [surface][item] ABCD factors met so far (run.py:215-219)
    rays = _Rays([st.field for st in states])  # the paraxial rays of every item

    # from which surface on nothing touches the field any more (index into keys[0]; len = never)
    order = keys[0]
    inert_from = len(order)
    while inert_from > 0 and all(_inert(c[order[inert_from - 1]]) for c in chains):
        inert_from -= 1
    for pos, key in enumerate(order):
        items = [c[key] for c in chains]
        if ledger is not None:
            ledger.decline()  # (an offer belongs to its surface: taken for a stop on a surface nobody saved)
        dxs, dys, wls = state[:, beams.DX].tolist(), state[:, beams.DY].tolist(), state[:, beams.WL].tolist()
        readout = []

        def wz_dtf():
            if not readout:
                readout.extend(beams.readout())
            return readout

        plans = _plan_surface(items, n, dxs, dys, wls, lambda i: wz_dtf()[0][i], rays)
        # (the ray-transfer factors met so far, one column per surface; a saved surface gets its product -- lazily)
        col_t, col_s = [it["ABCDt"] for it in items], [it["ABCDs"] for it in items]
        factor_cols_t.append(col_t)
        factor_cols_s.append(col_s)
        saved = any(it["save"] for it in items)
        if saved:  # push_results scalars (run.py:12-27) are those BEFORE magnification / lens / propagate
            # ... and so is the chief ray: behind this surface's coordinate break, before its ABCD matrices (run.py:209-210)
            plans.chief_ray = rays.chief()
            wz, dtf = wz_dtf()
            fr, props, ext = state[:, beams.FRATIO].tolist(), beams.propagators(), beams.extents()
            for i, (it, p) in enumerate(zip(items, plans)):
                if it["save"]:
                    p["scalars"] = {"wz": float(wz[i]), "distancetofocus": float(dtf[i]), "fratio": fr[i],
                                    "dx": dxs[i], "dy": dys[i], "wl": wls[i], "extent": ext[i],
                                    "propagator": props[i]}
                    p["ABCDt"] = ABCDProduct(tuple(col[i] for col in factor_cols_t))
                    p["ABCDs"] = ABCDProduct(tuple(col[i] for col in factor_cols_s))
        # the pilot beams of the whole batch (one C call) and the rays of each item through this surface
        lens, stw, ptp, wts, inv_stw, inv_wts = beams.surface(*_gate_arrays(col_t, col_s))
        rays.advance(col_t, col_s)
        # (a start field that waited for this surface: written now, with this surface's Zernike phase on it if that may be)
        zernike_done = (lean is not None and lean.deferred_start is not None
                        and _launch_start(dev, lean, plans, items, comp.pending()))
        fused_start += zernike_done
        if fresh is not None and not saved and all(_inert(it) for it in items):
            # (coordinate breaks in front of the first mirror: the field is still the constant it will be filled with;
            # the first surface that does something -- usually aperture + stop -- then writes it in one go, _start_field)
            continue
        any_stop, any_zern, any_map, any_ap = plans.summary()
        started, like = False, None  # like: the copies among the fields, for ``on_saved`` (``lean.same_as``)
        if fresh is not None:
            value, fresh = fresh, None
            # still copies of each other unless this surface puts a wavefront error on them
            untouched = not (any_zern or any_map)
            # A box start with nothing else on its surface and a surface behind it waits for that surface: if it is a Zernike
            # surface, the field is written once with the phase on it (_launch_start).  Nothing reads the field meanwhile: a
            # lean walk's saved surface wants its power only, which the deferred launch brings along.
            may_defer = (FUSE_START and untouched and hasattr(dev, "start_zernike") and pos + 1 < len(order)
                         and not (psf_at is not None and key == psf_at) and all(_identity_gates(it) for it in items))
            started, copies = _start_field(dev, fs, plans, value, lean, may_defer)
            if started:
                # (round 5) they stay copies until something wavelength-dependent is applied or queued: a Zernike surface
                # right behind the start (SYN20's S02) reads one field per group of them (paos_zernike_like)
                like, fs.twins = (copies if untouched else None), (copies if TWIN_FIELDS else None)
        if not started:
            fuse_ap = FUSE_APERTURES
            own_breaker = saved or any_stop or any_zern or any_map
            if fuse_ap == "auto":
                # an aperture followed on its own surface by a stop / Zernike / save could only ride
                # on a transform-free pass: the stand-alone aperture kernel is cheaper there
                # -- unless the previous propagation left a pass open: then the aperture becomes the
                # last operator of that pass (applied while the tile is stored) at no extra traffic
                fuse_ap = (plans.ap is not None and (not own_breaker or comp.open_takes_mask()) and
                           plans.ap.fits_line_records(dev.n, dev.precision))
            if fuse_ap:
                _queue_apertures(comp, plans)
            breaker = own_breaker or (any_ap and not fuse_ap)
            if breaker:
                # the field must be current before a non-fusable operator -- unless all this surface wants of it is the
                # PSF of every item (a lean walk's last, saved surface with nothing else on it): then the last pass
                # stores |u|^2 instead
                only_saved = (saved and all(it["save"] for it in items) and
                              not (any_stop or any_zern or any_map or (any_ap and not fuse_ap)))
                # ... the last surface -- or a surface behind which only inert ones follow (the image plane right behind a
                # saved slit): what the program stores here is what the chain ends with
                # (only when this surface has no steps of its own: its lens / propagation would act on the field the inert
                # surfaces receive -- a last mirror or lens some distance in front of the image plane)
                ends_here = key == psf_at or (INERT_TAIL and pos + 1 >= inert_from and psf_at == order[-1] and
                                              all(_identity_gates(it) for it in items))
                as_psf = (lean is not None and psf_at is not None and ends_here and only_saved and comp.pending()
                          and not fs.dead)
                # a stop right behind the program needs the power of what the program stores; a saved surface whose
                # field IS what the program stores reports it
                stop_rides = (STOP_FROM_PROGRAM and any_stop and comp.pending() and not fs.dead and
                              not (any_ap and not fuse_ap))
                npass += fs.flush(dev, comp, lean, ledger, final_intensity=as_psf,
                                  final_power=(not as_psf and comp.pending() and not fs.dead and
                                               (stop_rides or (ledger is not None and only_saved))))
            if not fuse_ap and any_ap:
                _launch_apertures(dev, plans)
                if not comp.pending():
                    _live_rows_after(plans, fs.live, dev.n)
            post = None
            if any_stop:
                fs.settle(dev)
                flags = [1.0 if p["stop"] else 0.0 for p in plans]
                if fs.power is not None:  # the program's last pass has summed the power on its way out
                    dev.make_stop(flags, power_known=True, defer=STOP_DEFERRED)
                    # should the surface be saved: the power BEHIND the stop is P (1 / sqrt P)^2 where the stop applies
                    post = lambda v, f=np.array(flags): np.where(f != 0.0, v * (1.0 / np.sqrt(v)) ** 2, v)
                else:
                    dev.make_stop(flags)
            if fs.power is not None:  # what the program has summed: this surface's to report, if somebody asks
                if ledger is not None:
                    ledger.offer(fs.power, post)
                else:
                    dev.norm2_release(fs.power)
                fs.power = None
            if fs.twins is not None and (comp.pending() or fuse_ap or any_ap or any_stop):
                fs.twins = None  # (something has been applied to the fields, or waits to be)
        # what is left of the surface, whichever way its aperture and stop were done
        wfe = None if zernike_done else _launch_zernike(dev, plans, want_wfe=len(plans) == 1 and bool(items[0]["save"]),
                                                        same_as=fs.twins)
        if any_zern or any_map:
            fs.twins = None
        wfe = _launch_phase_maps(dev, plans, wfe)
        if saved:
            if lean is None:
                fs.settle(dev)
            else:
                # The saved LAST surface of a lean walk that keeps its PSFs, reached without a pass program having stored
                # them (a single-surface chain; every hop shorter than lambda / 1000): ``on_saved`` then takes |u|^2 of the
                # WHOLE field (paos_psf_keep / paos_psf_keep_power), so rows that merely stand for zeros have to be zeros
                # first (the PSF and its power came out NaN on the model device)
                if psf_at is not None and key == psf_at and lean.psf_ticket is None:
                    fs.settle(dev)
                lean.rows = fs.known_rows() if not comp.pending() else None
                lean.cols, lean.same_as = fs.stale_cols_for(lean.rows), like
            on_saved(key, items, plans, wfe)
            if lean is not None:
                lean.rows, lean.psf_ticket, lean.cols, lean.same_as = None, None, None, None
        _queue_steps(comp, lens, stw, ptp, wts, inv_stw, inv_wts)
        if comp.pending():
            fs.twins = None
            if lean is not None and lean.deferred_start is not None:
                _launch_start(dev, lean)  # (the surface has queued something after all: the field must exist first)
    if ledger is not None:
        ledger.decline()  # (taken for a stop on the last surface, which nobody saved)
    if lean is not None and lean.deferred_start is not None:
        _launch_start(dev, lean)
    if fresh is not None:  # an empty chain still yields the initial wavefront
        dev.fill(fresh)
    npass += fs.flush(dev, comp, lean, ledger)
    fs.settle(dev)
    if stats is not None:
        stats["fused_passes"] = npass
        stats["fused_start"] = fused_start


# One idle single-wavefront context per (grid, precision, device) is kept between run() calls:
# creating and destroying one (HBM, pinned staging, twiddles) costs ~7 ms, several times the
# propagation of a small grid.  A context is either in the pool or in use by exactly one call, so
# concurrent run() calls from several threads each get their own.
_IDLE_CONTEXTS = {}
_IDLE_LOCK = threading.Lock()


def _borrow_context(n, precision, device):
    with _IDLE_LOCK:
        dev = _IDLE_CONTEXTS.pop((n, precision, device), None)
    return dev if dev is not None else _lib.DeviceFields(n, 1, precision, device)


def _return_context(dev, n, precision, device):
    with _IDLE_LOCK:
        if (n, precision, device) not in _IDLE_CONTEXTS:
            _IDLE_CONTEXTS[(n, precision, device)] = dev
            return
    dev.close()


def release_contexts():
    """Free the idle contexts kept by run() (also done at interpreter exit)."""
    with _IDLE_LOCK:
        devs = list(_IDLE_CONTEXTS.values())
        _IDLE_CONTEXTS.clear()
    for dev in devs:
        dev.close()


atexit.register(release_contexts)


def run(pupil_diameter, wavelength, gridsize, zoom, field, opt_chain, precision="fp64", device=0):
    """Drop-in for ``paos.core.run.run``: same arguments, same returned dict
    ``{num: {aperture, [wfe], amplitude, wz, distancetofocus, fratio, phase, dx, dy, wfo,
    wl, extent, propagator, ABCDt, ABCDs}}`` for surfaces with ``save`` set."""
    assert isinstance(opt_chain, dict), "opt_chain must be a dict"
    retval = {}
    state = _Item(pupil_diameter, wavelength, gridsize, zoom, field)
    dev = _borrow_context(int(gridsize), precision, device)

    def on_saved(key, items, plans, wfe):
        item, plan = items[0], plans[0]
        rec = {"aperture": plans.aperture(0)}
        if isinstance(wfe, np.ma.MaskedArray):  # Grid Sag / PSD: the host-built map itself
            rec["wfe"] = wfe
        elif wfe is not None:
            outside = np.isnan(wfe)
            rec["wfe"] = np.ma.MaskedArray(data=np.where(outside, 0.0, wfe), mask=outside,
                                           fill_value=0.0)
        s = plan["scalars"]
        rec.update({
            "amplitude": dev.download(0, _lib.WHAT_AMPLITUDE),
            "wz": s["wz"], "distancetofocus": s["distancetofocus"], "fratio": s["fratio"],
            "phase": dev.download(0, _lib.WHAT_PHASE),
            "dx": s["dx"], "dy": s["dy"],
            "wfo": dev.download(0, _lib.WHAT_FIELD),
            "wl": s["wl"], "extent": s["extent"], "propagator": s["propagator"],
        })
        rec["_plan"] = plan  # ABCDs are attached once the surface is fully processed
        retval[item["num"]] = rec

    try:
        _walk(dev, [state], [opt_chain], on_saved, fresh=1.0 + 0.0j)
        dev.sync()
    except BaseException:
        dev.close()  # whatever state it is in, it does not go back to the pool
        raise
    _return_context(dev, int(gridsize), precision, device)
    for rec in retval.values():
        plan = rec.pop("_plan")
        rec["ABCDt"] = deepcopy(plan["ABCDt"])
        rec["ABCDs"] = deepcopy(plan["ABCDs"])
    return retval


def _need_saved_last(chains, last_key, who):
    """Every product of the last surface asks for this first -- before anything is launched."""
    if last_key is None or not all(chain[last_key]["save"] for chain in chains):
        raise ValueError(f"{who} the last surface of the chain to be saved")


def _plan_wavefront(wavefront, chains, nb, sync):
    """Every check of ``wavefront`` -- before anything is launched.  Returns {chain key: the WavefrontFit asked for there}."""
    if wavefront is None:
        return {}
    from .wavefront import WavefrontFit

    requests = [wavefront] if isinstance(wavefront, WavefrontFit) else wavefront
    try:
        requests = list(requests)
    except TypeError:
        raise ValueError(f"wavefront must be a paos_amd.WavefrontFit or a sequence of them, got {wavefront!r}") from None
    at = {}
    for wf in requests:
        if not isinstance(wf, WavefrontFit):
            raise ValueError(f"wavefront must be a paos_amd.WavefrontFit or a sequence of them, got {wf!r}")
        if not sync:
            raise ValueError("wavefront synchronises: it cannot be combined with sync=False")
        wf.check(nb)
        if wf.surfaces is None:
            keys = [key for key in chains[0] if any(key in chain and chain[key]["save"] for chain in chains)]
        else:
            keys = []
            for num in wf.surfaces:
                hit = [key for key, item in chains[0].items() if item["num"] == num]
                if not hit or not all(hit[0] in chain and chain[hit[0]]["num"] == num and chain[hit[0]]["save"] for chain in chains):
                    raise ValueError(f"wavefront: surface {num!r} is not a saved surface of every chain")
                keys.append(hit[0])
        for key in keys:
            if key in at:
                raise ValueError(f"wavefront: two requests name surface {chains[0][key]['num']!r}")
            at[key] = wf
    return at


def _plan_focus(states, chains, focus_planes, last_key):
    """Every check of ``focus_planes`` -- on the scalars alone, so before anything is launched: the pilot beams are taken
    through the chain the way ``_walk`` takes them (one planner call per surface), the field is not.  Returns (the
    BeamBatch as the whole chain leaves it, the defocus values in the caller's order)."""
    try:
        planes = [float(dz) for dz in focus_planes]
    except TypeError:
        raise ValueError("focus_planes must be a sequence of defocus values in metres") from None
    if not all(math.isfinite(dz) for dz in planes):
        raise ValueError("focus_planes must be finite")
    if len(set(planes)) != len(planes):
        raise ValueError("focus_planes must be distinct")
    _need_saved_last(chains, last_key, "focus_planes need")
    keys = [list(c.keys()) for c in chains]
    if any(k != keys[0] for k in keys[1:]):
        raise ValueError("batched chains must list the same surfaces (same keys, same order)")
    st0 = states[0]
    beams = BeamBatch(st0.pupil_diameter, [st.wavelength for st in states], st0.gridsize, st0.zoom)
    for key in keys[0]:
        items = [c[key] for c in chains]
        beams.surface(*_gate_arrays([it["ABCDt"] for it in items], [it["ABCDs"] for it in items]))
    n, state = beams.n, beams.state
    for i in range(len(states)):
        wl, dx, dy = (float(state[i, k]) for k in (beams.WL, beams.DX, beams.DY))
        if state[i, beams.C] != 0.0:
            raise ValueError(f"focus_planes: the wavefront of item {i} is not planar behind the last surface "
                             f"(C = {float(state[i, beams.C])!r}); PTP wavefront should be planar")
        limit = min(n * dx * dx / wl, n * dy * dy / wl)
        for dz in planes:
            if dz != 0.0 and abs(dz) < 0.001 * wl:
                raise ValueError(f"focus_planes: |dz| = {abs(dz)!r} m is below a thousandth of item {i}'s wavelength "
                                 f"({wl!r} m): the reference would skip that plane")
            if abs(dz) > limit:
                raise ValueError(f"focus_planes: |dz| = {abs(dz)!r} m exceeds N d^2 / wl = {limit!r} m of item {i}: "
                                 "the plane would be aliased")
    return beams, planes


# The products of the last surface -- a blur of the kept PSFs (blur.PsfBlur), their energy curves (energy.EnergyProfile),
# pointing series (pointing.PointingSeries; with weights: _SeriesSumRequest), detector images, transfer functions, zoomed
# windows (zoom.PsfWindow) -- share one
# method: ``attach(dev, recs, dxs, dys)`` gives ``recs[i]`` item i's entries from what ``dev`` holds right now (the kept
# PSFs: ``reads_psf``, or the field) on the samplings ``dxs`` / ``dys``.  ``_attach_products`` walks them.
class _DetectorRequest:
    """The kept PSFs rebinned onto ``detector`` (paos_detector_*): added into the accumulator of ``dev`` with ``weights``
    (no record is touched), else every record gets its item's image.  ``origins``: every item's grid centre in the image
    plane (None: the origin); with ``chief`` the chief rays at the last surface, which ``on_saved`` fills in there."""

    reads_psf = True

    def __init__(self, detector, weights, origins, chief):
        self.detector, self.weights, self.origins, self.chief = detector, weights, origins, chief

    def attach(self, dev, recs, dxs, dys):
        if getattr(dev, "detector", None) != self.detector:
            dev.detector_begin(self.detector)
        placed = {} if self.origins is None else {"origins": self.origins}  # (paos_detector_*_placed)
        if self.weights is not None:
            dev.detector_add(dxs, dys, self.weights, **placed)
        else:
            for rec, image in zip(recs, dev.detector_images(dxs, dys, **placed)):
                rec["detector"] = image


class _SeriesSumRequest:
    """A pointing series added, with ``weights`` ((B,) or (B, T)), into the broadband sum of ``dev`` (paos_series_sum_*;
    ``pointing.PointingSeries.add_to_sum``): no record is touched and nothing synchronises."""

    reads_psf = True

    def __init__(self, pointing, weights):
        self.pointing, self.weights = pointing, weights

    def attach(self, dev, recs, dxs, dys):
        self.pointing.add_to_sum(dev, self.weights, dxs, dys)


class _OtfRequest:
    """What ``run_batch`` hands out of the transfer functions of the kept PSFs: the full arrays named in ``arrays``
    ('mtf', 'otf') and, with ``cuts``, the two MTF cuts with their frequency axes."""

    reads_psf = True

    def __init__(self, arrays, cuts, compute=True):
        # compute=False: a blur attached before this request has transformed the PSFs already (blur.PsfBlur.attach), and
        # the spectra ``dev`` holds are the system transfer functions
        self.arrays, self.cuts, self.compute = tuple(arrays), bool(cuts), bool(compute)

    def __bool__(self):
        return bool(self.arrays) or self.cuts

    def attach(self, dev, recs, dxs, dys):
        """``recs[i]`` gets item i's entries, from the PSFs ``dev`` keeps right now.  Synchronises."""
        if self.compute:
            dev.otf_compute()
        for i, rec in enumerate(recs):
            for name in self.arrays:
                rec[name] = dev.otf_fetch(i, name)
        if self.cuts:
            cuts = dev.otf_cuts()
            m = np.arange(dev.n // 2 + 1, dtype=np.float64)
            for i, rec in enumerate(recs):
                rec["mtf_x"], rec["mtf_y"] = cuts[i, 0].copy(), cuts[i, 1].copy()
                rec["freq_x"], rec["freq_y"] = m / (dev.n * dxs[i]), m / (dev.n * dys[i])


def _attach_products(dev, products, recs, dxs, dys, plane_power=None):
    """Every product's entries onto ``recs``: first those that read the kept PSFs, then those that read the field.
    ``plane_power`` (None: the nominal records -- the walk has kept the PSFs, the ledger has the powers): ``recs`` are a
    focus plane's, whose PSFs are kept here first if a product reads them and whose power, if wanted, is summed along."""
    from_psf = [p for p in products if p.reads_psf]
    ticket = None
    if plane_power is not None:
        if from_psf and plane_power:
            ticket = dev.psf_keep_power()
        elif from_psf:
            dev.psf_keep()
        elif plane_power:
            ticket = dev.norm2_enqueue()
    for p in from_psf:
        p.attach(dev, recs, dxs, dys)
    if ticket is not None:
        for rec, power in zip(recs, dev.norm2_fetch(ticket)):
            rec["power"] = float(power)
    for p in products:
        if not p.reads_psf:
            p.attach(dev, recs, dxs, dys)


_WHAT = {"psf": _lib.WHAT_INTENSITY, "wfo": _lib.WHAT_FIELD, "amplitude": _lib.WHAT_AMPLITUDE, "phase": _lib.WHAT_PHASE}


def _focus_stack(dev, focus, outputs, metrics_radii_px, power, products):
    """The planes of ``focus`` (``_plan_focus``) from the field ``dev`` holds behind the walk: [item][plane] dicts, planes in
    the caller's order.  The nominal plane (dz = 0) is read first, from the untouched field; then one ``focus_begin`` and
    one ``focus_plane`` per other plane (paos_focus_plane leaves the plane in the field).  Every plane's dict gets the
    arrays named in ``outputs``, its metrics, its power and the entries of ``products``."""
    (beams, planes), nb = focus, dev.batch
    state = beams.state
    z0 = state[:, beams.Z].copy()
    wls, dxs, dys = (state[:, k].tolist() for k in (beams.WL, beams.DX, beams.DY))
    stacks = [[None] * len(planes) for _ in range(nb)]
    opened = False
    try:
        for k in sorted(range(len(planes)), key=lambda k: planes[k] != 0.0):  # (stable: the nominal plane first)
            dz = planes[k]
            if dz != 0.0:
                if not opened:
                    dev.focus_begin()
                    opened = True
                blocks = [[1.0, 1.0 / (beams.n * dxs[i]), 1.0 / (beams.n * dys[i]), (np.pi * wls[i] * dz), -1.0]
                          for i in range(nb)]  # (PilotBeam.ptp's block: wfo.py:462-472)
                dev.focus_plane(blocks)
            state[:, beams.Z] = z0 + dz
            try:
                wz, dtf = beams.readout()
                zs = state[:, beams.Z].tolist()
            finally:
                state[:, beams.Z] = z0
            recs = [{"dz": dz, "z": zs[i], "distancetofocus": float(dtf[i]), "wz": float(wz[i])} for i in range(nb)]
            for i, rec in enumerate(recs):
                for name in outputs:
                    rec[name] = dev.download(i, _WHAT[name])
                stacks[i][k] = rec
            if metrics_radii_px is not None:
                for rec, met in zip(recs, dev.psf_metrics(metrics_radii_px)):
                    rec["metrics"] = met
            _attach_products(dev, products, recs, dxs, dys, plane_power=bool(power))
    finally:
        if opened:
            dev.focus_end()
    return stacks


def run_batch(pupil_diameter, wavelengths, gridsize, zoom, field, opt_chains, precision="fp64",
              device=0, outputs=("psf",), dev=None, sync=True, stats=None, metrics_radii_px=None,
              keep_psf=False, power=True, detector=None, detector_weights=None, detector_origin=None, focus_planes=None,
              mtf_cuts=False, psf_zoom=None, psf_blur=None, psf_energy=None, wavefront=None, pointing=None,
              pointing_weights=None):
    """Propagate ``B = len(opt_chains)`` wavefronts together on one GPU.

    ``wavelengths[i]`` / ``opt_chains[i]`` describe wavefront ``i`` (chains must
    contain the same surfaces).  ``field`` is one field point ``{'us': slope_x, 'ut': slope_y}`` for every
    wavefront, or a sequence of one such dict per wavefront (a field-of-view study in one batch); slopes must be
    finite (``ValueError`` otherwise, and for a sequence of another length).  Returns a list of ``B`` dicts
    ``{num: {scalars..., 'power': sum|u|^2, ['psf'], ['wfo'], ['amplitude'], ['phase']}}``
    for saved surfaces (with ``sync=False`` the power is left as ``'power_ticket'``, a :class:`PowerTicket`:
    ``ticket.fetch()[i]`` -- or ``dev.norm2_fetch(ticket)[i]`` -- is item i's power; records whose powers come from one
    reduction share one handle state, so every record may be fetched, in any order, any number of times).  ``outputs`` picks which N x N arrays are copied back to the
    host per saved surface and item ('psf' = |u|^2, plot.py:125-130); ``()`` keeps
    every array on the GPU and returns scalars and the power only -- the mode the
    throughput benchmark uses.  ``metrics_radii_px`` (up to 16 radii, pixels) adds
    ``'metrics'`` = power, centroid, peak and encircled power per radius of |u|^2 computed on
    the GPU (about the grid centre) -- what a Monte-Carlo encircled-energy study needs, without
    moving a PSF.  ``keep_psf`` writes |u|^2 of every item at the LAST surface of the chain (when it
    is saved) into the context's device-resident PSF buffer (``dev.psf_fetch(i)`` reads one back):
    the final intensity write of a run whose PSFs stay in HBM.  ``power=False`` skips the sum |u|^2
    reduction per saved surface (the reference does not return it; chains that save a dozen
    surfaces spend 7 % of their time there).  ``dev`` may pass a pre-allocated
    ``DeviceFields(gridsize, B)`` to reuse across calls.

    ``detector`` (a :class:`paos_amd.detector.Detector`) rebins every item's PSF at the LAST surface of the chain, which
    must be saved (``ValueError`` otherwise), onto that detector pixel grid on the GPU (README.md, "Detector images"; it
    implies ``keep_psf``).  With ``detector_weights`` (one per item) ``w_i A_i`` is added, item after item, into the
    accumulator of ``dev`` (``dev.detector_fetch()`` reads it; a ``dev`` that is not on that detector yet is started
    there, ``dev.detector_begin``): nothing synchronises.  Without weights each item's record of the last surface gets
    ``'detector'``, its image ``A_i`` as a (ny, nx) float64 array.  ``detector_origin`` says where each item's grid
    centre lies in the image plane: None puts every one at the origin (the detector's ``(xc, yc)`` are then measured
    from the grid centre); ``"chief_ray"`` puts item i's at its chief ray ``(vs_i[0], vt_i[0])`` at the last surface,
    behind that surface's coordinate break and before its ABCD matrices (the point its apertures are centred on, so
    ``(xc, yc)`` are measured from the optical axis); a (B, 2) array gives the positions ``(x0_i, y0_i)`` in metres.

    ``focus_planes`` (K distinct finite defocus values in metres, positive along the propagation direction) adds a
    through-focus stack behind the LAST surface, which must be saved (README.md, "Through-focus stacks"): with u_i, wl_i,
    dx_i, dy_i and the pilot beam (z, zw0, zr, C) of item i as everything the last surface does leaves them, plane ``dz`` is
    ``ifft2(exp(-i pi wl_i dz (fx^2 + fy^2)) fft2(u_i))`` -- ``WFO.ptp(dz)``, wfo.py:445-472, ortho norms, ``fx, fy`` from
    ``np.fft.fftfreq(N, dx_i)`` / ``(N, dy_i)`` -- on the unchanged sampling, at ``z + dz``.  The chain is walked once and
    the forward transform is done once (``paos_focus_begin``); a plane costs one inverse 2-D transform
    (``paos_focus_plane``).  The nominal records are what they are without the keyword; the last surface's record of each
    item additionally gets ``'focus'``, a list of K dicts in the order given: ``dz``, ``z``, ``distancetofocus``, ``wz``
    (the planner's formulas at ``z + dz``), ``power`` (unless ``power=False``), the arrays named in ``outputs``,
    ``'metrics'`` with ``metrics_radii_px`` and ``'detector'`` (the plane's image ``A_i``) with a detector.  ``dz == 0.0`` is
    served from the untouched last-surface field, before any other plane is computed.  ``ValueError``, before anything is
    launched: a last surface that is not saved; values that are not finite or not distinct; an item whose wavefront is not
    planar behind the last surface (``C != 0``, the reference's own precondition, wfo.py:458-460); ``0 < |dz| < wl_i /
    1000`` (the reference would skip that ``ptp``, wfo.py:454, for some items of a batch and not for others);
    ``|dz| > N dx_i^2 / wl_i`` or ``N dy_i^2 / wl_i`` (beyond it the transfer function's phase steps by more than pi
    between neighbouring frequency samples at the band edge: the plane would be aliased); ``detector_weights`` (what the
    accumulator should hold across planes is ambiguous).  The reference's ``propagate`` switches to ``wts`` and rescales
    the grid once ``|z + dz - zw0| >= 2 zr`` (wfo.py:280-302, 547-572); a focus stack keeps ``ptp`` and the
    detector-plane sampling on purpose -- inside ``2 zr`` the two coincide.  The planes synchronise (their powers are
    fetched as they are made); afterwards the field of ``dev`` holds the last plane computed and, with a detector, its
    PSF buffer that plane's PSF.

    ``'mtf'`` / ``'otf'`` in ``outputs`` and ``mtf_cuts=True`` hand out the transfer functions of every item's PSF at the
    LAST surface, which must be saved (README.md, "Transfer functions"; computed on the GPU from the kept PSFs by a packed
    real-input transform, ``paos_otf_compute``; any of the three implies ``keep_psf``): ``'mtf'`` a (N, N) float64 array
    ``|OTF|`` and ``'otf'`` the (N, N) complex128 OTF, zero frequency at pixel [N/2][N/2] and exactly 1 there, attached to
    the last surface's record only; ``mtf_cuts`` gives that record ``'mtf_x'``, ``'mtf_y'`` -- the MTF along ``fy = 0, fx
    >= 0`` and along ``fx = 0, fy >= 0``, N/2 + 1 values each from zero frequency to Nyquist, fetched for the whole batch
    in one small copy -- and ``'freq_x'``, ``'freq_y'`` = ``m / (N dx_i)``, ``m / (N dy_i)`` in cycles per metre with the
    item's sampling at the last surface.  ``outputs=()`` with ``mtf_cuts=True`` runs on the lean walk.  With
    ``focus_planes`` every plane's dict gets the same keys (through-focus MTF); the ``dz == 0.0`` plane's arrays equal the
    nominal record's bit for bit.  They synchronise: with ``sync=False`` any of the three is a ``ValueError``, as is a last
    surface that is not saved -- before anything is launched.

    ``psf_zoom`` (a :class:`paos_amd.PsfWindow`) adds a window of every item's PSF at the LAST surface, which must be
    saved, on a grid ``oversample`` times finer (README.md, "Zoomed PSFs"): the exact band-limited interpolant of the
    field, ``|Wy u Wx^T|^2`` with real Dirichlet-kernel weights, contracted on the GPU by the fp64 matrix instruction
    (``paos_zoom_compute``).  The last surface's record gets ``'psf_zoom'`` (size x size float64, samples of the same
    intensity as ``'psf'``, not divided by ``oversample^2``), ``'zoom_dx'``, ``'zoom_dy'`` (``dx_i / oversample``,
    ``dy_i / oversample``), ``'zoom_centre'`` (the window's centre ``(x, y)`` in pixels; fine sample ``[size/2][size/2]``
    lies there) and, with ``field=True``, ``'wfo_zoom'`` (complex128).  Fine samples that fall on grid pixels equal the
    field's samples bit for bit; a window that runs over the grid edge wraps.  With ``focus_planes`` every plane's dict
    gets the same keys.  It needs the field of the last surface, so the run takes the ordinary walk, and it synchronises:
    ``sync=False``, a last surface that is not saved, a size, oversampling or centres that ``paos_zoom_compute`` would
    refuse are a ``ValueError`` -- before anything is launched.

    ``psf_blur`` (a :class:`paos_amd.PsfBlur`) blurs every item's kept PSF at the LAST surface, which must be saved, on
    the GPU (README.md, "Blurred PSFs"; it implies ``keep_psf``): ``P' = ifft2(T fft2(P))`` with the separable transfer
    function of a Gaussian (jitter, charge diffusion) and, optionally, the pixel aperture on the item's sampling at the
    last surface -- ``paos_otf_compute``, then ``paos_blur_apply`` in place on the PSF buffer.  It is attached first, so
    everything made from the kept PSFs is made from ``P'``: ``'detector'`` images and the accumulator of
    ``detector_weights``, and ``'mtf'`` / ``'otf'`` / ``mtf_cuts``, which are then the SYSTEM transfer functions (the
    PSFs are transformed once for both).  The last surface's record gets ``'blur_sigma'`` = ``(sigma_x_i, sigma_y_i)``
    and, with ``array=True``, ``'psf_blur'``, ``P'`` as a (N, N) float64 array read from the PSF buffer.  What is read
    from the FIELD stays optical: ``'psf'`` (and the other arrays of ``outputs``), ``'metrics'``, ``'power'`` and
    ``psf_zoom``.  With ``focus_planes`` every plane is treated alike; ``outputs=()`` stays on the lean walk.
    ``ValueError``, before anything is launched: an argument that is not a ``PsfBlur``; a last surface that is not saved;
    ``sync=False``; per-item values of another length than the batch; ``pixel`` together with ``detector`` (the rebinning
    already integrates over the pixel).

    ``psf_energy`` (a :class:`paos_amd.EnergyProfile`) adds the encircled energy of every item's kept PSF at the LAST
    surface, which must be saved, computed on the GPU (README.md, "Encircled energy"; it implies ``keep_psf``): up to
    1024 radii ``(b + 1) step`` in metres at the image plane (or pixels), each item about its own centre -- the grid
    centre, given positions, or the centroid or the peak, which are formed on the device between the sweep that sums the
    PSF and the launch that bins it (``paos_ee_compute``; one small copy, ``paos_ee_fetch``).  The last surface's record
    gets ``'ee_radius'``, ``'ee'`` (the power inside each circle, not normalised), ``'ensq'`` with ``square=True``,
    ``'ee_total'``, ``'ee_centre'`` ``(x, y)`` in pixels, ``'ee_peak'`` ``(value, (col, row))``, ``'ee_fallback'`` and
    ``'ree'``, the radii at which ``'ee'`` reaches the requested fractions of ``'ee_total'`` (NaN where it does not).  It
    reads the kept PSFs: behind ``psf_blur`` the curves are those of ``P'``, ``outputs=()`` stays on the lean walk, and
    with ``focus_planes`` every plane's dict gets the same keys, each plane about its own centre (the ``dz == 0.0``
    plane's equal the nominal record's bit for bit).  ``ValueError``, before anything is launched: an argument that is
    not an ``EnergyProfile``; a last surface that is not saved; ``sync=False``; centres of another shape than (B, 2) or
    outside ``[0, N)``.  An item whose largest circle would be wider or taller than the grid (``bins step / dx_i`` or
    ``bins step / dy_i`` above ``N / 2``) is a ``ValueError`` that names it, raised before the curves are computed.

    ``wavefront`` (a :class:`paos_amd.WavefrontFit`, or a sequence of them: surfaces with different beam sizes need
    different radii) fits Zernike polynomials to the phase of every item's field at the saved surfaces a request names
    (all of them with ``surfaces=None``), on the GPU (README.md, "Wavefront fits": ``paos_wavefront_fit``; one small copy
    per surface, ``paos_wavefront_fetch``).  Each such record gets ``'wf_coeff'`` (metres, one per term), ``'wf_rms'``,
    ``'wf_residual_rms'``, ``'wf_pv'`` (metres), ``'wf_strehl'``, ``'wf_pixels'``, ``'wf_phase_absmax'`` (radians),
    ``'wf_fallback'`` and ``'wf_singular'``.  It needs the field, so the run takes the ordinary walk, like
    ``metrics_radii_px``; focus planes get nothing.  ``ValueError``, before anything is launched: an argument that is not
    a ``WavefrontFit``; ``sync=False``; a named surface that is not a saved surface of every chain; two requests that
    name the same surface; per-item values of another length than the batch.

    ``pointing`` (a :class:`paos_amd.PointingSeries`) adds the time series of a moving line of sight from every item's
    kept PSF at the LAST surface, which must be saved, made on the GPU (README.md, "Pointing series"; it implies
    ``keep_psf``): for each of its T offsets the PSF is rebinned onto the series' own detector with the item's grid centre
    at origin + offset, multiplied by the pixel response and summed inside its boxes of detector pixels in a fixed order
    (``paos_series_compute``; the fluxes come back in one copy, ``paos_series_fetch``).  The last surface's record gets
    ``'series_flux'`` (T, A), ``'series_offsets'`` (T, 2) and, with ``frames=True``, ``'series_frames'`` (T, ny, nx), each
    frame equal to the ``'detector'`` image placed there bit for bit (times the response).  It reads the kept PSFs: it is
    attached behind ``psf_blur`` and ``psf_energy`` (behind a blur the frames are those of ``P'``), ``outputs=()`` stays on
    the lean walk, and with ``focus_planes`` every plane's dict gets the same keys (the ``dz == 0.0`` plane's equal the
    nominal record's bit for bit).  It is independent of ``detector``, ``detector_weights`` and ``detector_origin``: the
    series carries its own detector and origin, and their results do not change by a bit.  ``ValueError``, before anything
    is launched: an argument that is not a ``PointingSeries``; ``sync=False``; a last surface that is not saved; per-item
    offsets or an origin array for another batch size; ``psf_blur`` with a ``pixel`` aperture (the rebinning already
    integrates over the pixel).

    ``pointing_weights`` ((B,) or (B, T) finite numbers) turns ``pointing`` into a contribution to a broadband series
    (README.md, "Broadband series"): instead of per-item records, every item's frames are added, weighted, into the sum
    that the caller's ``dev`` keeps in device memory, ``S[t] += w[i][t] F_i[t]`` in item order (``paos_series_sum_add``;
    the sum is opened, ``dev.series_sum_begin``, when ``dev`` has none for this detector and T).  No record is touched and
    nothing synchronises, so ``sync=False`` is allowed; the caller reads ``dev.series_sum_flux(boxes, response)`` and
    ``dev.series_sum_fetch()`` when the sweep is done (the response, the apertures and ``frames`` of ``pointing`` play no
    part in the add).  Behind ``psf_blur`` it reads ``P'``; ``origin="chief_ray"`` resolves as above.  ``ValueError``,
    before anything is launched: weights without ``pointing``; weights without a caller-owned ``dev``; a wrong shape or
    non-finite weights; ``focus_planes`` (what the sum should hold across planes is ambiguous); ``psf_blur`` with a
    ``pixel`` aperture.
    """
    nb = len(opt_chains)
    if len(wavelengths) != nb:
        raise ValueError("one wavelength per chain is required")
    if nb == 0:
        return []
    unknown = set(outputs) - set(_WHAT) - {"mtf", "otf"}
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")
    last_key = list(opt_chains[0].keys())[-1] if len(opt_chains[0]) else None
    # the transfer functions of the last surface's PSFs: not arrays of the field (they are not downloaded per saved surface)
    otf = _OtfRequest([name for name in ("mtf", "otf") if name in outputs], mtf_cuts, compute=psf_blur is None)
    outputs = tuple(name for name in outputs if name not in ("mtf", "otf"))
    if psf_blur is not None:
        from .blur import PsfBlur

        if not isinstance(psf_blur, PsfBlur):
            raise ValueError(f"psf_blur must be a paos_amd.PsfBlur, got {psf_blur!r}")
        if not sync:
            raise ValueError("psf_blur cannot be combined with sync=False")
        _need_saved_last(opt_chains, last_key, "psf_blur needs")
        psf_blur.check(nb)
        if psf_blur.pixel is not None and detector is not None:
            raise ValueError("psf_blur with a pixel aperture and a detector: the rebinning already integrates over the pixel")
    if psf_energy is not None:
        from .energy import EnergyProfile

        if not isinstance(psf_energy, EnergyProfile):
            raise ValueError(f"psf_energy must be a paos_amd.EnergyProfile, got {psf_energy!r}")
        if not sync:
            raise ValueError("psf_energy synchronises: it cannot be combined with sync=False")
        _need_saved_last(opt_chains, last_key, "psf_energy needs")
        psf_energy.check(nb, int(gridsize))
    if pointing is not None:
        from .pointing import PointingSeries

        if not isinstance(pointing, PointingSeries):
            raise ValueError(f"pointing must be a paos_amd.PointingSeries, got {pointing!r}")
        if not sync and pointing_weights is None:
            raise ValueError("pointing synchronises: it cannot be combined with sync=False")
        _need_saved_last(opt_chains, last_key, "pointing needs")
        pointing.check(nb, int(gridsize))
        if pointing_weights is not None:
            pointing_weights = pointing.weights_for(pointing_weights, nb)
            if dev is None:
                raise ValueError("pointing_weights accumulate into `dev`: pass a DeviceFields that outlives the call")
            if focus_planes is not None:
                raise ValueError("focus_planes with pointing_weights: what the sum should hold across planes is ambiguous")
        if psf_blur is not None and psf_blur.pixel is not None:
            raise ValueError("psf_blur with a pixel aperture and a pointing series: the rebinning already integrates over the pixel")
    elif pointing_weights is not None:
        raise ValueError("pointing_weights without pointing")
    wf_at =_plan_wavefront(wavefront, opt_chains, nb, sync)
    if otf:
        if not sync:
            raise ValueError("'mtf' / 'otf' outputs and mtf_cuts synchronise: they cannot be combined with sync=False")
        _need_saved_last(opt_chains, last_key, "'mtf' / 'otf' outputs and mtf_cuts need")
    if psf_zoom is not None:
        from .zoom import PsfWindow

        if not isinstance(psf_zoom, PsfWindow):
            raise ValueError(f"psf_zoom must be a paos_amd.PsfWindow, got {psf_zoom!r}")
        if not sync:
            raise ValueError("psf_zoom synchronises: it cannot be combined with sync=False")
        _need_saved_last(opt_chains, last_key, "psf_zoom needs")
        psf_zoom.check(nb, int(gridsize))
    if detector is not None:
        _need_saved_last(opt_chains, last_key, "a detector needs")
        if detector_weights is not None:
            detector_weights = np.asarray(detector_weights, dtype=np.float64).reshape(-1)
            if detector_weights.size != nb:
                raise ValueError("one detector weight per chain is required")
            if dev is None:
                raise ValueError("detector_weights accumulate into `dev`: pass a DeviceFields that outlives the call")
    elif detector_weights is not None:
        raise ValueError("detector_weights without a detector")
    origins = None
    if detector_origin is not None:
        if detector is None:
            raise ValueError("detector_origin without a detector")
        if isinstance(detector_origin, str):
            if detector_origin != "chief_ray":
                raise ValueError(f"detector_origin must be None, 'chief_ray' or a (B, 2) array, got {detector_origin!r}")
        else:
            origins = np.array(detector_origin, dtype=np.float64)
            if origins.shape != (nb, 2):
                raise ValueError(f"detector_origin must have shape ({nb}, 2), got {origins.shape}")
            if not np.all(np.isfinite(origins)):
                raise ValueError("detector_origin must be finite")
    det = None if detector is None else _DetectorRequest(detector, detector_weights, origins, isinstance(detector_origin, str))
    # (in the order in which they are attached: a blur rewrites the kept PSFs, so it goes before everything that reads them)
    series = pointing if pointing_weights is None else _SeriesSumRequest(pointing, pointing_weights)
    products = [p for p in (psf_blur, psf_energy, series, det, otf, psf_zoom) if p]
    placed_at_chief = [p for p in (det, pointing) if p is not None and p.chief]  # their origins: the chief rays at the last surface
    keep_psf = keep_psf or any(p.reads_psf for p in products)
    fields = _fields_of(field, nb)
    states = [_Item(pupil_diameter, wl, gridsize, zoom, f) for wl, f in zip(wavelengths, fields)]
    focus = None
    if focus_planes is not None:
        if detector_weights is not None:
            raise ValueError("focus_planes with detector_weights: what the accumulator should hold across planes is ambiguous")
        focus = _plan_focus(states, list(opt_chains), focus_planes, last_key)
    own = dev is None
    if own:
        dev = _lib.DeviceFields(int(gridsize), nb, precision, device)
    elif dev.batch != nb or dev.n != int(gridsize):
        raise ValueError("supplied DeviceFields does not match the batch")
    results = [dict() for _ in range(nb)]

    # nobody reads an array at a saved surface: the walk may skip writing dead rows at the start and store the PSF
    # straight from the last pass (csrc/frugal_pass.h: STORE)
    # (a focus stack and a zoomed window need the field of the last surface: the ordinary walk)
    lean = _WalkState() if (not outputs and metrics_radii_px is None and focus is None and psf_zoom is None and not wf_at) else None
    ledger = _PowerLedger(dev)

    def on_saved(key, items, plans, wfe):
        pending = []
        for i, (item, plan) in enumerate(zip(items, plans)):
            if not item["save"]:
                continue
            rec = dict(plan["scalars"])
            rec["aperture"] = plans.aperture(i)
            for name in outputs:
                rec[name] = dev.download(i, _WHAT[name])
            rec["_plan"] = plan
            results[i][item["num"]] = rec
            pending.append((i, rec))
        if metrics_radii_px is not None:
            met = dev.psf_metrics(metrics_radii_px)
            for i, rec in pending:
                rec["metrics"] = met[i]
        if key in wf_at and pending:
            # (an item that does not save here is fitted on the first saving item's sampling, and its result dropped)
            saved = dict(pending)
            scalars = [saved.get(i, pending[0][1]) for i in range(nb)]
            fits = wf_at[key].fit(dev, [sc["dx"] for sc in scalars], [sc["dy"] for sc in scalars], [sc["wl"] for sc in scalars])
            for i, rec in pending:
                rec.update(fits[i])
        keep = keep_psf and key == last_key
        if key == last_key:
            for p in placed_at_chief:
                p.origins = plans.chief_ray
        # the last pass has stored |u|^2 and enqueued its sum -- for this surface, or for good (inert surfaces behind it)
        fused = (lean.psf_ticket if lean.psf_ticket is not None else lean.final_ticket) if lean is not None else None
        if not power:
            if fused is not None:
                ledger.final(fused).release()  # (once, however many surfaces it stands for)
            elif keep:
                dev.psf_keep()
        elif fused is not None:
            ledger.record(fused, pending, final=True)
        else:
            ledger.make_room(spare=1)
            if ledger.offered is not None and not keep:
                ledger.claim(pending)  # the pass that stored this surface's field has summed it
            elif keep:
                # the saved last surface of a run that keeps its PSFs: |u|^2 written and summed in one sweep
                ledger.decline()  # (the kept PSF brings its own sum)
                ledger.record(dev.psf_keep_power(), pending)
            elif lean is not None and lean.deferred_start is not None:
                # the start field is launched at the next surface (_walk: _launch_start), which enqueues this sum and names its slot
                lean.deferred_start["power"] = ledger.record(-1, pending)
            elif lean is not None:
                ledger.record(_enqueue_power(dev, lean.rows, lean.same_as, lean.cols), pending)
            else:
                ledger.record(dev.norm2_enqueue(), pending)

    # The walk allocates a few thousand small containers per surface of a large batch (plans, blocks, handles); a
    # generation-2 pass of the cycle collector in the middle of it costs as much as planning several surfaces (round 5:
    # 10 ms of a 29 ms walk at 256 wavefronts).  Nothing the walk builds is cyclic garbage worth collecting before it
    # ends, so the collector is paused for its duration (and left as it was found).
    gc_was_on = gc.isenabled()
    gc.disable()
    try:
        _walk(dev, states, list(opt_chains), on_saved, stats=stats, fresh=1.0 + 0.0j, lean=lean,
              psf_at=last_key if (keep_psf and lean is not None) else None,
              ledger=ledger if (power and POWER_ON_STORE) else None)
        if products or focus is not None:
            recs = [results[i][opt_chains[i][last_key]["num"]] for i in range(nb)]
            # (before a focus stack, whose planes store their own PSFs and overwrite the field)
            _attach_products(dev, products, recs, [rec["dx"] for rec in recs], [rec["dy"] for rec in recs])
            if focus is not None:
                for rec, stack in zip(recs, _focus_stack(dev, focus, outputs, metrics_radii_px, power, products)):
                    rec["focus"] = stack
        if sync or own:
            ledger.drain()
        else:  # the caller synchronises later
            ledger.hand_out()
    finally:
        if gc_was_on:
            gc.enable()
        if own:
            dev.close()
    for res in results:
        for rec in res.values():
            plan = rec.pop("_plan")
            rec["ABCDt"], rec["ABCDs"] = plan["ABCDt"], plan["ABCDs"]
    return results
