"""Worker of tests/test_gpu_aperture_xprec.py::test_generic_pass_at_1024_with_the_production_kernels_switched_off: device code
that has to run in a process of its own, because the library reads PAOS_NO_FRUGAL once."""
import numpy as np

import aperture_xprec as ax


def no_frugal_worker(out):
    """Runs in a fresh process (the library reads PAOS_NO_FRUGAL once): the riding geometries at 1024^2 on the generic
    pass kernel, mask in the pre, mid and post slot around a disabled transform, both axes, against the render path's weights of
    the same context bit for bit.  Puts ("ok", passes checked) or ("fail", message) on ``out``."""
    import os

    try:
        os.environ["PAOS_NO_FRUGAL"] = "1"
        from paos_amd import _lib

        n, batch, value = 1024, 4, 1.0 + 0.5j
        dev = _lib.DeviceFields(n, batch)
        try:
            checked = 0
            for axis in (0, 1):
                geoms = ax.frugal_ellipses(n, axis)
                for k in (0, 4):
                    items = geoms[k:k + batch]
                    blocks = np.zeros((3, batch, 5))  # the aperture's two block sets and a disabled transform's control block
                    want = []
                    for i, (xc, yc, a, b, obsc) in enumerate(items):
                        blocks[0, i] = [1.0, xc, yc, a, b]
                        blocks[1, i] = [0.0, obsc, 0.0, float(_lib.SHAPE_ELLIPSE), 0.0]
                        m = dev.aperture_mask(_lib.SHAPE_ELLIPSE, [1.0, xc, yc, a, b, 0.0, 0.0, 0.0])
                        w = (1.0 - m) if obsc else m
                        want.append(w * value.real + 1j * (w * value.imag))
                    for slot in ("pre", "mid", "post"):
                        p = {"axis": axis, "fft1": 2, "fft2": -1, "pre": [], "mid": [], "post": []}
                        p[slot] = [(_lib.PW_MASK, 0, 0)]
                        dev.fill(value)
                        dev.run_passes([p], blocks)
                        for i in range(batch):
                            if not np.array_equal(dev.download(i), want[i]):
                                out.put(("fail", f"axis {axis} {slot} item {i} {items[i]}: not the rendered weights"))
                                return
                        checked += 1
            if dev.record_set_stats() != (0, 0):
                out.put(("fail", f"line records were used under PAOS_NO_FRUGAL=1: {dev.record_set_stats()}"))
                return
            out.put(("ok", checked))
        finally:
            dev.close()
    except Exception as exc:  # noqa: BLE001 -- the parent reports it
        out.put(("fail", repr(exc)))
