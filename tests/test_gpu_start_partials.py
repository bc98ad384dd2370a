"""GPU test of the kept power partials of the fused start (csrc/paos_hip.hip: start_body): with a power ticket,
paos_start_zernike_box sums the power of the start field from the aperture weights (start_norm2_partial_kernel); the
per-workgroup sums are kept with everything they depend on -- shape, constant, aperture records, stop flags, row windows,
rounded column windows, which items lead a sum -- and the next start with the same key skips the kernel.  The final
reduction runs every time, so a found power is the same bits.  One context goes through a sequence of starts that change one
of those things at a time; after each, the field (inside the box, and NaN as before outside it) and the fetched power equal
those of a fresh context bit for bit."""
import numpy as np
import pytest

import start_partials_worker as worker

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fresh():
    """{name: (fields, powers)} of every start on a context of its own: computed once."""
    from paos_amd import _lib

    zargs, out = worker.zernike_args(), {}
    for name, start in worker.starts().items():
        dev = _lib.DeviceFields(worker.N, worker.NB)
        try:
            out[name] = worker.fused_start(dev, start, zargs)
        finally:
            dev.close()
    return out


def test_starts_on_one_context_equal_fresh_contexts(fresh):
    """The same start twice (the second finds both kept sums), another row window, another column window, one that rounds to
    the same columns, another aperture, two start groups in the batch, other stop flags, another constant, the first again."""
    from paos_amd import _lib

    starts, zargs = worker.starts(), worker.zernike_args()
    dev = _lib.DeviceFields(worker.N, worker.NB)
    try:
        for k, name in enumerate(worker.SEQUENCE):
            fields, power = worker.fused_start(dev, starts[name], zargs)
            want_fields, want_power = fresh[name]
            print(k, name, "power", [float(p).hex() for p in power], "fresh", [float(p).hex() for p in want_power])
            assert np.array_equal(power, want_power), (k, name, power, want_power)
            rows, cols = starts[name][3], starts[name][4]
            for i in range(worker.NB):
                assert np.array_equal(fields[i], want_fields[i], equal_nan=True), (k, name, i)
                inside = fields[i][rows[i][0]:rows[i][1], cols[i][0]:cols[i][1]]
                assert np.isfinite(inside).all() and np.abs(inside).max() > 0.0 and np.isnan(fields[i][0, 0])
    finally:
        dev.close()
    # the starts are told apart by what they give: the windows and the flags change the power, the rounding does not
    power = {name: fresh[name][1] for name in starts}
    assert power["rows"][0] != power["first"][0] and power["cols"][0] != power["rows"][0]
    assert np.array_equal(power["cols that round alike"], power["cols"])
    assert power["two groups"][2] != power["two groups"][0] and power["flags"][1] != power["two groups"][1]
    assert worker.digest(fresh["constant"])["fields"] != worker.digest(fresh["flags"])["fields"]


def test_without_the_memo_the_same_bits(fresh):
    """PAOS_START_POWER_MEMO=0 (a fresh process: the switch is read once) keeps neither sum: the first start, twice."""
    import multiprocessing as mp

    ctx = mp.get_context("forkserver")  # (the server conftest.py started before this process touched the GPU)
    out = ctx.Queue()
    proc = ctx.Process(target=worker.switched_worker, args=(out, "PAOS_START_POWER_MEMO"))
    proc.start()
    try:
        status, got = out.get(timeout=120)
        proc.join(timeout=60)
    finally:
        if proc.is_alive():  # (a worker that hangs must not stay behind with the GPU open)
            proc.kill()
    assert status == "ok", got
    want = worker.digest(fresh["first"])
    assert got == [want, want]
